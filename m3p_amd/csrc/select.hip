// Word selection of the decoding loops (decoder.py: generate / generate_beam) straight from the bf16 logits of the
// vocabulary GEMM: per row the log-sum-exp, per sentence the k best of its beam * V entries - without an fp32 copy of the
// logits, a log_softmax tensor or a sort.  Each logit is read once.
//
// The score of entry (row r, word w) is  fl32(fl32(float(x[r, w]) - lse[r]) + beam_scores[r]);  a sentence's entries are
// ranked by the total order T: score descending, then beam ascending, then logit descending, then word ascending.
// Inside one row the score is a monotone function of the logit, so T restricted to a row is (logit descending, word
// ascending) - which needs no lse.  Hence the first k entries of a sentence under T lie in the union of every row's
// first k entries under (logit descending, word ascending), and a row's first k lie in the union of its chunks' first k:
//   phase 1  (vs_chunk_kernel, a workgroup per (row, chunk of 4096 columns)): the chunk's maximum, its sum of
//            exp(x - max) and its first k entries as 32-bit keys  (sortable bf16 bits << 16 | 0xFFFF - column in chunk) -
//            one unsigned maximum is "logit descending, column ascending"; k rounds of a block-wide maximum;
//   phase 2  (vs_merge_kernel, a workgroup per sentence): lse of the sentence's rows from the chunks' (max, sum), then k
//            rounds of a block-wide maximum over the beam * chunks * k candidates under T.
// No atomics; sums are added in a fixed order, so results are reproducible bit for bit.
#include "common.hpp"

namespace {

constexpr int VS_CHUNK = 4096;        // columns per workgroup of phase 1: 256 threads x 2 loads x 8 bf16
constexpr int VS_MAX_K = 16;          // entries per sentence (2 * beam of the search loop: beams up to 8)
constexpr int VS_MAX_BEAM = 64;       // rows per sentence (their lse sit in LDS in phase 2)

typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;

// bf16 bits -> u16 whose unsigned order is the order of the values (-0 was folded into +0 by the caller)
__device__ __forceinline__ uint32_t vs_sortable16(uint32_t b) { return (b & 0x8000u) ? (~b & 0xFFFFu) : (b | 0x8000u); }
__device__ __forceinline__ float vs_value16(uint32_t sk) {
  const uint32_t b = (sk & 0x8000u) ? (sk & 0x7FFFu) : (~sk & 0xFFFFu);
  return __uint_as_float(b << 16);
}
__device__ __forceinline__ uint32_t vs_sortable32(float f) {
  const uint32_t b = f == 0.f ? 0u : __float_as_uint(f);       // (-0 and +0 are one score)
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float vs_value32(uint32_t s) { return __uint_as_float((s & 0x80000000u) ? (s & 0x7FFFFFFFu) : ~s); }

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
  return v;
}

// logits bf16 [n, ld]; block (row, chunk) -> pstat[(row * nchunks + chunk) * 2 + {0, 1}] = {max, sum exp(x - max)},
// cand[(row * nchunks + chunk) * k + j] = key of the chunk's j-th entry (0: the chunk holds fewer than j + 1 columns)
__global__ __launch_bounds__(256) void vs_chunk_kernel(const bf16* __restrict__ logits, int ld, int V, int nchunks, int k,
                                                      float* __restrict__ pstat, uint32_t* __restrict__ cand) {
  __shared__ uint32_t red[2][4];
  __shared__ float reds[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int row = blockIdx.x / nchunks, chunk = blockIdx.x % nchunks;
  const unsigned short* base = reinterpret_cast<const unsigned short*>(logits) + (size_t)row * ld + (size_t)chunk * VS_CHUNK;
  // 16 keys per thread; columns at or past V hold anything (NaN, inf) and become the key 0, below every real entry
  uint32_t key[16];
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int lc0 = half * (VS_CHUNK / 2) + tid * 8;
    const int left = V - (chunk * VS_CHUNK + lc0);          // valid columns from lc0 on (ld % 8 == 0: a load that starts below V ends inside the row)
    u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (left > 0) v = *reinterpret_cast<const u16x8*>(base + lc0);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      uint32_t b = v[e];
      if (b == 0x8000u) b = 0;
      key[half * 8 + e] = e < left ? (vs_sortable16(b) << 16 | (uint32_t)(0xFFFF - (lc0 + e))) : 0u;
    }
  }
  uint32_t lm = 0;
#pragma unroll
  for (int e = 0; e < 16; ++e) lm = max(lm, key[e]);
  uint32_t* out = cand + (size_t)blockIdx.x * k;
  for (int j = 0; j < k; ++j) {
    const uint32_t w = wave_max_u32(lm);
    if (lane == 0) red[j & 1][wv] = w;
    __syncthreads();            // (two buffers: round j + 2 writes this one again only behind the barrier of round j + 1)
    const uint32_t win = max(max(red[j & 1][0], red[j & 1][1]), max(red[j & 1][2], red[j & 1][3]));
    if (j == 0) {
      // the first winner carries the chunk's maximum (the chunk starts below V: it holds at least one column)
      const float mx = vs_value16(win >> 16);
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (key[e] != 0u && mx > -INFINITY) s += __expf(vs_value16(key[e] >> 16) - mx);
      s = wave_sum(s);
      if (lane == 0) reds[wv] = s;
      __syncthreads();
      if (tid == 0) {
        pstat[(size_t)blockIdx.x * 2] = mx;
        pstat[(size_t)blockIdx.x * 2 + 1] = (reds[0] + reds[1]) + (reds[2] + reds[3]);
      }
    }
    if (tid == 0) out[j] = win;
    if (lm == win && win != 0u) {       // keys are unique (the column is part of them): one thread holds the winner
      lm = 0;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        key[e] = key[e] == win ? 0u : key[e];
        lm = max(lm, key[e]);
      }
    }
  }
}

struct VsKey {                 // order T as one unsigned comparison of (hi, lo)
  unsigned long long hi;       // sortable score << 32 | 0xFFFF - beam << 16 | sortable logit;  0 = no entry
  uint32_t lo;                 // ~word
};
__device__ __forceinline__ bool vs_less(const VsKey& a, const VsKey& b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }

__global__ __launch_bounds__(256) void vs_merge_kernel(const float* __restrict__ pstat, const uint32_t* __restrict__ cand,
                                                      const float* __restrict__ beam_scores, float* __restrict__ scores,
                                                      long long* __restrict__ flat_idx, float* __restrict__ lse, int V,
                                                      int nchunks, int beam, int k) {
  __shared__ float s_lse[VS_MAX_BEAM];
  __shared__ unsigned long long r_hi[2][4];
  __shared__ uint32_t r_lo[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int sent = blockIdx.x;
  for (int r = wv; r < beam; r += 4) {             // a wave per row: merge the chunks' (max, sum)
    const size_t row = (size_t)sent * beam + r;
    const float* ps = pstat + row * nchunks * 2;
    float m = -INFINITY;
    for (int c = lane; c < nchunks; c += 64) m = fmaxf(m, ps[2 * c]);
    m = wave_max(m);
    float s = 0.f;
    for (int c = lane; c < nchunks; c += 64) {
      const float pm = ps[2 * c];
      if (pm > -INFINITY) s += ps[2 * c + 1] * expf(pm - m);
    }
    s = wave_sum(s);
    const float l = m + logf(s);
    if (lane == 0) {
      s_lse[r] = l;
      lse[row] = l;
    }
  }
  __syncthreads();
  const int per_row = nchunks * k, total = beam * per_row;
  const uint32_t* cs = cand + (size_t)sent * total;
  VsKey bound = {~0ull, ~0u};            // entries strictly below it are still to be had by this thread
  VsKey best;
  auto scan = [&]() {
    best.hi = 0ull;
    best.lo = 0u;
    for (int i = tid; i < total; i += 256) {
      const uint32_t key = cs[i];
      if (key == 0u) continue;
      const int r = i / per_row, c = (i - r * per_row) / k;
      const uint32_t sk = key >> 16;
      const float bsc = beam_scores ? beam_scores[(size_t)sent * beam + r] : 0.f;
      const float sc = (vs_value16(sk) - s_lse[r]) + bsc;
      VsKey x;
      x.hi = (unsigned long long)vs_sortable32(sc) << 32 | (unsigned long long)(uint32_t)(0xFFFF - r) << 16 | sk;
      x.lo = ~(uint32_t)(c * VS_CHUNK + (int)(0xFFFFu - (key & 0xFFFFu)));
      if (vs_less(x, bound) && vs_less(best, x)) best = x;
    }
  };
  scan();
  for (int j = 0; j < k; ++j) {
    VsKey w = best;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      VsKey y;
      y.hi = (unsigned long long)__shfl_xor((long long)w.hi, o, 64);
      y.lo = (uint32_t)__shfl_xor((int)w.lo, o, 64);
      if (vs_less(w, y)) w = y;
    }
    if (lane == 0) {
      r_hi[j & 1][wv] = w.hi;
      r_lo[j & 1][wv] = w.lo;
    }
    __syncthreads();
    VsKey win = {r_hi[j & 1][0], r_lo[j & 1][0]};
#pragma unroll
    for (int q = 1; q < 4; ++q) {
      const VsKey y = {r_hi[j & 1][q], r_lo[j & 1][q]};
      if (vs_less(win, y)) win = y;
    }
    if (tid == 0) {
      const bool have = win.hi != 0ull;       // (the launcher asks for k <= beam * V: always)
      const int r = 0xFFFF - (int)((win.hi >> 16) & 0xFFFFu);
      scores[(size_t)sent * k + j] = have ? vs_value32((uint32_t)(win.hi >> 32)) : -INFINITY;
      flat_idx[(size_t)sent * k + j] = have ? (long long)r * V + (long long)(~win.lo) : 0ll;
    }
    if (best.hi == win.hi && best.lo == win.lo && win.hi != 0ull) {   // (beam, word) is part of the key: one thread
      bound = win;
      scan();
    }
  }
}

int vs_plan(int n, int V, int ld, int beam, int k) {
  if (n <= 0 || V <= 0 || beam <= 0 || k <= 0 || n % beam != 0 || ld < V || (ld % 8) != 0) return M3P_EINVAL;
  if ((long long)beam * V < k) return M3P_EINVAL;
  if (k > VS_MAX_K || beam > VS_MAX_BEAM) return M3P_ENOTIMPL;
  const long long nchunks = ((long long)V + VS_CHUNK - 1) / VS_CHUNK;
  if ((long long)n * nchunks * VS_MAX_K >= (1ll << 31)) return M3P_ENOTIMPL;       // 32-bit block and candidate indices
  return M3P_OK;
}

}  // namespace

extern "C" {

int m3p_vocab_select_max_k(void) { return VS_MAX_K; }

int m3p_vocab_select_plan(int n, int V, int ld, int beam, int k) { return vs_plan(n, V, ld, beam, k); }

size_t m3p_vocab_select_workspace_bytes(int n, int V, int k) {
  if (n <= 0 || V <= 0 || k <= 0) return 0;
  const size_t blocks = (size_t)n * (((size_t)V + VS_CHUNK - 1) / VS_CHUNK);
  return blocks * (2 * sizeof(float) + (size_t)k * sizeof(uint32_t));
}

int m3p_vocab_select(const void* logits, int ld, int n, int V, const float* beam_scores, int beam, int k, void* workspace,
                     size_t workspace_bytes, float* scores, long long* flat_idx, float* lse, void* stream) {
  const int rc = vs_plan(n, V, ld, beam, k);
  if (rc != M3P_OK) return rc;
  if (!logits || !workspace || !scores || !flat_idx || !lse || ((uintptr_t)logits & 15) || ((uintptr_t)workspace & 15)) return M3P_EINVAL;
  if (workspace_bytes < m3p_vocab_select_workspace_bytes(n, V, k)) return M3P_EINVAL;
  const int nchunks = (V + VS_CHUNK - 1) / VS_CHUNK;
  float* pstat = (float*)workspace;
  uint32_t* cand = (uint32_t*)(pstat + (size_t)n * nchunks * 2);
  hipLaunchKernelGGL(vs_chunk_kernel, dim3((unsigned)(n * nchunks)), dim3(256), 0, (hipStream_t)stream, (const bf16*)logits, ld, V,
                     nchunks, k, pstat, cand);
  M3P_CHECK_LAUNCH();
  hipLaunchKernelGGL(vs_merge_kernel, dim3((unsigned)(n / beam)), dim3(256), 0, (hipStream_t)stream, (const float*)pstat,
                     (const uint32_t*)cand, beam_scores, scores, flat_idx, lse, V, nchunks, beam, k);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

}  // extern "C"
