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
//
// Seeded sampling (decoder.py: generate(sample_seed=...); m3p_vocab_sample) draws the next word of every row from
// softmax(float(logit) * inv_t) over an allowed set by Gumbel-max - an exponential race: one pass, no prefix sums, and the
// random number of (row r, word w) is a pure function of (seed, r * V + w), so the NumPy twin (m3p_amd/rng.py: sample_*)
// regenerates the very numbers a launch used:
//   m = m3p_hash32(r * V + w, seed) >> 8        24 bits
//   u = (m + 0.5) * 2^-24                       in (0, 1), never 0 or 1
//   E = -log(u)                                 a unit exponential
//   key(r, w) = float(logit[r, w]) * inv_t - log(E)
// The sampled word is the argmax of key over the allowed set, ties to the lowest word: P(w wins) = softmax(x * inv_t)[w]
// exactly, but for the 24-bit grid of u - log(E) spans [-17.33, 2.85], so a word whose probability is below about 2^-24 of
// the most likely one's is never drawn.  Allowed set: top_k = 0 every word below V; 1 <= top_k <= VS_MAX_K the row's first
// top_k entries under (logit descending, word ascending) - phase 1 of the selection above, run as it is.  Outputs per row:
// the word, logprob = x_w * inv_t - lse_T (lse_T = log-sum-exp of x * inv_t over the allowed set) and the winning key.
// Columns at or past V are never chosen whatever they hold; a -inf logit has key -inf and loses to every finite one.
//   all words  phase 1 (vsmp_chunk_kernel, a workgroup per (row, chunk), the loads of vs_chunk_kernel): per element the
//              hash and a key, the winner by one unsigned maximum of the 64-bit (sortable key << 32 | ~column) - every
//              element gets a cheap approximate key, the few that can still win the accurate one (see the kernel) -; the
//              chunk's winner and its (max, sum exp) of x * inv_t;  phase 2 (vsmp_merge_kernel, a wave per row): the row's winner, lse_T
//              from the chunks' (max, sum), logprob from the winner's own logit.
//   top_k      vs_chunk_kernel with k = top_k, then vsmp_topk_kernel (a wave per row): top_k rounds of a wave-wide maximum
//              over the chunks' candidates, lane j keeps entry j; keys, lse_T and the argmax over those lanes.
// Noise accuracy: E comes from the accurate logf / log1pf (never __logf: near u = 1 the native log's ABSOLUTE error is as
// large as E itself).  u and 1 - u are both exact in fp32 in their own half: m < 2^23 takes logf(u), m >= 2^23 takes
// log1pf(-(1 - u)) with 1 - u = (2^24 - m - 0.5) * 2^-24.  The key is ONE fma (x * inv_t is not rounded on its own).
// __expf in the chunk sums of phase 1, by the argument above restated for y = x * inv_t: what __expf adds to expf is the
// rounding of (y - max) * log2 e, which moves a term by |y - max| * 6e-8 relative at most; terms that matter to the sum lie
// within ln V + a few of the row's maximum WHATEVER inv_t is (a term d below the maximum weighs e^-d), so the sum moves by
// < 1e-6 relative, below the rounding of lse_T itself.  The scale inv_t enters only through the size of lse_T: its fp32
// rounding is |lse_T| * 6e-8, which is why the tests hold logprob to 1e-5 * max(1, max|x| * inv_t / 16).
//
// Nucleus (top-p) sampling (decoder.py: generate(sample_top_p=...); m3p_vocab_nucleus_sample) cuts that allowed set to the
// words whose logit is at least x*, the largest logit value whose cumulated mass reaches top_p - see the block in front of
// vnuc_coarse_kernel; with 1 <= top_k <= 16 the cut is a sum over the lanes of vsmp_topk_kernel<true>.
//
// More than VS_MAX_K candidates (generate(sample_top_k=40 ...); m3p_vocab_sample_wide, 1 <= top_k <= VSW_MAX_K = 1024, with or
// without the nucleus cut) keep that contract - the same counter, keys, tie rule and outputs - but find the candidate set by
// an exact count selection over the 16-bit keys instead of top_k rounds of a maximum, compact it to [n, top_k] entries and
// finish each row in one workgroup in LDS - see the block in front of vsw_coarse_kernel.  The decoding loop sends top_k > 16
// there; nothing leaves the device for any top_k <= 1024.
//
// More than VS_MAX_K entries per sentence (generate_beam with 9 .. 32 beams; m3p_vocab_select_wide, 1 <= k <= VSB_MAX_K = 64)
// keep the contract of the selection at the top - the same lse bits, scores and order T - with that count selection as phase 1
// (vsw_launch_select, shared with the seeded draw) and one sort of a sentence's beam * k entries in LDS as phase 2 - see the
// block in front of vsb_merge_kernel.
//
// Shared pieces, each defined once (the kernels are thin bodies over them):
//   chunk reader   VsChunk / vs_chunk_of_block / vs_chunk_run -> VsRun / vs_slot_column: which columns a thread of workgroup
//                  (row, chunk) owns, the load guard at V, the fold of -0, the sortable key - the seven (row, chunk) kernels
//   histogram      VnHist<T>: 256 bins in replicated LDS copies, zero / add / flush - vnuc_coarse, vnuc_fine, vsw_coarse
//   bin scan       vn_bin_scan: the highest bin at which the value cumulated from the top satisfies a predicate - vnuc_scan,
//                  vnuc_cut, vsw_scan
//   row lse        vs_row_lse: log-sum-exp from the chunks' (max, sum) - vs_merge, vsmp_merge, vsb_merge
//   draw epilogue  vsmp_write_draw (word, logprob, key, cut) and vsmp_merge_row (the body of vsmp_merge and vnuc_merge)
//   host side      vs_nchunks, vsmp_plan (the seeded draws' plan, by the bounds on top_k), vs_args_ok, vsmp_launch_topk,
//                  vsw_launch_select (the count selection's launches) - m3p_vocab_sample_wide, m3p_vocab_select_wide
#include "common.hpp"
#include <math.h>
#include <initializer_list>

namespace {

constexpr int VS_CHUNK = 4096;        // columns per workgroup of phase 1: 256 threads x 2 loads x 8 bf16
constexpr int VS_MAX_K = 16;          // entries per sentence (2 * beam of the search loop: beams up to 8)
constexpr int VS_MAX_BEAM = 64;       // rows per sentence (their lse sit in LDS in phase 2)

int vs_nchunks(int V) { return (int)(((long long)V + VS_CHUNK - 1) / VS_CHUNK); }      // workgroups of phase 1 per row

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

// ------------------------------------------------------------------------------------------------------------------------
// the chunk reader: workgroup (row, chunk) of 256 threads over its VS_CHUNK columns, 16 per thread
// ------------------------------------------------------------------------------------------------------------------------
// Thread tid owns VS_RUNS runs of VS_RUN consecutive columns, a run per half of the chunk (one 16-byte load each, the
// workgroup's loads of a half contiguous): its slot s = run * VS_RUN + e is the chunk's column vs_slot_column(tid, s).  A kernel
// walks  for run: VsRun r = vs_chunk_run(...); for e: ...  with both loops unrolled, so slots index registers.  Columns at or
// past V hold anything (NaN, inf): in(e) is false there and NOTHING else of such a column may reach a result - this guard is the
// only thing that keeps them out.  (Two plain loops in the kernel, not a visitor taking a lambda or one flat loop over the 16
// slots: either compiles several of the kernels to a branch per column where this form gives selects.  For the same reason a
// kernel reads sk(e) in front of its in(e) test, not behind it.)
constexpr int VS_RUNS = 2, VS_RUN = 8;
struct VsChunk {
  int row, chunk;
  const unsigned short* base;                // the chunk's column 0 in the row
};
__device__ __forceinline__ VsChunk vs_chunk_of_block(const bf16* __restrict__ logits, int ld, int nchunks) {
  const int row = blockIdx.x / nchunks, chunk = blockIdx.x % nchunks;
  return {row, chunk, reinterpret_cast<const unsigned short*>(logits) + (size_t)row * ld + (size_t)chunk * VS_CHUNK};
}
__device__ __forceinline__ int vs_slot_column(int tid, int slot) {
  return (slot / VS_RUN) * (VS_CHUNK / VS_RUNS) + tid * VS_RUN + slot % VS_RUN;
}
struct VsRun {
  int lc0, left;                             // the run's first column in the chunk; valid columns from there on (<= 0: none)
  u16x8 v;                                   // the bf16 bits (zeros where the whole run is past V)
  __device__ __forceinline__ int lc(int e) const { return lc0 + e; }                          // column in the chunk
  __device__ __forceinline__ bool in(int e) const { return e < left; }                        // below V
  __device__ __forceinline__ uint32_t raw(int e) const { return v[e]; }                       // the bf16 as loaded
  __device__ __forceinline__ uint32_t bits(int e) const { return v[e] == 0x8000u ? 0u : (uint32_t)v[e]; }      // -0 folded into +0
  __device__ __forceinline__ uint32_t sk(int e) const { return vs_sortable16(bits(e)); }     // the sortable 16-bit key
};
__device__ __forceinline__ VsRun vs_chunk_run(const VsChunk& c, int V, int tid, int run) {
  VsRun r;
  r.lc0 = vs_slot_column(tid, run * VS_RUN);
  r.left = V - (c.chunk * VS_CHUNK + r.lc0);               // (ld % 8 == 0: a load that starts below V ends inside the row)
  r.v = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
  if (r.left > 0) r.v = *reinterpret_cast<const u16x8*>(c.base + r.lc0);
  return r;
}

// the row's (max, sum exp(x - max)) from its chunks' pairs ps[2 c + {0, 1}] -> log-sum-exp, in every lane of the wave.
// also(c): what else the caller has to fetch per chunk c of this lane, riding along the first pass (a loop of its own would
// put one more memory latency into a kernel that is nothing but latency)
template <class F>
__device__ __forceinline__ float vs_row_lse(const float* __restrict__ ps, int nchunks, int lane, F&& also) {
  float m = -INFINITY;
  for (int c = lane; c < nchunks; c += 64) {
    also(c);
    m = fmaxf(m, ps[2 * c]);
  }
  m = wave_max(m);
  float s = 0.f;
  for (int c = lane; c < nchunks; c += 64) {
    const float pm = ps[2 * c];
    if (pm > -INFINITY) s += ps[2 * c + 1] * expf(pm - m);
  }
  s = wave_sum(s);
  return m + logf(s);
}

// logits bf16 [n, ld]; block (row, chunk) -> pstat[(row * nchunks + chunk) * 2 + {0, 1}] = {max, sum exp(x - max)},
// cand[(row * nchunks + chunk) * k + j] = key of the chunk's j-th entry (0: the chunk holds fewer than j + 1 columns)
__global__ __launch_bounds__(256) void vs_chunk_kernel(const bf16* __restrict__ logits, int ld, int V, int nchunks, int k,
                                                      float* __restrict__ pstat, uint32_t* __restrict__ cand) {
  __shared__ uint32_t red[2][4];
  __shared__ float reds[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  // 16 keys per thread; a column at or past V becomes the key 0, below every real entry
  const VsChunk c = vs_chunk_of_block(logits, ld, nchunks);
  uint32_t key[16];
#pragma unroll
  for (int run = 0; run < VS_RUNS; ++run) {
    const VsRun r = vs_chunk_run(c, V, tid, run);
#pragma unroll
    for (int e = 0; e < VS_RUN; ++e) key[run * VS_RUN + e] = r.in(e) ? (r.sk(e) << 16 | (uint32_t)(0xFFFF - r.lc(e))) : 0u;
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
    const float l = vs_row_lse(pstat + row * nchunks * 2, nchunks, lane, [](int) {});
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
  if ((long long)n * vs_nchunks(V) * VS_MAX_K >= (1ll << 31)) return M3P_ENOTIMPL;       // 32-bit block and candidate indices
  return M3P_OK;
}

// ------------------------------------------------------------------------------------------------------------------------
// seeded sampling
// ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long y = (unsigned long long)__shfl_xor((long long)v, o, 64);
    v = y > v ? y : v;
  }
  return v;
}

// log(E) of element idx = row * V + word, E = -log(u), u = (m + 0.5) 2^-24: in [-17.33, 2.85]
__device__ __forceinline__ float vsmp_log_e(uint32_t idx, uint32_t seed) {
  const uint32_t m = m3p_hash32(idx, seed) >> 8;
  // 2 m + 1 < 2^24 in the lower half and 2^25 - 2 m - 1 < 2^24 in the upper half: both conversions and the scaling are exact
  const float E = m >= (1u << 23) ? -log1pf(-((float)((1u << 25) - 2u * m - 1u) * 0x1p-25f))
                                  : -logf((float)(2u * m + 1u) * 0x1p-25f);
  return logf(E);
}
__device__ __forceinline__ unsigned long long vsmp_key64(float key, uint32_t word) {
  return (unsigned long long)vs_sortable32(key) << 32 | (unsigned long long)(~word);
}

// A cheap stand-in for vsmp_log_e, within 0.01 of it: native log2 (v_log_f32), and in the upper half
// log E = log(1 - u) + log(E / (1 - u)) with the series  log(-log(1 - v) / v) = v/2 + 5 v^2/24 + v^3/8 + ...  cut after the
// cube: every further term is positive and at v <= 1/2 they add up to 0.0089; the native log's own error is below 1e-5 here.
__device__ __forceinline__ float vsmp_log_e_approx(uint32_t idx, uint32_t seed) {
  const uint32_t m = m3p_hash32(idx, seed) >> 8;
  const bool up = m >= (1u << 23);
  const float a = (float)(up ? (1u << 25) - 2u * m - 1u : 2u * m + 1u) * 0x1p-25f;     // 1 - u or u, exact
  const float l = __log2f(a) * 0.69314718f;                                             // log(1 - u) or log(u) < 0
  return up ? l + a * (0.5f + a * (5.f / 24.f + a * 0.125f)) : __log2f(-l) * 0.69314718f;
}
constexpr float VSMP_BAND = 0.04f;        // twice a bound (0.02) on |approximate key - key|, the roundings of the keys aside

// logits bf16 [n, ld]; block (row, chunk) -> wkey[block] = (sortable key << 32 | ~word) of the chunk's winner,
// pstat[block * 2 + {0, 1}] = {max, sum exp(y - max)} of y = x * inv_t over the chunk's columns below V.
// Three accurate logarithms per element would make this kernel VALU bound (measured: 152 us at 128 x 250 002 against 25 us
// of vs_chunk_kernel), and all but one or two of a thread's 16 keys cannot win.  So every element gets an APPROXIMATE key
// first (vsmp_log_e_approx: two native logarithms), within d = 0.02 + |key| 2^-21 of the accurate one; the thread's accurate
// maximum then lies among the elements whose approximate key is within 2 d of the approximate maximum (if e* holds the
// accurate maximum and e^ the approximate one:  approx(e*) >= key(e*) - d >= key(e^) - d >= approx(e^) - 2 d), and only
// those are evaluated with vsmp_log_e - the approximate maximum itself by every lane, the others (a few per cent of the
// lanes hold one) in a loop that re-reads their logit.  The winner and its key are those of evaluating every element.
// CUT (nucleus sampling): columns whose sortable logit lies below cutkey[row] get no key, and no statistics are written.
template <bool CUT>
__global__ __launch_bounds__(256) void vsmp_chunk_kernel(const bf16* __restrict__ logits, int ld, int V, int nchunks, float inv_t,
                                                        uint32_t seed, unsigned long long* __restrict__ wkey,
                                                        float* __restrict__ pstat, const uint32_t* __restrict__ cutkey) {
  __shared__ unsigned long long redk[4];
  __shared__ float redm[4];
  __shared__ float reds[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const VsChunk c = vs_chunk_of_block(logits, ld, nchunks);
  const uint32_t col0 = (uint32_t)c.chunk * VS_CHUNK;
  const uint32_t idx0 = (uint32_t)c.row * (uint32_t)V + col0;      // (the launcher holds n * V below 2^32)
  float y[16], ka[16];                     // x * inv_t (-inf: no column) and the approximate key (NaN: no column)
  float mx = -INFINITY, amax = -INFINITY;
  uint32_t ck = 0u;
  if constexpr (CUT) ck = cutkey[c.row];
  int lbest = -1;                          // column in the chunk of the approximate maximum (-1: the thread holds no column)
  float xbest = 0.f;
#pragma unroll
  for (int run = 0; run < VS_RUNS; ++run) {
    const VsRun r = vs_chunk_run(c, V, tid, run);
#pragma unroll
    for (int e = 0; e < VS_RUN; ++e) {
      float yy = -INFINITY, k = __builtin_nanf("");
      // (the column's values in front of the guard: taken inside it, the update of the maximum below compiles to a branch per
      // column instead of three selects - and this is the kernel whose VALU work shows)
      const uint32_t raw = r.raw(e), sk = r.sk(e);
      const int lc = r.lc(e);
      bool take = r.in(e);
      if constexpr (CUT) take = take && sk >= ck;
      if (take) {
        const float x = __uint_as_float(raw << 16);        // (the bits as loaded: -0 keeps its sign in y and in the key)
        yy = __fmul_rn(x, inv_t);
        k = __fmaf_rn(x, inv_t, -vsmp_log_e_approx(idx0 + (uint32_t)lc, seed));
        mx = fmaxf(mx, yy);
        if (lbest < 0 || k > amax) {                       // (the first column, then strictly better ones)
          amax = k;
          lbest = lc;
          xbest = x;
        }
      }
      y[run * VS_RUN + e] = yy;
      ka[run * VS_RUN + e] = k;
    }
  }
  unsigned long long best = 0ull;          // 0: no entry (a key's upper word is 0 for one NaN pattern only)
  if (lbest >= 0) best = vsmp_key64(__fmaf_rn(xbest, inv_t, -vsmp_log_e(idx0 + (uint32_t)lbest, seed)), col0 + (uint32_t)lbest);
  // the other columns that may still hold the accurate maximum (amax = -inf: the threshold is -inf, every column of the thread)
  const float thr = amax - (VSMP_BAND + fabsf(amax) * 0x1p-20f);
  uint32_t pending = 0u;
#pragma unroll
  for (int e = 0; e < 16; ++e)
    if (ka[e] >= thr && vs_slot_column(tid, e) != lbest) pending |= 1u << e;
  while (pending) {
    const int e = __builtin_ctz(pending);
    pending &= pending - 1u;
    const int lc = vs_slot_column(tid, e);                 // (a column below V: ka is NaN elsewhere)
    const float x = __uint_as_float((uint32_t)c.base[lc] << 16);
    const unsigned long long k64 = vsmp_key64(__fmaf_rn(x, inv_t, -vsmp_log_e(idx0 + (uint32_t)lc, seed)), col0 + (uint32_t)lc);
    best = k64 > best ? k64 : best;
  }
  best = wave_max_u64(best);
  mx = wave_max(mx);
  if (lane == 0) {
    redk[wv] = best;
    redm[wv] = mx;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    best = redk[q] > best ? redk[q] : best;
    mx = fmaxf(mx, redm[q]);
  }
  if constexpr (CUT) {                     // (the allowed set's log-sum-exp comes from vnuc_cut_kernel)
    if (tid == 0) wkey[blockIdx.x] = best;
    return;
  }
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e)
    if (y[e] > -INFINITY) s += __expf(y[e] - mx);          // (a finite y: the maximum is finite too)
  s = wave_sum(s);
  if (lane == 0) reds[wv] = s;
  __syncthreads();
  if (tid == 0) {
    wkey[blockIdx.x] = best;
    pstat[(size_t)blockIdx.x * 2] = mx;
    pstat[(size_t)blockIdx.x * 2 + 1] = (reds[0] + reds[1]) + (reds[2] + reds[3]);
  }
}

// The draw of a row, written by the one thread that holds the winner win = (sortable key << 32 | ~word) of a word of logit x:
// logprob is ONE fma against the allowed set's lse.  cut() is the row's cut, asked for only if cut_out wants it and behind the
// other stores (vsw_draw_kernel's sits in LDS: read ahead of its fp64 logarithm it lengthens the kernel's tail); the second
// form is for the kernels without a cut.
template <class C>
__device__ __forceinline__ void vsmp_write_draw(long long row, unsigned long long win, uint32_t word, float x, float inv_t, float lse,
                                                long long* __restrict__ words, float* __restrict__ logprob,
                                                float* __restrict__ key_out, float* __restrict__ cut_out, C&& cut) {
  words[row] = (long long)word;
  logprob[row] = __fmaf_rn(x, inv_t, -lse);
  if (key_out) key_out[row] = vs_value32((uint32_t)(win >> 32));
  if (cut_out) cut_out[row] = cut();
}
__device__ __forceinline__ void vsmp_write_draw(long long row, unsigned long long win, uint32_t word, float x, float inv_t, float lse,
                                                long long* __restrict__ words, float* __restrict__ logprob,
                                                float* __restrict__ key_out) {
  vsmp_write_draw(row, win, word, x, inv_t, lse, words, logprob, key_out, nullptr, [] { return 0.f; });
}

// a wave per row (four rows per workgroup): the row's winner among its chunks' winners wkey; logprob from the winner's own
// logit against lse[row] (LSE_GIVEN), or against the log-sum-exp merged from the chunks' (max, sum) in pstat
template <bool LSE_GIVEN>
__device__ __forceinline__ void vsmp_merge_row(const bf16* __restrict__ logits, int ld, int n, int V, int nchunks, float inv_t,
                                               const unsigned long long* __restrict__ wkey, const float* __restrict__ pstat,
                                               const float* __restrict__ lse, long long* __restrict__ words,
                                               float* __restrict__ logprob, float* __restrict__ key_out) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;                                    // (wave-uniform; the callers have no barrier)
  const unsigned long long* wk = wkey + (size_t)row * nchunks;
  unsigned long long best = 0ull;
  auto winner = [&](int c) { best = wk[c] > best ? wk[c] : best; };
  float l;
  if constexpr (LSE_GIVEN) {
    for (int c = lane; c < nchunks; c += 64) winner(c);
    l = lse[row];
  } else {
    l = vs_row_lse(pstat + (size_t)row * nchunks * 2, nchunks, lane, winner);
  }
  best = wave_max_u64(best);
  if (lane == 0) {
    const uint32_t word = min(~(uint32_t)best, (uint32_t)(V - 1));      // (a chunk's winner is a column below V; the clamp guards the read)
    const float x = __uint_as_float((uint32_t)reinterpret_cast<const unsigned short*>(logits)[(size_t)row * ld + word] << 16);
    vsmp_write_draw(row, best, word, x, inv_t, l, words, logprob, key_out);
  }
}

// a wave per row: the row's winner among its chunks' winners, lse_T from the chunks' (max, sum)
__global__ __launch_bounds__(256) void vsmp_merge_kernel(const bf16* __restrict__ logits, int ld, int n, int V, int nchunks, float inv_t,
                                                        const unsigned long long* __restrict__ wkey,
                                                        const float* __restrict__ pstat, long long* __restrict__ words,
                                                        float* __restrict__ logprob, float* __restrict__ key_out) {
  vsmp_merge_row<false>(logits, ld, n, V, nchunks, inv_t, wkey, pstat, nullptr, words, logprob, key_out);
}

// a wave per row over the candidates vs_chunk_kernel left with k = top_k: lane j ends up with the row's j-th entry under
// (logit descending, word ascending); keys, lse_T and the argmax over those lanes.
// CUT (nucleus sampling): the lanes are the candidate set in the order of the cumulated mass, so the cut is a sum over
// <= 16 lanes - lane j is allowed iff the mass of the lanes with a LARGER logit is below top_p * Z (whole classes of equal
// logits).  fp32 sums in lane order, the same in every lane: reproducible.
template <bool CUT>
__global__ __launch_bounds__(256) void vsmp_topk_kernel(const uint32_t* __restrict__ cand, int n, int V, int nchunks, int k, float inv_t,
                                                       uint32_t seed, long long* __restrict__ words, float* __restrict__ logprob,
                                                       float* __restrict__ key_out, float top_p, float* __restrict__ cut_out) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;                                    // (wave-uniform; the kernel has no barrier)
  const int total = nchunks * k;
  const uint32_t* cs = cand + (size_t)row * total;
  unsigned long long bound = ~0ull;        // entries strictly below it are still to be had by this lane
  unsigned long long best;
  auto scan = [&]() {
    best = 0ull;
    for (int i = lane; i < total; i += 64) {
      const uint32_t c32 = cs[i];
      if (c32 == 0u) continue;
      const uint32_t word = (uint32_t)(i / k) * VS_CHUNK + (0xFFFFu - (c32 & 0xFFFFu));
      const unsigned long long x = (unsigned long long)(c32 >> 16) << 32 | (unsigned long long)(~word);
      if (x < bound && x > best) best = x;
    }
  };
  scan();
  unsigned long long mine = 0ull;
  for (int j = 0; j < k; ++j) {
    const unsigned long long w = wave_max_u64(best);
    if (lane == j) mine = w;
    if (best == w && w != 0ull) {          // the word is part of the entry: one lane
      bound = w;
      scan();
    }
  }
  const uint32_t word = ~(uint32_t)mine;
  const float x = vs_value16((uint32_t)(mine >> 32));
  float yy = -INFINITY;
  unsigned long long k64 = 0ull;
  if (mine != 0ull) {                      // (lanes 0 .. top_k - 1: the launcher asks for top_k <= V)
    yy = __fmul_rn(x, inv_t);
    k64 = vsmp_key64(__fmaf_rn(x, inv_t, -vsmp_log_e((uint32_t)row * (uint32_t)V + word, seed)), word);
  }
  const float m = wave_max(yy);
  if constexpr (CUT) {
    float w = mine != 0ull ? expf(__fmaf_rn(x, inv_t, -m)) : 0.f;      // (ONE rounding of x * inv_t - m; -inf: mass 0)
    w = w == w ? w : 0.f;
    float Z = 0.f, above = 0.f;
    for (int i = 0; i < k; ++i) {
      const float xi = __shfl(x, i, 64), wi = __shfl(w, i, 64);
      Z += wi;
      if (xi > x) above += wi;
    }
    const bool in = mine != 0ull && (double)above < (double)top_p * (double)Z;
    float sa = 0.f, xc = x;
    for (int i = 0; i < k; ++i) {
      const float xi = __shfl(x, i, 64), wi = __shfl(w, i, 64);
      if (__shfl((int)in, i, 64)) {        // (the allowed lanes are a prefix: the last one holds the cut)
        sa += wi;
        xc = xi;
      }
    }
    k64 = in ? k64 : 0ull;
    const unsigned long long win = wave_max_u64(k64);
    if (k64 == win && win != 0ull)
      vsmp_write_draw(row, win, word, x, inv_t, m + logf(sa), words, logprob, key_out, cut_out, [&] { return xc; });
    return;
  }
  // (NOT the sum above with top_p = 1: there a term is expf of ONE fma(x, inv_t, -m) and the terms are added in lane order;
  // here it is expf(fl(x * inv_t) - m) under the butterfly of wave_sum - the two lse differ in their last bits)
  const float s = wave_sum(yy > -INFINITY ? expf(yy - m) : 0.f);
  const unsigned long long win = wave_max_u64(k64);
  if (k64 == win && win != 0ull) vsmp_write_draw(row, win, word, x, inv_t, m + logf(s), words, logprob, key_out);
}

// ------------------------------------------------------------------------------------------------------------------------
// nucleus (top-p) sampling: m3p_vocab_nucleus_sample
// ------------------------------------------------------------------------------------------------------------------------
// The allowed set of a row is { w : x_w >= x* }, x* the largest logit value v whose cumulated mass C(v) (all words with a
// logit >= v, softmax of x * inv_t) reaches top_p * Z: whole classes of equal logits, an exact weighted selection over the
// 65 536 bf16 values.  Two levels of 256 bins over the sortable 16-bit key:
//   vs_chunk_kernel (k = 1)   the chunks' maxima -> the row's m = fl(max x * inv_t)
//   vnuc_coarse_kernel        a workgroup per (row, chunk): per HIGH byte of the key the mass of its words, every word's mass
//                             the INTEGER  rint(expf(fma(x, inv_t, -m)) * 2^shift)  - integer sums do not depend on their
//                             order, so LDS and global atomics leave the result reproducible bit for bit
//   vnuc_scan_kernel          a wave per row: Z, the coarse bin that holds the cut, the mass above that bin
//   vnuc_fine_kernel          a workgroup per (row, chunk): per LOW byte the NUMBER of words inside that bin - all words of
//                             one value have one mass, so count * mass(value) adds up to the bin's mass of the coarse pass
//   vnuc_cut_kernel           a wave per row: x*, the allowed set's mass -> its log-sum-exp
//   vsmp_chunk_kernel<true>   the Gumbel-max pass, columns below x* without a key;  vnuc_merge_kernel: the row's winner
// A -inf logit has mass 0; x* is the value of a word with a positive mass, so it is finite.  shift = min(40, 63 - bits(V)):
// the sum of V masses of at most 2^shift (1 + 2^-20) stays below 2^64.
constexpr int VN_BINS = 256;

// A workgroup's VN_BINS bins of T in LDS (declare it __shared__), summed into a row's bins in memory.  Integer adds commute,
// so neither the LDS nor the global atomics make a result depend on their order.  T* mine = zero(tid), a barrier of the
// caller's (behind whatever else it fetches meanwhile), add(mine, bin, v) per word, flush(): 256 threads, thread tid folds
// bin tid.  (`mine`, the thread's copy of the bins, is handed out once: an address computed per word costs two instructions.)
template <class T>
struct VnHist {
  static constexpr int VN_COPIES = 8;      // copies of the bins, by tid & 7 (padded by one bin: other banks)
  T bins[VN_COPIES][VN_BINS + 1];
  __device__ __forceinline__ T* zero(int tid) {
#pragma unroll
    for (int c = 0; c < VN_COPIES; ++c) bins[c][tid] = T(0);
    return bins[tid & (VN_COPIES - 1)];
  }
  static __device__ __forceinline__ void add(T* mine, uint32_t bin, T v) { atomicAdd(&mine[bin], v); }
  __device__ __forceinline__ void flush(int tid, T* __restrict__ row_bins) {
    __syncthreads();
    T s = T(0);
#pragma unroll
    for (int c = 0; c < VN_COPIES; ++c) s += bins[c][tid];
    if (s != T(0)) atomicAdd(row_bins + tid, s);
  }
};

struct VnucLayout {
  size_t hist, fine, wkey, rowz, pstat, cand, rowbin, bytes;
  int shift;
};
VnucLayout vnuc_layout(int n, int V) {
  const size_t rows = (size_t)n, blocks = rows * (size_t)vs_nchunks(V);
  VnucLayout L;
  size_t o = 0;
  L.hist = o;   o += rows * VN_BINS * sizeof(unsigned long long);       // [n, 256] u64, zeroed by the launcher with ...
  L.fine = o;   o += rows * VN_BINS * sizeof(uint32_t);                 // ... [n, 256] u32 behind it
  L.wkey = o;   o += blocks * sizeof(unsigned long long);
  L.rowz = o;   o += rows * 2 * sizeof(unsigned long long);             // Z [n], mass above the cut's coarse bin [n]
  L.pstat = o;  o += blocks * 2 * sizeof(float);
  L.cand = o;   o += blocks * sizeof(uint32_t);
  L.rowbin = o; o += rows * 3 * sizeof(uint32_t);                       // coarse bin [n], sortable cut [n], lse [n]
  L.bytes = o;
  int bits = 0;
  while (bits < 32 && ((unsigned long long)V >> bits) != 0ull) ++bits;
  L.shift = 63 - bits < 40 ? 63 - bits : 40;
  return L;
}

// the row's m from the chunk maxima vs_chunk_kernel left (every lane of a wave gets it)
__device__ __forceinline__ float vnuc_row_max(const float* __restrict__ pstat, long long row, int nchunks, float inv_t, int lane) {
  const float* ps = pstat + (size_t)row * nchunks * 2;
  float mx = -INFINITY;
  for (int c = lane; c < nchunks; c += 64) mx = fmaxf(mx, ps[2 * c]);
  return __fmul_rn(wave_max(mx), inv_t);
}
// the integer mass of a word of logit x: one rounding of x * inv_t - m, expf (not __expf: 1 ulp, documented), 2^-shift grid
__device__ __forceinline__ unsigned long long vnuc_mass(float x, float inv_t, float m, float scale) {
  const float w = expf(__fmaf_rn(x, inv_t, -m)) * scale;
  return w > 0.f && w < 0x1p62f ? (unsigned long long)rintf(w) : 0ull;       // (NaN, inf - rows outside the contract - add nothing)
}
// do the cumulated mass c and the row's Z satisfy  c >= top_p * Z ?  (fp64: 2^-53 relative on either side)
__device__ __forceinline__ bool vnuc_reaches(unsigned long long c, unsigned long long Z, float top_p) {
  return (double)c >= (double)top_p * (double)Z;
}
// inclusive sums over the lanes at and above this one (lane 63 holds its own value, lane 0 the total)
__device__ __forceinline__ unsigned long long vnuc_suffix_u64(unsigned long long v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long t = (unsigned long long)__shfl_down((long long)v, o, 64);
    if (lane + o < 64) v += t;
  }
  return v;
}

// The bin scan of a wave over a row's 256 bins, lane l holding b = bins 4 l .. 4 l + 3: the HIGHEST bin at which the value
// cumulated from the top, behind `carry`, satisfies reached(cumulated, total) - total = the sum of all 256 bins, carry not
// included.  Empty bins are skipped: one cannot be the first to get there (its cumulated value is that of the next bin above,
// or the bare carry at the top).  Every lane gets bin (-1: none) and total; `owner` is true in ONE lane, the bin's (lane 0
// without a bin), and there above / at are the values cumulated above the bin and with it (both 0 without a bin).
struct VnBinScan {
  int bin;
  bool owner;
  unsigned long long above, at, total;
};
template <class P>
__device__ __forceinline__ VnBinScan vn_bin_scan(const unsigned long long (&b)[4], unsigned long long carry, int lane, P&& reached) {
  const unsigned long long s = (b[0] + b[1]) + (b[2] + b[3]);
  const unsigned long long inc = vnuc_suffix_u64(s, lane);
  VnBinScan r;
  r.total = (unsigned long long)__shfl((long long)inc, 0, 64);
  r.above = r.at = 0ull;
  unsigned long long c = carry + (inc - s);
  int best = -1;
#pragma unroll
  for (int q = 3; q >= 0; --q) {
    const unsigned long long ci = c + b[q];
    const bool hit = reached(ci, r.total);                 // (asked of every bin: behind the other tests its threshold is computed per bin)
    if (best < 0 && b[q] != 0ull && hit) {
      best = 4 * lane + q;
      r.above = c;
      r.at = ci;
    }
    c = ci;
  }
  r.bin = (int)wave_max_u32((uint32_t)(best + 1)) - 1;
  r.owner = r.bin < 0 ? lane == 0 : best == r.bin;         // (a bin belongs to one lane)
  return r;
}

__global__ __launch_bounds__(256) void vnuc_coarse_kernel(const bf16* __restrict__ logits, int ld, int V, int nchunks, float inv_t,
                                                         float scale, const float* __restrict__ pstat,
                                                         unsigned long long* __restrict__ hist) {
  __shared__ VnHist<unsigned long long> bins;
  const int tid = threadIdx.x, lane = tid & 63;
  const VsChunk c = vs_chunk_of_block(logits, ld, nchunks);
  unsigned long long* mine = bins.zero(tid);
  const float m = vnuc_row_max(pstat, c.row, nchunks, inv_t, lane);
  __syncthreads();
#pragma unroll
  for (int run = 0; run < VS_RUNS; ++run) {
    const VsRun r = vs_chunk_run(c, V, tid, run);
#pragma unroll
    for (int e = 0; e < VS_RUN; ++e)
      if (r.in(e)) {
        const unsigned long long w = vnuc_mass(__uint_as_float(r.bits(e) << 16), inv_t, m, scale);
        if (w != 0ull) bins.add(mine, r.sk(e) >> 8, w);
      }
  }
  bins.flush(tid, hist + (size_t)c.row * VN_BINS);
}

// a wave per row over its 256 coarse bins: Z, the highest bin at which the mass cumulated from the top reaches top_p * Z, and
// the mass above that bin.  (No bin - a row outside the contract -: bin -1, nothing below.)
__global__ __launch_bounds__(256) void vnuc_scan_kernel(const unsigned long long* __restrict__ hist, int n, float top_p,
                                                       unsigned long long* __restrict__ rowz, unsigned long long* __restrict__ rowabove,
                                                       int* __restrict__ rowbin) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;                                    // (wave-uniform; the kernel has no barrier)
  const unsigned long long* h = hist + (size_t)row * VN_BINS + 4 * lane;
  const unsigned long long b[4] = {h[0], h[1], h[2], h[3]};
  const VnBinScan r = vn_bin_scan(b, 0ull, lane, [&](unsigned long long c, unsigned long long Z) {
    return Z != 0ull && vnuc_reaches(c, Z, top_p);
  });
  if (r.owner) {
    rowz[row] = r.total;
    rowabove[row] = r.above;
    rowbin[row] = r.bin;
  }
}

__global__ __launch_bounds__(256) void vnuc_fine_kernel(const bf16* __restrict__ logits, int ld, int V, int nchunks,
                                                       const int* __restrict__ rowbin, uint32_t* __restrict__ fine) {
  __shared__ VnHist<uint32_t> cnt;
  const int tid = threadIdx.x;
  const VsChunk c = vs_chunk_of_block(logits, ld, nchunks);
  uint32_t* mine = cnt.zero(tid);
  const uint32_t bin = (uint32_t)rowbin[c.row];            // (-1: no column matches)
  __syncthreads();
#pragma unroll
  for (int run = 0; run < VS_RUNS; ++run) {
    const VsRun r = vs_chunk_run(c, V, tid, run);
#pragma unroll
    for (int e = 0; e < VS_RUN; ++e) {
      const uint32_t sk = r.sk(e);
      if (r.in(e) && (sk >> 8) == bin) cnt.add(mine, sk & 0xFFu, 1u);
    }
  }
  cnt.flush(tid, fine + (size_t)c.row * VN_BINS);
}

// a wave per row over the 256 values of the cut's coarse bin (lane l holds the low bytes 4 l .. 4 l + 3): count * mass(value),
// cumulated from the top behind the mass above the bin -> x* (sortable, and as a float), lse of the allowed set
__global__ __launch_bounds__(256) void vnuc_cut_kernel(const uint32_t* __restrict__ fine, const float* __restrict__ pstat,
                                                      const unsigned long long* __restrict__ rowz,
                                                      const unsigned long long* __restrict__ rowabove, const int* __restrict__ rowbin,
                                                      int n, int nchunks, float inv_t, float top_p, float scale, int shift,
                                                      uint32_t* __restrict__ cutkey, float* __restrict__ lse, float* __restrict__ cut_out) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;                                    // (wave-uniform; the kernel has no barrier)
  const float m = vnuc_row_max(pstat, row, nchunks, inv_t, lane);
  const int bin = rowbin[row];
  const unsigned long long Z = rowz[row], above0 = rowabove[row];
  unsigned long long b[4] = {0ull, 0ull, 0ull, 0ull};
  if (bin >= 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t c = fine[(size_t)row * VN_BINS + 4 * lane + q];
      if (c != 0u) b[q] = (unsigned long long)c * vnuc_mass(vs_value16((uint32_t)bin << 8 | (uint32_t)(4 * lane + q)), inv_t, m, scale);
    }
  }
  const VnBinScan r = vn_bin_scan(b, above0, lane, [&](unsigned long long c, unsigned long long) { return vnuc_reaches(c, Z, top_p); });
  if (r.owner) {
    // (no value - a row outside the contract -: no cut, every word allowed)
    const int win = r.bin;
    const uint32_t sk = win < 0 ? 0u : ((uint32_t)bin << 8 | (uint32_t)win);
    const unsigned long long mass = win < 0 ? Z : r.at;
    cutkey[row] = sk;
    lse[row] = (float)((double)m + (log((double)mass) - (double)shift * 0.693147180559945309417));
    if (cut_out) cut_out[row] = win < 0 ? -INFINITY : vs_value16(sk);
  }
}

// a wave per row: the row's winner among its chunks' winners; logprob against the allowed set's lse
__global__ __launch_bounds__(256) void vnuc_merge_kernel(const bf16* __restrict__ logits, int ld, int n, int V, int nchunks, float inv_t,
                                                        const unsigned long long* __restrict__ wkey, const float* __restrict__ lse,
                                                        long long* __restrict__ words, float* __restrict__ logprob,
                                                        float* __restrict__ key_out) {
  vsmp_merge_row<true>(logits, ld, n, V, nchunks, inv_t, wkey, nullptr, lse, words, logprob, key_out);
}

// the plan of every seeded draw: min_k <= top_k <= V, launchers up to max_k candidates
int vsmp_plan(int n, int V, int ld, int top_k, int min_k, int max_k) {
  if (n <= 0 || V <= 0 || top_k < min_k || ld < V || (ld % 8) != 0 || top_k > V) return M3P_EINVAL;
  if (top_k > max_k) return M3P_ENOTIMPL;
  if ((long long)n * V >= (1ll << 32)) return M3P_ENOTIMPL;                          // the hash counter r * V + w is 32 bits
  if ((long long)n * vs_nchunks(V) * VS_MAX_K >= (1ll << 31)) return M3P_ENOTIMPL;       // 32-bit block and candidate indices
  return M3P_OK;
}

// ------------------------------------------------------------------------------------------------------------------------
// seeded sampling over more than VS_MAX_K candidates: m3p_vocab_sample_wide (1 <= top_k <= VSW_MAX_K), nucleus cut included
// ------------------------------------------------------------------------------------------------------------------------
// k rounds of a block-wide maximum (vs_chunk_kernel: every chunk hands on its own first k, a wave then merges chunks * k
// candidates in k more rounds) cost k barriers per workgroup and k * chunks * k merge work per row - 62 chunks at k = 50 are
// 3 100 candidates scanned 50 times by one wave, at k = 1024 it is 65 million reads per row.  Here the candidate set K is
// found by an exact SELECTION instead, and only K is ever sorted:
//   vsw_coarse_kernel    a workgroup per (row, chunk): the NUMBER of words per HIGH byte of the sortable 16-bit key (LDS
//                        and global integer atomics: counts do not depend on their order)
//   vsw_scan_kernel      a wave per row: the coarse bin at which the count cumulated from the top reaches top_k
//   vnuc_fine_kernel     (the nucleus route's, as it is) the number of words per LOW byte inside that bin
//   vsw_scan_kernel      again, behind the count above the bin: the k-th value v_k and above = #{x > v_k}
//   vsw_tie_kernel       per (row, chunk) the words above v_k and the words equal to it
//   vsw_compact_kernel   K -> ent[row, top_k] as (sortable logit << 32 | ~word): every word above v_k, and of the class at v_k
//                        the quota q = top_k - above in COLUMN order - the chunks before this one hold so many of the class
//                        (a sum over chunkcnt), inside the chunk a block prefix sum over (tid * 8 + e, then 2048 + tid * 8 + e)
//   vsw_draw_kernel      a workgroup per row, K in LDS: a bitonic sort (logit descending, word ascending), masses as the
//                        integers of vnuc_mass (shift 40: 1024 of them stay below 2^51), their prefix sums, the nucleus cut
//                        at the first class end whose cumulated mass reaches top_p * Z, the keys of the allowed entries by
//                        vsmp_log_e, the winner, lse = m + log(mass) - shift ln 2 in fp64.  top_p >= 1: no cut, cut = -inf.
// The selection is on integer keys alone, so every kernel agrees on K; integer atomics only; the same inputs, the same bits.
constexpr int VSW_MAX_K = 1024;
constexpr int VSW_SHIFT = 40;

struct VswLayout {
  size_t ent, hist, fine, chunkcnt, rowbin, rowlow, above0, above1, bytes;
};
VswLayout vsw_layout(int n, int V, int top_k) {
  const size_t rows = (size_t)n, blocks = rows * (size_t)vs_nchunks(V);
  VswLayout L;
  size_t o = 0;
  L.ent = o;      o += rows * (size_t)top_k * sizeof(unsigned long long);
  L.hist = o;     o += rows * VN_BINS * sizeof(uint32_t);                 // [n, 256] u32, zeroed by the launcher with ...
  L.fine = o;     o += rows * VN_BINS * sizeof(uint32_t);                 // ... [n, 256] u32 behind it
  L.chunkcnt = o; o += blocks * 2 * sizeof(uint32_t);                     // per (row, chunk): words above v_k, words equal to it
  L.rowbin = o;   o += rows * sizeof(int);                                // high byte of v_k's key
  L.rowlow = o;   o += rows * sizeof(int);                                // low byte
  L.above0 = o;   o += rows * sizeof(uint32_t);                           // words above the coarse bin
  L.above1 = o;   o += rows * sizeof(uint32_t);                           // words above v_k
  L.bytes = o;
  return L;
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}
// the sortable key of v_k (0x10000, above every key, when a scan found none - a row outside the contract)
__device__ __forceinline__ uint32_t vsw_kth(const int* __restrict__ rowbin, const int* __restrict__ rowlow, int row) {
  const int b = rowbin[row], l = rowlow[row];
  return b < 0 || l < 0 ? 0x10000u : ((uint32_t)b << 8 | (uint32_t)l);
}
// exclusive prefix of v over the 256 threads of a workgroup and the workgroup's total (sh: 4 words of LDS of this call's own)
__device__ __forceinline__ unsigned long long vsw_block_excl(unsigned long long v, int tid, unsigned long long* sh,
                                                             unsigned long long& total) {
  const int lane = tid & 63, wv = tid >> 6;
  unsigned long long inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long t = (unsigned long long)__shfl_up((long long)inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) sh[wv] = inc;
  __syncthreads();
  unsigned long long base = 0ull;
  total = 0ull;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (q < wv) base += sh[q];
    total += sh[q];
  }
  return base + (inc - v);
}

__global__ __launch_bounds__(256) void vsw_coarse_kernel(const bf16* __restrict__ logits, int ld, int V, int nchunks,
                                                        uint32_t* __restrict__ hist) {
  __shared__ VnHist<uint32_t> cnt;
  const int tid = threadIdx.x;
  const VsChunk c = vs_chunk_of_block(logits, ld, nchunks);
  uint32_t* mine = cnt.zero(tid);
  __syncthreads();
#pragma unroll
  for (int run = 0; run < VS_RUNS; ++run) {
    const VsRun r = vs_chunk_run(c, V, tid, run);
#pragma unroll
    for (int e = 0; e < VS_RUN; ++e) {
      const uint32_t sk = r.sk(e);
      if (r.in(e)) cnt.add(mine, sk >> 8, 1u);
    }
  }
  cnt.flush(tid, hist + (size_t)c.row * VN_BINS);
}

// a wave per row over 256 counts: the highest bin at which the count cumulated from the top, behind above_in[row] (NULL: 0),
// reaches top_k, and the count above that bin.  (No bin: -1 and 0.)
__global__ __launch_bounds__(256) void vsw_scan_kernel(const uint32_t* __restrict__ cnt, int n, uint32_t top_k,
                                                      const uint32_t* __restrict__ above_in, int* __restrict__ bin_out,
                                                      uint32_t* __restrict__ above_out) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;                                    // (wave-uniform; the kernel has no barrier)
  const uint32_t* h = cnt + (size_t)row * VN_BINS + 4 * lane;
  const unsigned long long b[4] = {h[0], h[1], h[2], h[3]};
  const VnBinScan r = vn_bin_scan(b, above_in ? (unsigned long long)above_in[row] : 0ull, lane,
                                  [&](unsigned long long c, unsigned long long) { return c >= (unsigned long long)top_k; });
  if (r.owner) {
    bin_out[row] = r.bin;
    above_out[row] = (uint32_t)r.above;
  }
}

__global__ __launch_bounds__(256) void vsw_tie_kernel(const bf16* __restrict__ logits, int ld, int V, int nchunks,
                                                     const int* __restrict__ rowbin, const int* __restrict__ rowlow,
                                                     uint32_t* __restrict__ chunkcnt) {
  __shared__ uint32_t red[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const VsChunk ch = vs_chunk_of_block(logits, ld, nchunks);
  const uint32_t kth = vsw_kth(rowbin, rowlow, ch.row);
  uint32_t c = 0u;                                          // words above << 16 | words equal (a chunk holds 4096: 13 bits each)
#pragma unroll
  for (int run = 0; run < VS_RUNS; ++run) {
    const VsRun r = vs_chunk_run(ch, V, tid, run);
#pragma unroll
    for (int e = 0; e < VS_RUN; ++e) {
      const uint32_t sk = r.sk(e);                          // (in front of the guard: the guarded add then compiles to selects)
      if (r.in(e)) c += sk > kth ? 0x10000u : (sk == kth ? 1u : 0u);
    }
  }
  c = wave_sum_u32(c);
  if (lane == 0) red[wv] = c;
  __syncthreads();
  if (tid == 0) {
    c = (red[0] + red[1]) + (red[2] + red[3]);
    chunkcnt[(size_t)blockIdx.x * 2] = c >> 16;
    chunkcnt[(size_t)blockIdx.x * 2 + 1] = c & 0xFFFFu;
  }
}

__global__ __launch_bounds__(256) void vsw_compact_kernel(const bf16* __restrict__ logits, int ld, int V, int nchunks, int top_k,
                                                         const int* __restrict__ rowbin, const int* __restrict__ rowlow,
                                                         const uint32_t* __restrict__ rowabove, const uint32_t* __restrict__ chunkcnt,
                                                         unsigned long long* __restrict__ ent) {
  __shared__ unsigned long long sh[2][4];
  const int tid = threadIdx.x;
  const VsChunk ch = vs_chunk_of_block(logits, ld, nchunks);
  const int row = ch.row, chunk = ch.chunk;
  const uint32_t kth = vsw_kth(rowbin, rowlow, row);
  const uint32_t above = min(rowabove[row], (uint32_t)top_k), quota = (uint32_t)top_k - above;
  // the chunks in front of this one: their words above v_k (slots 0 .. above - 1) and their members of the class at v_k
  const uint32_t* cc = chunkcnt + (size_t)row * nchunks * 2;
  unsigned long long before = 0ull, total;
  for (int c = tid; c < chunk; c += 256) before += (unsigned long long)cc[2 * c] << 32 | (unsigned long long)cc[2 * c + 1];
  vsw_block_excl(before, tid, sh[0], total);
  const uint32_t a0 = (uint32_t)(total >> 32), t0 = (uint32_t)total;
  if (cc[2 * chunk] == 0u && (cc[2 * chunk + 1] == 0u || t0 >= quota)) return;       // (the same in every thread) nothing of K here
  uint32_t sk[16];
  unsigned long long mine = 0ull;                           // words above << 40 | class members of half 1 << 20 | of half 0
#pragma unroll
  for (int run = 0; run < VS_RUNS; ++run) {
    const VsRun r = vs_chunk_run(ch, V, tid, run);
#pragma unroll
    for (int e = 0; e < VS_RUN; ++e) {
      const uint32_t s = r.in(e) ? r.sk(e) : 0xFFFFFFFFu;   // (no column)
      sk[run * VS_RUN + e] = s;
      if (s != 0xFFFFFFFFu) mine += s > kth ? 1ull << 40 : (s == kth ? 1ull << (20 * run) : 0ull);
    }
  }
  const unsigned long long excl = vsw_block_excl(mine, tid, sh[1], total);
  uint32_t pa = a0 + (uint32_t)(excl >> 40);                                           // the slot of this thread's next word above v_k
  uint32_t pt[2] = {t0 + (uint32_t)(excl & 0xFFFFFu),                                  // the class rank of its next member, per half
                    t0 + (uint32_t)(total & 0xFFFFFu) + (uint32_t)((excl >> 20) & 0xFFFFFu)};
  unsigned long long* out = ent + (size_t)row * top_k;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const uint32_t s = sk[e];
    if (s == 0xFFFFFFFFu) continue;
    const uint32_t word = (uint32_t)chunk * VS_CHUNK + (uint32_t)vs_slot_column(tid, e);
    uint32_t slot = 0xFFFFFFFFu;
    if (s > kth) slot = pa++;
    else if (s == kth) {
      const uint32_t rank = pt[e >> 3]++;
      if (rank < quota) slot = above + rank;
    }
    if (slot < (uint32_t)top_k) out[slot] = (unsigned long long)s << 32 | (unsigned long long)(~word);
  }
}

__global__ __launch_bounds__(256) void vsw_draw_kernel(const unsigned long long* __restrict__ ent, int V, int top_k, int N,
                                                      float inv_t, float top_p, uint32_t seed, long long* __restrict__ words,
                                                      float* __restrict__ logprob, float* __restrict__ key_out,
                                                      float* __restrict__ cut_out) {
  __shared__ unsigned long long keys[VSW_MAX_K];
  __shared__ unsigned long long sh[4], redk[4], s_mass;
  __shared__ int rede[4];
  __shared__ uint32_t s_cut;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int row = blockIdx.x;
  // N = the power of two at or above top_k (at least 2): the entries, then zeros - below every entry
  for (int i = tid; i < N; i += 256) keys[i] = i < top_k ? ent[(size_t)row * top_k + i] : 0ull;
  __syncthreads();
  for (int k2 = 2; k2 <= N; k2 <<= 1)                       // bitonic sort, descending: (logit descending, word ascending)
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < N / 2; t += 256) {
        const int i = 2 * t - (t & (j - 1)), l = i + j;
        const unsigned long long a = keys[i], b = keys[l];
        if ((a < b) == ((i & k2) == 0)) {
          keys[i] = b;
          keys[l] = a;
        }
      }
      __syncthreads();
    }
  // thread t holds the entries t * per .. t * per + per - 1
  const int per = N > 256 ? N / 256 : 1, i0 = tid * per;
  const float m = __fmul_rn(vs_value16((uint32_t)(keys[0] >> 32)), inv_t);
  const float scale = (float)(1ull << VSW_SHIFT);
  unsigned long long kk[4], w[4], mine = 0ull;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = i0 + q;
    kk[q] = q < per && i < top_k ? keys[i] : 0ull;
    w[q] = kk[q] != 0ull ? vnuc_mass(vs_value16((uint32_t)(kk[q] >> 32)), inv_t, m, scale) : 0ull;
    mine += w[q];
  }
  unsigned long long Z;
  const unsigned long long excl = vsw_block_excl(mine, tid, sh, Z);
  // the last allowed entry: the first end of a class of equal logits at which the cumulated mass reaches top_p * Z
  int cand = top_k - 1;
  if (top_p < 1.f && Z != 0ull) {
    unsigned long long c = excl;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (kk[q] == 0ull) continue;
      const int i = i0 + q;
      c += w[q];
      const bool end = i == top_k - 1 || (uint32_t)(keys[i + 1] >> 32) != (uint32_t)(kk[q] >> 32);
      if (end && vnuc_reaches(c, Z, top_p)) cand = min(cand, i);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
  if (lane == 0) rede[wv] = cand;
  __syncthreads();
  const int last = min(min(rede[0], rede[1]), min(rede[2], rede[3]));
  if (last >= i0 && last < i0 + per) {                      // (one thread)
    unsigned long long c = excl;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (i0 + q <= last) c += w[q];
    s_mass = c;
    s_cut = (uint32_t)(keys[last] >> 32);
  }
  unsigned long long best = 0ull;
  float xbest = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (kk[q] == 0ull || i0 + q > last) continue;
    const uint32_t word = ~(uint32_t)kk[q];
    const float x = vs_value16((uint32_t)(kk[q] >> 32));
    const unsigned long long k64 = vsmp_key64(__fmaf_rn(x, inv_t, -vsmp_log_e((uint32_t)row * (uint32_t)V + word, seed)), word);
    if (k64 > best) {
      best = k64;
      xbest = x;
    }
  }
  unsigned long long win = wave_max_u64(best);
  if (lane == 0) redk[wv] = win;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) win = redk[q] > win ? redk[q] : win;
  if (best == win && win != 0ull) {                         // the word is part of the key: one thread
    const float lse = (float)((double)m + (log((double)s_mass) - (double)VSW_SHIFT * 0.693147180559945309417));
    vsmp_write_draw(row, win, ~(uint32_t)win, xbest, inv_t, lse, words, logprob, key_out, cut_out,
                    [&] { return top_p < 1.f ? vs_value16(s_cut) : -INFINITY; });
  }
}

// ------------------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------------------
// What every launcher asks of its arguments behind its plan: logits, a workspace of `need` bytes and the required outputs
// `outs`, the 16-byte alignment of the vector loads, a finite inv_t > 0 and top_p > 0 (1: a launcher without one).
bool vs_args_ok(const void* logits, const void* workspace, size_t workspace_bytes, size_t need, std::initializer_list<const void*> outs,
                float inv_t = 1.f, float top_p = 1.f) {
  if (!(inv_t > 0.f) || isinf(inv_t) || !(top_p > 0.f)) return false;
  if (!logits || !workspace || ((uintptr_t)logits & 15) || ((uintptr_t)workspace & 15)) return false;
  for (const void* p : outs)
    if (!p) return false;
  return workspace_bytes >= need;
}

// 1 <= top_k <= VS_MAX_K: the chunks' first top_k entries, then a wave per row draws among the row's first top_k (CUT: behind
// the nucleus cut at top_p).  The workspace is m3p_vocab_select's: the chunks' unscaled (max, sum) - written, not read - and cand.
template <bool CUT>
int vsmp_launch_topk(const void* logits, int ld, int n, int V, float inv_t, int top_k, float top_p, uint32_t seed, void* workspace,
                     long long* words, float* logprob, float* key, float* cut, hipStream_t st) {
  const int nchunks = vs_nchunks(V);
  float* pstat = (float*)workspace;
  uint32_t* cand = (uint32_t*)(pstat + (size_t)n * nchunks * 2);
  hipLaunchKernelGGL(vs_chunk_kernel, dim3((unsigned)(n * nchunks)), dim3(256), 0, st, (const bf16*)logits, ld, V, nchunks, top_k,
                     pstat, cand);
  M3P_CHECK_LAUNCH();
  hipLaunchKernelGGL(vsmp_topk_kernel<CUT>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, (const uint32_t*)cand, n, V, nchunks,
                     top_k, inv_t, seed, words, logprob, key, top_p, cut);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

int vs_pow2_at_least(int v) {           // the size of a bitonic sort over v entries (at least 2)
  int N = 2;
  while (N < v) N <<= 1;
  return N;
}

// The count selection of every row's first top_k words under (logit descending, word ascending), the launches the seeded draw
// (m3p_vocab_sample_wide) and the wide beam selection (m3p_vocab_select_wide) share: a workspace that BEGINS with
// vsw_layout(n, V, top_k) -> *ent_out = ent[n, top_k] as (sortable logit << 32 | ~word), in no order inside a row.
int vsw_launch_select(const void* logits, int ld, int n, int V, int top_k, void* workspace, hipStream_t st,
                      const unsigned long long** ent_out) {
  const int nchunks = vs_nchunks(V);
  const unsigned rows4 = (unsigned)((n + 3) / 4), blocks = (unsigned)(n * nchunks);
  const VswLayout L = vsw_layout(n, V, top_k);
  char* ws = (char*)workspace;
  unsigned long long* ent = (unsigned long long*)(ws + L.ent);
  uint32_t* hist = (uint32_t*)(ws + L.hist);
  uint32_t* fine = (uint32_t*)(ws + L.fine);
  uint32_t* chunkcnt = (uint32_t*)(ws + L.chunkcnt);
  int* rowbin = (int*)(ws + L.rowbin);
  int* rowlow = (int*)(ws + L.rowlow);
  uint32_t* above0 = (uint32_t*)(ws + L.above0);
  uint32_t* above1 = (uint32_t*)(ws + L.above1);
  if (hipMemsetAsync(hist, 0, (size_t)n * VN_BINS * 2 * sizeof(uint32_t), st) != hipSuccess) return M3P_EINVAL;
  hipLaunchKernelGGL(vsw_coarse_kernel, dim3(blocks), dim3(256), 0, st, (const bf16*)logits, ld, V, nchunks, hist);
  M3P_CHECK_LAUNCH();
  hipLaunchKernelGGL(vsw_scan_kernel, dim3(rows4), dim3(256), 0, st, (const uint32_t*)hist, n, (uint32_t)top_k,
                     (const uint32_t*)nullptr, rowbin, above0);
  M3P_CHECK_LAUNCH();
  hipLaunchKernelGGL(vnuc_fine_kernel, dim3(blocks), dim3(256), 0, st, (const bf16*)logits, ld, V, nchunks, (const int*)rowbin, fine);
  M3P_CHECK_LAUNCH();
  hipLaunchKernelGGL(vsw_scan_kernel, dim3(rows4), dim3(256), 0, st, (const uint32_t*)fine, n, (uint32_t)top_k,
                     (const uint32_t*)above0, rowlow, above1);
  M3P_CHECK_LAUNCH();
  hipLaunchKernelGGL(vsw_tie_kernel, dim3(blocks), dim3(256), 0, st, (const bf16*)logits, ld, V, nchunks, (const int*)rowbin,
                     (const int*)rowlow, chunkcnt);
  M3P_CHECK_LAUNCH();
  hipLaunchKernelGGL(vsw_compact_kernel, dim3(blocks), dim3(256), 0, st, (const bf16*)logits, ld, V, nchunks, top_k,
                     (const int*)rowbin, (const int*)rowlow, (const uint32_t*)above1, (const uint32_t*)chunkcnt, ent);
  M3P_CHECK_LAUNCH();
  *ent_out = ent;
  return M3P_OK;
}

// ------------------------------------------------------------------------------------------------------------------------
// beam search beyond VS_MAX_K entries per sentence: m3p_vocab_select_wide (1 <= k <= VSB_MAX_K, beam <= VSB_MAX_BEAM)
// ------------------------------------------------------------------------------------------------------------------------
// The contract of m3p_vocab_select for wider beams.  Phase 1 is the count selection above with top_k = k: a row's first k
// entries under (logit descending, word ascending) are what T leaves of the row, whatever its lse and beam score, so a
// sentence's first k under T lie among its beam * k <= 2048 entries of ent.  vs_chunk_kernel at k = 1 supplies the chunks'
// (max, sum) - its sum does not depend on k, so lse has the bits m3p_vocab_select gives.  Phase 2 (vsb_merge_kernel, a workgroup
// per sentence): lse per row as in vs_merge_kernel, the VsKey of every entry into LDS, ONE bitonic sort over the power of two
// at or above beam * k in place of k rounds of a maximum, the first k out.  Keys are unique ((beam, word) is part of them): the
// sorted order is T itself, and the outputs for k <= VS_MAX_K are those of m3p_vocab_select bit for bit.  No atomics here.
constexpr int VSB_MAX_K = 64;          // entries per sentence (2 * beam: beams up to 32)
constexpr int VSB_MAX_BEAM = 32;       // rows per sentence
constexpr int VSB_MAX_ENT = VSB_MAX_K * VSB_MAX_BEAM;      // keys of a sentence in LDS: 2048 x 12 bytes

struct VsbLayout {
  size_t pstat, cand, bytes;           // behind vsw_layout(n, V, k): the chunks' (max, sum) and the k = 1 candidates of vs_chunk_kernel
};
VsbLayout vsb_layout(int n, int V, int k) {
  const size_t blocks = (size_t)n * (size_t)vs_nchunks(V);
  VsbLayout B;
  size_t o = (vsw_layout(n, V, k).bytes + 15) & ~(size_t)15;
  B.pstat = o; o += blocks * 2 * sizeof(float);
  B.cand = o;  o += blocks * sizeof(uint32_t);
  B.bytes = o;
  return B;
}

int vsb_plan(int n, int V, int ld, int beam, int k) {
  if (n <= 0 || V <= 0 || beam <= 0 || k <= 0 || n % beam != 0 || ld < V || (ld % 8) != 0) return M3P_EINVAL;
  if (k > V) return M3P_EINVAL;                              // a row supplies at most V entries to its own first k
  if (k > VSB_MAX_K || beam > VSB_MAX_BEAM) return M3P_ENOTIMPL;
  if ((long long)n * vs_nchunks(V) * VS_MAX_K >= (1ll << 31)) return M3P_ENOTIMPL;       // 32-bit block and candidate indices
  return M3P_OK;
}

// ent [n, k] as vsw_compact_kernel left it; N = the power of two at or above beam * k (at least 2, at most VSB_MAX_ENT)
__global__ __launch_bounds__(256) void vsb_merge_kernel(const float* __restrict__ pstat, const unsigned long long* __restrict__ ent,
                                                       const float* __restrict__ beam_scores, float* __restrict__ scores,
                                                       long long* __restrict__ flat_idx, float* __restrict__ lse, int V, int nchunks,
                                                       int beam, int k, int N) {
  __shared__ unsigned long long s_hi[VSB_MAX_ENT];
  __shared__ uint32_t s_lo[VSB_MAX_ENT];
  __shared__ float s_lse[VSB_MAX_BEAM];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int sent = blockIdx.x;
  const int total = beam * k;
  if (beam > VSB_MAX_BEAM || N > VSB_MAX_ENT || total > N) return;      // (the launcher's plan holds all three; uniform)
  for (int r = wv; r < beam; r += 4) {             // a wave per row: merge the chunks' (max, sum)
    const size_t row = (size_t)sent * beam + r;
    const float l = vs_row_lse(pstat + row * nchunks * 2, nchunks, lane, [](int) {});
    if (lane == 0) {
      s_lse[r] = l;
      lse[row] = l;
    }
  }
  __syncthreads();
  const unsigned long long* es = ent + (size_t)sent * total;       // (the sentence's rows are consecutive: [beam, k])
  for (int i = tid; i < N; i += 256) {
    VsKey x = {0ull, 0u};                          // past the entries: zeros, below every entry
    if (i < total) {
      const unsigned long long e = es[i];
      const int r = i / k;
      const uint32_t sk = (uint32_t)(e >> 32) & 0xFFFFu;
      const float bsc = beam_scores ? beam_scores[(size_t)sent * beam + r] : 0.f;
      const float sc = (vs_value16(sk) - s_lse[r]) + bsc;
      x.hi = (unsigned long long)vs_sortable32(sc) << 32 | (unsigned long long)(uint32_t)(0xFFFF - r) << 16 | sk;
      x.lo = (uint32_t)e;                          // ~word
    }
    s_hi[i] = x.hi;
    s_lo[i] = x.lo;
  }
  __syncthreads();
  for (int k2 = 2; k2 <= N; k2 <<= 1)              // bitonic sort, descending under vs_less: the order T
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < N / 2; t += 256) {
        const int i = 2 * t - (t & (j - 1)), l = i + j;
        const VsKey a = {s_hi[i], s_lo[i]}, b = {s_hi[l], s_lo[l]};
        if (vs_less(a, b) == ((i & k2) == 0)) {
          s_hi[i] = b.hi;
          s_lo[i] = b.lo;
          s_hi[l] = a.hi;
          s_lo[l] = a.lo;
        }
      }
      __syncthreads();
    }
  for (int j = tid; j < k; j += 256) {             // (k <= total <= N)
    const VsKey win = {s_hi[j], s_lo[j]};
    const bool have = win.hi != 0ull;              // (the plan asks for k <= V: every row supplies k entries - always)
    const int r = 0xFFFF - (int)((win.hi >> 16) & 0xFFFFu);
    scores[(size_t)sent * k + j] = have ? vs_value32((uint32_t)(win.hi >> 32)) : -INFINITY;
    flat_idx[(size_t)sent * k + j] = have ? (long long)r * V + (long long)(~win.lo) : 0ll;
  }
}

}  // namespace

extern "C" {

int m3p_vocab_select_max_k(void) { return VS_MAX_K; }

int m3p_vocab_select_plan(int n, int V, int ld, int beam, int k) { return vs_plan(n, V, ld, beam, k); }

size_t m3p_vocab_select_workspace_bytes(int n, int V, int k) {
  if (n <= 0 || V <= 0 || k <= 0) return 0;
  return (size_t)n * (size_t)vs_nchunks(V) * (2 * sizeof(float) + (size_t)k * sizeof(uint32_t));
}

int m3p_vocab_select(const void* logits, int ld, int n, int V, const float* beam_scores, int beam, int k, void* workspace,
                     size_t workspace_bytes, float* scores, long long* flat_idx, float* lse, void* stream) {
  const int rc = vs_plan(n, V, ld, beam, k);
  if (rc != M3P_OK) return rc;
  if (!vs_args_ok(logits, workspace, workspace_bytes, m3p_vocab_select_workspace_bytes(n, V, k), {scores, flat_idx, lse})) return M3P_EINVAL;
  const int nchunks = vs_nchunks(V);
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

int m3p_vocab_sample_plan(int n, int V, int ld, int top_k) { return vsmp_plan(n, V, ld, top_k, 0, VS_MAX_K); }

size_t m3p_vocab_sample_workspace_bytes(int n, int V, int top_k) {
  if (n <= 0 || V <= 0 || top_k < 0) return 0;
  if (top_k > 0) return m3p_vocab_select_workspace_bytes(n, V, top_k);
  return (size_t)n * (size_t)vs_nchunks(V) * (sizeof(unsigned long long) + 2 * sizeof(float));
}

int m3p_vocab_sample(const void* logits, int ld, int n, int V, float inv_t, int top_k, uint32_t seed, void* workspace,
                     size_t workspace_bytes, long long* words, float* logprob, float* key, void* stream) {
  const int rc = m3p_vocab_sample_plan(n, V, ld, top_k);
  if (rc != M3P_OK) return rc;
  if (!vs_args_ok(logits, workspace, workspace_bytes, m3p_vocab_sample_workspace_bytes(n, V, top_k), {words, logprob}, inv_t)) return M3P_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (top_k > 0) return vsmp_launch_topk<false>(logits, ld, n, V, inv_t, top_k, 1.f, seed, workspace, words, logprob, key, nullptr, st);
  const int nchunks = vs_nchunks(V);
  unsigned long long* wkey = (unsigned long long*)workspace;
  float* pstat = (float*)(wkey + (size_t)n * nchunks);
  hipLaunchKernelGGL(vsmp_chunk_kernel<false>, dim3((unsigned)(n * nchunks)), dim3(256), 0, st, (const bf16*)logits, ld, V, nchunks,
                     inv_t, seed, wkey, pstat, (const uint32_t*)nullptr);
  M3P_CHECK_LAUNCH();
  hipLaunchKernelGGL(vsmp_merge_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, (const bf16*)logits, ld, n, V, nchunks, inv_t,
                     (const unsigned long long*)wkey, (const float*)pstat, words, logprob, key);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

int m3p_vocab_nucleus_plan(int n, int V, int ld, int top_k) { return m3p_vocab_sample_plan(n, V, ld, top_k); }

size_t m3p_vocab_nucleus_workspace_bytes(int n, int V, int top_k) {
  if (n <= 0 || V <= 0 || top_k < 0) return 0;
  const size_t plain = m3p_vocab_sample_workspace_bytes(n, V, top_k);       // (top_p >= 1 is m3p_vocab_sample itself)
  if (top_k > 0) return plain;
  const size_t nuc = vnuc_layout(n, V).bytes;
  return nuc > plain ? nuc : plain;
}

int m3p_vocab_nucleus_sample(const void* logits, int ld, int n, int V, float inv_t, int top_k, float top_p, uint32_t seed,
                             void* workspace, size_t workspace_bytes, long long* words, float* logprob, float* key, float* cut,
                             void* stream) {
  const int rc = m3p_vocab_nucleus_plan(n, V, ld, top_k);
  if (rc != M3P_OK) return rc;
  if (!vs_args_ok(logits, workspace, workspace_bytes, m3p_vocab_nucleus_workspace_bytes(n, V, top_k), {words, logprob}, inv_t, top_p)) return M3P_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (top_p >= 1.f) {                                      // no cut: today's draw, bit for bit; cut = -inf
    if (cut && hipMemsetD32Async((hipDeviceptr_t)cut, (int)0xFF800000u, (size_t)n, st) != hipSuccess) return M3P_EINVAL;
    return m3p_vocab_sample(logits, ld, n, V, inv_t, top_k, seed, workspace, workspace_bytes, words, logprob, key, stream);
  }
  if (top_k > 0) return vsmp_launch_topk<true>(logits, ld, n, V, inv_t, top_k, top_p, seed, workspace, words, logprob, key, cut, st);
  const int nchunks = vs_nchunks(V);
  const unsigned rows4 = (unsigned)((n + 3) / 4), blocks = (unsigned)(n * nchunks);
  const VnucLayout L = vnuc_layout(n, V);
  char* ws = (char*)workspace;
  unsigned long long* hist = (unsigned long long*)(ws + L.hist);
  uint32_t* fine = (uint32_t*)(ws + L.fine);
  unsigned long long* wkey = (unsigned long long*)(ws + L.wkey);
  unsigned long long* rowz = (unsigned long long*)(ws + L.rowz);
  unsigned long long* rowabove = rowz + n;
  float* pstat = (float*)(ws + L.pstat);
  uint32_t* cand = (uint32_t*)(ws + L.cand);
  int* rowbin = (int*)(ws + L.rowbin);
  uint32_t* cutkey = (uint32_t*)rowbin + n;
  float* lse = (float*)rowbin + 2 * (size_t)n;
  const float scale = ldexpf(1.f, L.shift);
  if (hipMemsetAsync(hist, 0, (size_t)n * VN_BINS * (sizeof(unsigned long long) + sizeof(uint32_t)), st) != hipSuccess) return M3P_EINVAL;
  hipLaunchKernelGGL(vs_chunk_kernel, dim3(blocks), dim3(256), 0, st, (const bf16*)logits, ld, V, nchunks, 1, pstat, cand);
  M3P_CHECK_LAUNCH();
  hipLaunchKernelGGL(vnuc_coarse_kernel, dim3(blocks), dim3(256), 0, st, (const bf16*)logits, ld, V, nchunks, inv_t, scale,
                     (const float*)pstat, hist);
  M3P_CHECK_LAUNCH();
  hipLaunchKernelGGL(vnuc_scan_kernel, dim3(rows4), dim3(256), 0, st, (const unsigned long long*)hist, n, top_p, rowz, rowabove, rowbin);
  M3P_CHECK_LAUNCH();
  hipLaunchKernelGGL(vnuc_fine_kernel, dim3(blocks), dim3(256), 0, st, (const bf16*)logits, ld, V, nchunks, (const int*)rowbin, fine);
  M3P_CHECK_LAUNCH();
  hipLaunchKernelGGL(vnuc_cut_kernel, dim3(rows4), dim3(256), 0, st, (const uint32_t*)fine, (const float*)pstat,
                     (const unsigned long long*)rowz, (const unsigned long long*)rowabove, (const int*)rowbin, n, nchunks, inv_t, top_p,
                     scale, L.shift, cutkey, lse, cut);
  M3P_CHECK_LAUNCH();
  hipLaunchKernelGGL(vsmp_chunk_kernel<true>, dim3(blocks), dim3(256), 0, st, (const bf16*)logits, ld, V, nchunks, inv_t, seed, wkey,
                     (float*)nullptr, (const uint32_t*)cutkey);
  M3P_CHECK_LAUNCH();
  hipLaunchKernelGGL(vnuc_merge_kernel, dim3(rows4), dim3(256), 0, st, (const bf16*)logits, ld, n, V, nchunks, inv_t,
                     (const unsigned long long*)wkey, (const float*)lse, words, logprob, key);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

int m3p_vocab_sample_wide_max_k(void) { return VSW_MAX_K; }

int m3p_vocab_sample_wide_plan(int n, int V, int ld, int top_k) { return vsmp_plan(n, V, ld, top_k, 1, VSW_MAX_K); }

size_t m3p_vocab_sample_wide_workspace_bytes(int n, int V, int top_k) {
  if (n <= 0 || V <= 0 || top_k < 1) return 0;
  return vsw_layout(n, V, top_k).bytes;
}

int m3p_vocab_sample_wide(const void* logits, int ld, int n, int V, float inv_t, int top_k, float top_p, uint32_t seed,
                          void* workspace, size_t workspace_bytes, long long* words, float* logprob, float* key, float* cut,
                          void* stream) {
  const int rc = m3p_vocab_sample_wide_plan(n, V, ld, top_k);
  if (rc != M3P_OK) return rc;
  if (!vs_args_ok(logits, workspace, workspace_bytes, m3p_vocab_sample_wide_workspace_bytes(n, V, top_k), {words, logprob}, inv_t, top_p)) return M3P_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const unsigned long long* ent = nullptr;
  const int rc2 = vsw_launch_select(logits, ld, n, V, top_k, workspace, st, &ent);
  if (rc2 != M3P_OK) return rc2;
  hipLaunchKernelGGL(vsw_draw_kernel, dim3((unsigned)n), dim3(256), 0, st, ent, V, top_k, vs_pow2_at_least(top_k), inv_t, top_p,
                     seed, words, logprob, key, cut);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

int m3p_vocab_select_wide_max_k(void) { return VSB_MAX_K; }

int m3p_vocab_select_wide_plan(int n, int V, int ld, int beam, int k) { return vsb_plan(n, V, ld, beam, k); }

size_t m3p_vocab_select_wide_workspace_bytes(int n, int V, int beam, int k) {
  if (n <= 0 || V <= 0 || beam <= 0 || k <= 0) return 0;
  return vsb_layout(n, V, k).bytes;
}

int m3p_vocab_select_wide(const void* logits, int ld, int n, int V, const float* beam_scores, int beam, int k, void* workspace,
                          size_t workspace_bytes, float* scores, long long* flat_idx, float* lse, void* stream) {
  const int rc = vsb_plan(n, V, ld, beam, k);
  if (rc != M3P_OK) return rc;
  if (!vs_args_ok(logits, workspace, workspace_bytes, m3p_vocab_select_wide_workspace_bytes(n, V, beam, k), {scores, flat_idx, lse})) return M3P_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int nchunks = vs_nchunks(V);
  const VsbLayout B = vsb_layout(n, V, k);
  float* pstat = (float*)((char*)workspace + B.pstat);
  uint32_t* cand = (uint32_t*)((char*)workspace + B.cand);
  // the chunks' (max, sum) exactly as m3p_vocab_select takes them (the sum does not depend on k): the same lse bits
  hipLaunchKernelGGL(vs_chunk_kernel, dim3((unsigned)(n * nchunks)), dim3(256), 0, st, (const bf16*)logits, ld, V, nchunks, 1, pstat,
                     cand);
  M3P_CHECK_LAUNCH();
  const unsigned long long* ent = nullptr;
  const int rc2 = vsw_launch_select(logits, ld, n, V, k, workspace, st, &ent);
  if (rc2 != M3P_OK) return rc2;
  hipLaunchKernelGGL(vsb_merge_kernel, dim3((unsigned)(n / beam)), dim3(256), 0, st, (const float*)pstat, ent, beam_scores, scores,
                     flat_idx, lse, V, nchunks, beam, k, vs_pow2_at_least(beam * k));
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

}  // extern "C"
