// Optimizer path of Trainer.optimize (M3P/src/xtrainer.py:205-243) on flat fp32 arenas:
//   * global gradient L2 norm (clip_grad_norm_, xtrainer.py:225) as one streaming reduction
//   * Adam.step (M3P/src/optim.py:45-86) fused with the clip scaling, the refresh of the
//     bf16 working copy the GEMMs read, and zero_grad — one pass over p, g, m, v.
//   * bf16 transposes of the weight copies used by the data-gradient GEMMs.
// All HBM-bound: 16-byte accesses, grid-stride.
#include "common.hpp"
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

namespace {

__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, size_t n4, double* __restrict__ out) {
  __shared__ double red[4];
  float acc = 0.f;
  // four 16-byte loads in flight per thread: the bucket-sized launches of the sharded data-parallel step (15 of ~75 MB) ran
  // at 2 TB/s with one
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 3 * stride < n4; i += 4 * stride) {
    f32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g + 4 * (i + u * stride)));
#pragma unroll
    for (int u = 0; u < 4; ++u) acc += (v[u][0] * v[u][0] + v[u][1] * v[u][1]) + (v[u][2] * v[u][2] + v[u][3] * v[u][3]);
  }
  for (; i < n4; i += stride) {
    const f32x4 v = Vec4<float>::load(g + 4 * i);
    acc += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = (double)acc;
  __syncthreads();
  if (threadIdx.x == 0) unsafeAtomicAdd(out, (red[0] + red[1]) + (red[2] + red[3]));
}

// the same over up to SUMSQ_MAX_RANGES ranges of one buffer in ONE launch (the sharded data-parallel step owns a piece of every
// bucket: fifteen launches of ~30 us for what one launch does in the time the bytes take).  Blocks are dealt to the ranges
// in proportion to their sizes (blk0[r] = first block of range r).
constexpr int SUMSQ_MAX_RANGES = 32;
struct SumsqRanges {
  const float* g[SUMSQ_MAX_RANGES];
  unsigned long long n4[SUMSQ_MAX_RANGES];
  int blk0[SUMSQ_MAX_RANGES + 1];
  int n;
};
__global__ __launch_bounds__(256) void sumsq_ranges_kernel(SumsqRanges a, double* __restrict__ out) {
  __shared__ double red[4];
  int r = 0;
  while (r + 1 < a.n && (int)blockIdx.x >= a.blk0[r + 1]) ++r;
  const float* __restrict__ g = a.g[r];
  const size_t n4 = a.n4[r];
  const size_t stride = (size_t)(a.blk0[r + 1] - a.blk0[r]) * blockDim.x;
  size_t i = (size_t)((int)blockIdx.x - a.blk0[r]) * blockDim.x + threadIdx.x;
  float acc = 0.f;
  for (; i + 3 * stride < n4; i += 4 * stride) {
    f32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g + 4 * (i + u * stride)));
#pragma unroll
    for (int u = 0; u < 4; ++u) acc += (v[u][0] * v[u][0] + v[u][1] * v[u][1]) + (v[u][2] * v[u][2] + v[u][3] * v[u][3]);
  }
  for (; i < n4; i += stride) {
    const f32x4 v = Vec4<float>::load(g + 4 * i);
    acc += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = (double)acc;
  __syncthreads();
  if (threadIdx.x == 0) unsafeAtomicAdd(out, (red[0] + red[1]) + (red[2] + red[3]));
}

struct AdamArgs {
  float* p; float* g; float* m; float* v; bf16* w16;
  size_t n4;
  float lr, beta1, beta2, eps, weight_decay, step_size;
  const double* gnorm_sq;   // device scalar: sum of squares of ALL gradients (or NULL)
  float max_norm;           // <= 0: no clipping
  float grad_scale;         // extra multiplier on g (1/world for DP averaging, loss-scale inverse)
  int zero_grad;
};

__global__ __launch_bounds__(256) void adam_kernel(AdamArgs a) {
  float coef = a.grad_scale;
  if (a.gnorm_sq && a.max_norm > 0.f) {
    // torch.nn.utils.clip_grad_norm_: coef = max_norm / (norm + 1e-6), clamped to 1
    const float norm = (float)sqrt(*a.gnorm_sq) * a.grad_scale;
    const float c = a.max_norm / (norm + 1e-6f);
    coef *= (c < 1.f) ? c : 1.f;
  }
  const float ob1 = 1.f - a.beta1, ob2 = 1.f - a.beta2, wdl = a.weight_decay * a.lr;
  // Nine streams (4 read, 5 written) of data touched once per step: non-temporal accesses keep them out of the way
  // of the bf16 weights / activations the next forward re-reads, and two 16-byte quads per thread and iteration put
  // eight loads in flight before the first use.
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < a.n4; i0 += 2 * stride) {
    const size_t i1 = i0 + stride;
    const bool two = i1 < a.n4;
    f32x4 p[2], g[2], m[2], v[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const size_t i = u ? i1 : i0;
      if (u == 0 || two) {
        p[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.p + 4 * i));
        g[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.g + 4 * i));
        m[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.m + 4 * i));
        v[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.v + 4 * i));
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const size_t i = u ? i1 : i0;
      if (u == 0 || two) {
        const f32x4 gc = g[u] * coef;
        const f32x4 mn = m[u] * a.beta1 + gc * ob1;
        const f32x4 vn = v[u] * a.beta2 + gc * gc * ob2;
        f32x4 pn = p[u];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float denom = sqrtf(vn[j]) + a.eps;
          if (wdl != 0.f) pn[j] -= wdl * pn[j];
          pn[j] -= a.step_size * (mn[j] / denom);
        }
        __builtin_nontemporal_store(pn, reinterpret_cast<f32x4*>(a.p + 4 * i));
        __builtin_nontemporal_store(mn, reinterpret_cast<f32x4*>(a.m + 4 * i));
        __builtin_nontemporal_store(vn, reinterpret_cast<f32x4*>(a.v + 4 * i));
        if (a.w16) Vec4<bf16>::store(a.w16 + 4 * i, pn);       // (re-read by the very next forward: default policy)
        if (a.zero_grad) __builtin_nontemporal_store(f32x4{0.f, 0.f, 0.f, 0.f}, reinterpret_cast<f32x4*>(a.g + 4 * i));
      }
    }
  }
}

// bf16 -> fp8 (e4m3) / bf8 (e5m2) with a per-tensor scale, saturating, + running max |x| for the next step's scale
// (delayed scaling, m3p_amd/fp8.py).  8 elements (16 B in, 8 B out) per thread and iteration.
template <bool BF8>
__global__ __launch_bounds__(256) void quant_fp8_kernel(const bf16* __restrict__ src, int ld_src, uint8_t* __restrict__ dst, int ld_dst,
                                                        int rows, int cols8, const float* __restrict__ scale, float* __restrict__ amax) {
  const float s = scale ? *scale : 1.f;
  constexpr float kMax = BF8 ? 57344.f : 448.f;
  float mx = 0.f;
  const size_t total = (size_t)rows * cols8;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / cols8), c = (int)(i - (size_t)r * cols8) * 8;
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(src + (size_t)r * ld_src + c);
    float f[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float x = (float)v[e];
      mx = fmaxf(mx, fabsf(x));
      f[e] = fminf(fmaxf(x * s, -kMax), kMax);
    }
    int w0 = 0, w1 = 0;
    if (BF8) {
      w0 = __builtin_amdgcn_cvt_pk_bf8_f32(f[0], f[1], w0, false); w0 = __builtin_amdgcn_cvt_pk_bf8_f32(f[2], f[3], w0, true);
      w1 = __builtin_amdgcn_cvt_pk_bf8_f32(f[4], f[5], w1, false); w1 = __builtin_amdgcn_cvt_pk_bf8_f32(f[6], f[7], w1, true);
    } else {
      w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], w0, false); w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], w0, true);
      w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], w1, false); w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], w1, true);
    }
    *reinterpret_cast<int2*>(dst + (size_t)r * ld_dst + c) = int2{w0, w1};
  }
  if (amax) {
    // One candidate per workgroup, and only if it beats the value already there: thousands of same-address atomics
    // from every wave cost ~200 us per launch (they serialise at the memory side), the filtered ones a few.
    __shared__ float wmax[4];
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
      mx = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
      unsigned int* slot = reinterpret_cast<unsigned int*>(amax);
      // non-negative floats order like their bit patterns: an integer atomic max is a float max.  The plain read may be
      // stale (another XCD's L2) - then it is too small and the atomic merely runs without effect.
      if (__float_as_uint(mx) > __builtin_nontemporal_load(slot)) atomicMax(slot, __float_as_uint(mx));
    }
  }
}

// Batched form for the weights (fp8 path: ~120 matrices per optimizer step, 8-10 us of launch each on their own): one
// grid.y slice per matrix.  desc[i] = {src, dst, scale ptr, amax ptr or 0, elements / 8} (int64 each); e4m3 only.
__global__ __launch_bounds__(256) void quant_fp8_batch_kernel(const long long* __restrict__ desc) {
  const long long* dsc = desc + 5 * blockIdx.y;
  const bf16* src = reinterpret_cast<const bf16*>(dsc[0]);
  uint8_t* dst = reinterpret_cast<uint8_t*>(dsc[1]);
  const float s = *reinterpret_cast<const float*>(dsc[2]);
  float* amax = reinterpret_cast<float*>(dsc[3]);
  const size_t total = (size_t)dsc[4];
  float mx = 0.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(src + 8 * i);
    float f[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float x = (float)v[e];
      mx = fmaxf(mx, fabsf(x));
      f[e] = fminf(fmaxf(x * s, -448.f), 448.f);
    }
    int w0 = 0, w1 = 0;
    w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], w0, false); w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], w0, true);
    w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], w1, false); w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], w1, true);
    *reinterpret_cast<int2*>(dst + 8 * i) = int2{w0, w1};
  }
  if (amax) {
    __shared__ float wmax[4];
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
      mx = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
      unsigned int* slot = reinterpret_cast<unsigned int*>(amax);
      if (__float_as_uint(mx) > __builtin_nontemporal_load(slot)) atomicMax(slot, __float_as_uint(mx));
    }
  }
}

// dst[c][r] = src[r][c], 64x64 tiles through LDS; ld_dst >= rows (pad columns untouched)
__global__ __launch_bounds__(256) void transpose_bf16_kernel(const bf16* __restrict__ src, bf16* __restrict__ dst,
                                                             int rows, int cols, int ld_src, int ld_dst) {
  __shared__ bf16 tile[64][66];
  const int tr = blockIdx.y * 64, tc = blockIdx.x * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int i = ty; i < 64; i += 4) {
    const int r = tr + i, c = tc + tx;
    tile[i][tx] = (r < rows && c < cols) ? src[(size_t)r * ld_src + c] : (bf16)0.f;
  }
  __syncthreads();
  for (int i = ty; i < 64; i += 4) {
    const int c = tc + i, r = tr + tx;
    if (c < cols && r < rows) dst[(size_t)c * ld_dst + r] = tile[tx][i];
  }
}

// batched variant: desc[i] = {src, dst, rows, cols, ld_src, ld_dst} (int64 each), one grid.y slice per matrix
__global__ __launch_bounds__(256) void transpose_batch_kernel(const long long* __restrict__ desc) {
  __shared__ bf16 tile[64][72];       // 144-byte rows: 16-byte aligned for the row-wise stores, 4-bank skew for the column reads
  const long long* dsc = desc + 6 * blockIdx.y;
  const bf16* src = reinterpret_cast<const bf16*>(dsc[0]);
  bf16* dst = reinterpret_cast<bf16*>(dsc[1]);
  const int rows = (int)dsc[2], cols = (int)dsc[3], ld_src = (int)dsc[4], ld_dst = (int)dsc[5];
  const int tiles_c = (cols + 63) / 64, tiles_r = (rows + 63) / 64;
  if ((int)blockIdx.x >= tiles_c * tiles_r) return;
  const int tr = (blockIdx.x / tiles_c) * 64, tc = (blockIdx.x % tiles_c) * 64;
  // whole 64 x 64 tiles of 16-byte-aligned matrices (every layer weight): 16-byte accesses on both sides - a lane reads 8
  // consecutive columns of a row and later writes 8 consecutive rows of a column (2-byte accesses moved 2.2 TB/s: r02)
  const bool fast = tr + 64 <= rows && tc + 64 <= cols && (ld_src & 7) == 0 && (ld_dst & 7) == 0 &&
                    (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
  if (fast) {
    const int q = threadIdx.x & 7, rr = threadIdx.x >> 3;          // 8 lanes per 128-byte row piece, 32 rows per pass
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int r = rr + 32 * p;
      *reinterpret_cast<bf16x8*>(&tile[r][8 * q]) = *reinterpret_cast<const bf16x8*>(src + (size_t)(tr + r) * ld_src + tc + 8 * q);
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int c = rr + 32 * p;                                   // output row = source column
      bf16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = tile[8 * q + e][c];
      *reinterpret_cast<bf16x8*>(dst + (size_t)(tc + c) * ld_dst + tr + 8 * q) = o;
    }
    return;
  }
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int i = ty; i < 64; i += 4) {
    const int r = tr + i, c = tc + tx;
    tile[i][tx] = (r < rows && c < cols) ? src[(size_t)r * ld_src + c] : (bf16)0.f;
  }
  __syncthreads();
  for (int i = ty; i < 64; i += 4) {
    const int c = tc + i, r = tr + tx;
    if (c < cols && r < rows) dst[(size_t)c * ld_dst + r] = tile[tx][i];
  }
}

// h = gelu_erf(u), bf16 in/out, 16-byte accesses (the FFN activation as its own streaming
// pass: 129 M elements at HBM speed cost less than the same VALU work serialised behind the
// MFMA stream of the persistent GEMM — see DESIGN.md)
template <bool GRAD>
__global__ __launch_bounds__(256) void gelu_fwd_kernel(const bf16* u, bf16* __restrict__ h, bf16* dh, size_t n8) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(u + 8 * i);
    bf16x8 o, d;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float x = (float)v[j];
      const GeluParts g = gelu_parts(x);        // Phi(x), phi(x) share one exp
      o[j] = (bf16)(x * g.cdf);
      if (GRAD) d[j] = (bf16)(g.cdf + x * g.pdf);
    }
    *reinterpret_cast<bf16x8*>(h + 8 * i) = o;
    if (GRAD) *reinterpret_cast<bf16x8*>(dh + 8 * i) = d;     // may overwrite u: each thread has read its 8 values
  }
}

// The same pass leaving gelu'(u) as one byte per element in the eight-wave GEMM's fragment order (common.hpp): a workgroup
// takes 16 rows x 256 columns = one row block of the four column quarters of a tile (4 KB of codes).  Phase 1 walks the
// rows in 16-byte pieces (coalesced u reads and h writes) and drops the codes into LDS in row order; phase 2 reads them in
// accumulator order (lane = 16 fg + fr holds columns 16 j + 4 fg .. + 3 of row fr) and writes 1 KB per wave, coalesced.
__global__ __launch_bounds__(256) void gelu_fwd_gq_kernel(const bf16* __restrict__ u, bf16* __restrict__ h, uint8_t* __restrict__ gq,
                                                          int N, int tiles_n, int nblocks) {
  __shared__ __attribute__((aligned(16))) uint8_t codes[16][256 + 16];
  const int t = threadIdx.x;
  for (int b = blockIdx.x; b < nblocks; b += gridDim.x) {
    const int rb = b / tiles_n, tn = b - rb * tiles_n;        // 16-row block, column tile
    const size_t row0 = (size_t)rb * 16;
    const int col0 = tn * 256;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int r = (t >> 5) + 8 * half, c = (t & 31) * 8;
      const size_t off = (row0 + r) * (size_t)N + col0 + c;
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(u + off);
      bf16x8 o;
      uint32_t lo = 0, hi = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float x = (float)v[j];
        const GeluParts g = gelu_parts(x);
        o[j] = (bf16)(x * g.cdf);
        const uint32_t q = gelu_grad_code(g.cdf + x * g.pdf);
        if (j < 4) lo |= q << (8 * j); else hi |= q << (8 * (j - 4));
      }
      *reinterpret_cast<bf16x8*>(h + off) = o;
      *reinterpret_cast<uint2*>(&codes[r][c]) = uint2{lo, hi};
    }
    __syncthreads();
    {
      const int wn = t >> 6, l = t & 63, fr = l & 15, fg = l >> 4;
      uint4 q;
      q.x = *reinterpret_cast<const uint32_t*>(&codes[fr][wn * 64 + 0 + fg * 4]);
      q.y = *reinterpret_cast<const uint32_t*>(&codes[fr][wn * 64 + 16 + fg * 4]);
      q.z = *reinterpret_cast<const uint32_t*>(&codes[fr][wn * 64 + 32 + fg * 4]);
      q.w = *reinterpret_cast<const uint32_t*>(&codes[fr][wn * 64 + 48 + fg * 4]);
      const int tm = rb >> 4, ib = rb & 15, wm = ib >> 3, i = ib & 7;
      *reinterpret_cast<uint4*>(gq + gq_block_offset(tm, tn, tiles_n, wm * 4 + wn, i) + l * 16) = q;
    }
    __syncthreads();
  }
}

// The same pass also emitting the e4m3 copy of h the fp8 lin2 product reads (fp8 path: a separate quantisation pass would
// read the 280-MB activation again) + the running max |h| for the next step's scale.  The 8-bit value is the
// quantisation of the ROUNDED bf16 h, i.e. exactly what m3p_quant_fp8 would produce from h.
__global__ __launch_bounds__(256) void gelu_fwd_q8_kernel(const bf16* __restrict__ u, bf16* __restrict__ h, uint8_t* __restrict__ h8,
                                                          size_t n8, const float* __restrict__ scale, float* __restrict__ amax) {
  const float s = *scale;
  float mx = 0.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(u + 8 * i);
    bf16x8 o;
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float x = (float)v[j];
      const GeluParts g = gelu_parts(x);
      o[j] = (bf16)(x * g.cdf);
      const float hr = (float)o[j];
      mx = fmaxf(mx, fabsf(hr));
      f[j] = fminf(fmaxf(hr * s, -448.f), 448.f);
    }
    *reinterpret_cast<bf16x8*>(h + 8 * i) = o;
    int w0 = 0, w1 = 0;
    w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], w0, false); w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], w0, true);
    w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], w1, false); w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], w1, true);
    *reinterpret_cast<int2*>(h8 + 8 * i) = int2{w0, w1};
  }
  if (amax) {
    __shared__ float wmax[4];
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
      mx = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
      unsigned int* slot = reinterpret_cast<unsigned int*>(amax);
      if (__float_as_uint(mx) > __builtin_nontemporal_load(slot)) atomicMax(slot, __float_as_uint(mx));
    }
  }
}

// du = dy * gelu_erf'(u): backward of a GELU that sits between a Linear and a LayerNorm
// (BertPredictionHeadTransform, transformer.py:595-606), bf16 in/out, 16-byte accesses
__global__ __launch_bounds__(256) void gelu_bwd_kernel(const bf16* __restrict__ dy, const bf16* __restrict__ u,
                                                       bf16* __restrict__ du, size_t n8) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
    const bf16x8 g = *reinterpret_cast<const bf16x8*>(dy + 8 * i);
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(u + 8 * i);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (bf16)((float)g[j] * gelu_erf_grad_f((float)v[j]));
    *reinterpret_cast<bf16x8*>(du + 8 * i) = o;
  }
}

// Masked-region feature regression loss (xtrainer.py:2346): one wave per row,
// row_sq[i] = sum_j (pred[i][j] - tgt[i][j])^2 and dpred = 2 (pred - tgt) * gscale in bf16.
__global__ __launch_bounds__(256) void mse_fwd_bwd_kernel(const bf16* __restrict__ pred, int ld_pred, const float* __restrict__ tgt,
                                                          int ld_tgt, bf16* __restrict__ dpred, float* __restrict__ row_sq,
                                                          int rows, int cols, float gscale) {
  const int lane = threadIdx.x & 63;
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row >= rows) return;
  const bf16* pr = pred + (size_t)row * ld_pred;
  const float* tr = tgt + (size_t)row * ld_tgt;
  bf16* dr = dpred + (size_t)row * ld_pred;
  float acc = 0.f;
  for (int c = lane * 4; c < cols; c += 256) {
    const f32x4 p = Vec4<bf16>::load(pr + c);
    const f32x4 t = *reinterpret_cast<const f32x4*>(tr + c);
    const f32x4 e = p - t;
    acc += (e[0] * e[0] + e[1] * e[1]) + (e[2] * e[2] + e[3] * e[3]);
    Vec4<bf16>::store(dr + c, e * (2.f * gscale));
  }
  acc = wave_sum(acc);
  if (lane == 0) row_sq[row] = acc;
}

}  // namespace

extern "C" {

int m3p_gelu_bwd(const void* dy, const void* u, void* du, long long n, void* stream) {
  if (n <= 0 || (n % 8) != 0 || ((uintptr_t)dy & 15) || ((uintptr_t)u & 15) || ((uintptr_t)du & 15)) return M3P_EINVAL;
  const size_t n8 = (size_t)n / 8;
  const int blocks = (int)((n8 + 255) / 256 < 8192 ? (n8 + 255) / 256 : 8192);
  hipLaunchKernelGGL(gelu_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const bf16*)dy, (const bf16*)u, (bf16*)du, n8);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

int m3p_mse_fwd_bwd(const void* pred, int ld_pred, const float* tgt, int ld_tgt, void* dpred, float* row_sq, int rows,
                    int cols, float grad_scale, void* stream) {
  if (rows <= 0 || cols <= 0 || (cols % 4) != 0 || (ld_pred % 4) != 0 || (ld_tgt % 4) != 0) return M3P_EINVAL;
  if (((uintptr_t)pred & 7) || ((uintptr_t)dpred & 7) || ((uintptr_t)tgt & 15)) return M3P_EINVAL;
  hipLaunchKernelGGL(mse_fwd_bwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const bf16*)pred, ld_pred, tgt,
                     ld_tgt, (bf16*)dpred, row_sq, rows, cols, grad_scale);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

int m3p_gelu_fwd(const void* u, void* h, void* dh, long long n, void* stream) {
  if (n <= 0 || (n % 8) != 0 || ((uintptr_t)u & 15) || ((uintptr_t)h & 15) || ((uintptr_t)dh & 15)) return M3P_EINVAL;
  const size_t n8 = (size_t)n / 8;
  const int blocks = (int)((n8 + 255) / 256 < 8192 ? (n8 + 255) / 256 : 8192);
  if (dh)
    hipLaunchKernelGGL(gelu_fwd_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const bf16*)u, (bf16*)h, (bf16*)dh, n8);
  else
    hipLaunchKernelGGL(gelu_fwd_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const bf16*)u, (bf16*)h, (bf16*)nullptr, n8);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

int m3p_gelu_fwd_gq(const void* u, void* h, void* gq, int M, int N, void* stream) {
  if (M <= 0 || N <= 0 || (M % 256) || (N % 256) || !u || !h || !gq) return M3P_EINVAL;
  if (((uintptr_t)u & 15) || ((uintptr_t)h & 15) || ((uintptr_t)gq & 15)) return M3P_EINVAL;
  const long long nb = (long long)(M / 16) * (N / 256);
  if (nb > 0x7fffffffLL) return M3P_EINVAL;
  const int blocks = (int)(nb < 16384 ? nb : 16384);
  hipLaunchKernelGGL(gelu_fwd_gq_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const bf16*)u, (bf16*)h, (uint8_t*)gq, N,
                     N / 256, (int)nb);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

int m3p_gelu_fwd_q8(const void* u, void* h, void* h8, long long n, const float* scale, float* amax, void* stream) {
  if (n <= 0 || (n % 8) != 0 || ((uintptr_t)u & 15) || ((uintptr_t)h & 15) || ((uintptr_t)h8 & 7) || !scale) return M3P_EINVAL;
  const size_t n8 = (size_t)n / 8;
  const int blocks = (int)((n8 + 255) / 256 < 8192 ? (n8 + 255) / 256 : 8192);
  hipLaunchKernelGGL(gelu_fwd_q8_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const bf16*)u, (bf16*)h, (uint8_t*)h8, n8,
                     scale, amax);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

int m3p_transpose_batch_bf16(const long long* desc, int n_desc, int max_tiles, void* stream) {
  if (n_desc <= 0 || max_tiles <= 0) return M3P_EINVAL;
  hipLaunchKernelGGL(transpose_batch_kernel, dim3(max_tiles, n_desc), dim3(256), 0, (hipStream_t)stream, desc);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}


int m3p_quant_fp8(const void* src, int ld_src, void* dst, int ld_dst, int rows, int cols, const float* scale, float* amax,
                  int bf8, void* stream) {
  if (rows <= 0 || cols <= 0 || (cols % 8) != 0 || (ld_src % 8) != 0 || (ld_dst % 8) != 0 || ld_src < cols || ld_dst < cols)
    return M3P_EINVAL;
  if (((uintptr_t)src & 15) || ((uintptr_t)dst & 7)) return M3P_EINVAL;
  const size_t total = (size_t)rows * (cols / 8);
  const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  if (bf8)
    hipLaunchKernelGGL(quant_fp8_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const bf16*)src, ld_src,
                       (uint8_t*)dst, ld_dst, rows, cols / 8, scale, amax);
  else
    hipLaunchKernelGGL(quant_fp8_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const bf16*)src, ld_src,
                       (uint8_t*)dst, ld_dst, rows, cols / 8, scale, amax);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

int m3p_quant_fp8_batch(const long long* desc, int n_desc, int blocks_per_matrix, void* stream) {
  if (!desc || n_desc <= 0 || blocks_per_matrix <= 0 || blocks_per_matrix > 4096) return M3P_EINVAL;
  hipLaunchKernelGGL(quant_fp8_batch_kernel, dim3(blocks_per_matrix, n_desc), dim3(256), 0, (hipStream_t)stream, desc);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

int m3p_sumsq_f32(const float* g, long long n, double* out, void* stream) {
  if (n <= 0 || (n % 4) != 0 || ((uintptr_t)g & 15)) return M3P_EINVAL;
  const size_t n4 = (size_t)n / 4;
  const size_t want = (n4 + 1023) / 1024;      // ~four quads per thread
  const int blocks = (int)(want < 1 ? 1 : (want < 2048 ? want : 2048));
  hipLaunchKernelGGL(sumsq_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, g, n4, out);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

int m3p_sumsq_ranges_f32(const float* base, const long long* starts, const long long* counts, int n_ranges, double* out, void* stream) {
  if (!base || !starts || !counts || !out || n_ranges <= 0) return M3P_EINVAL;
  int done = 0;
  while (done < n_ranges) {            // (more ranges than one launch's descriptor holds: several launches)
    SumsqRanges a;
    a.n = 0;
    long long total4 = 0;
    for (int r = done; r < n_ranges && a.n < SUMSQ_MAX_RANGES; ++r) {
      if (counts[r] < 0 || (counts[r] % 4) != 0 || starts[r] < 0 || (((uintptr_t)(base + starts[r])) & 15)) return M3P_EINVAL;
      if (counts[r] == 0) continue;
      a.g[a.n] = base + starts[r];
      a.n4[a.n] = (unsigned long long)counts[r] / 4;
      total4 += counts[r] / 4;
      ++a.n;
    }
    int taken = 0;
    for (int r = done, k = 0; r < n_ranges && k < SUMSQ_MAX_RANGES; ++r) { if (counts[r] != 0) ++k; ++taken; }
    done += taken;
    if (a.n == 0) continue;
    // ~four quads per thread, at most 2048 blocks, at least one block per range
    long long want = (total4 + 1023) / 1024;
    if (want > 2048) want = 2048;
    if (want < a.n) want = a.n;
    int b = 0;
    for (int r = 0; r < a.n; ++r) {
      a.blk0[r] = b;
      long long share = (long long)((double)a.n4[r] / (double)total4 * (double)want);
      if (share < 1) share = 1;
      b += (int)share;
    }
    a.blk0[a.n] = b;
    hipLaunchKernelGGL(sumsq_ranges_kernel, dim3(b), dim3(256), 0, (hipStream_t)stream, a, out);
    M3P_CHECK_LAUNCH();
  }
  return M3P_OK;
}

// The same update over several pieces of the flat arenas in ONE launch (round 5): blocks are dealt to the pieces in proportion
// to their sizes like m3p_sumsq_ranges_f32.  A sharded data-parallel rank steps fifteen bucket shards per optimizer step, the
// single-GPU step two pieces (the lazily zeroed vocabulary range and the rest): per piece a launch ramps up and drains on its
// own - fifteen launches streamed the one-rank wrapped step's 9.5 GB in 2.00 ms where two take 1.61 (profiles/r05_dp_prof.txt).
constexpr int ADAM_MAX_RANGES = 32;
struct AdamRanges {
  AdamArgs c;                                  // common fields; p / g / m / v / w16 = the arenas' bases, n4 / step_size / zero_grad unused
  unsigned long long start4[ADAM_MAX_RANGES];  // first quad of the piece
  unsigned long long n4[ADAM_MAX_RANGES];
  float step_size[ADAM_MAX_RANGES];
  int zero_grad[ADAM_MAX_RANGES];
  int blk0[ADAM_MAX_RANGES + 1];
  int n;
};
// loop shape of the fused update over the arena: every shape swept measured the same 6.1 TB/s (profiles/r05_adam_sweep.txt)
constexpr int ADAM_Q = 2;            // 16-byte quads per thread and trip (x 4 read streams = loads in flight before the first use)
constexpr int ADAM_MAXBLK = 4096;    // blocks per launch at most
}  // extern "C" (a template has C++ linkage)

namespace {
// GUARD: the non-finite guard's form (include/m3p_hip.h, m3p_step_guard).  *skip is one word every workgroup reads before
// anything else; on a skipped step the workgroup stores zeros over its share of a piece that asks for them - the same
// elements it would have updated - and loads nothing from the arenas.  GUARD = false is the launch as it always was.
template <bool GUARD>
__global__ __launch_bounds__(256) void adam_ranges_kernel(AdamRanges a, const int* __restrict__ skip) {
  int r = 0;
  while (r + 1 < a.n && (int)blockIdx.x >= a.blk0[r + 1]) ++r;
  if (GUARD && *skip != 0) {
    if (a.zero_grad[r] == 0) return;
    float* const G = a.c.g + 4 * (size_t)a.start4[r];
    const size_t n4 = (size_t)a.n4[r];
    const size_t stride = (size_t)(a.blk0[r + 1] - a.blk0[r]) * blockDim.x;
    for (size_t i = (size_t)((int)blockIdx.x - a.blk0[r]) * blockDim.x + threadIdx.x; i < n4; i += stride)
      __builtin_nontemporal_store(f32x4{0.f, 0.f, 0.f, 0.f}, reinterpret_cast<f32x4*>(G + 4 * i));
    return;
  }
  float coef = a.c.grad_scale;
  if (a.c.gnorm_sq && a.c.max_norm > 0.f) {
    const float norm = (float)sqrt(*a.c.gnorm_sq) * a.c.grad_scale;
    const float cc = a.c.max_norm / (norm + 1e-6f);
    coef *= (cc < 1.f) ? cc : 1.f;
  }
  const float ob1 = 1.f - a.c.beta1, ob2 = 1.f - a.c.beta2, wdl = a.c.weight_decay * a.c.lr;
  const float step_size = a.step_size[r];
  const bool zero = a.zero_grad[r] != 0;
  const size_t base = (size_t)a.start4[r], n4 = (size_t)a.n4[r];
  float* const P = a.c.p + 4 * base; float* const G = a.c.g + 4 * base; float* const M = a.c.m + 4 * base; float* const V = a.c.v + 4 * base;
  bf16* const W = a.c.w16 ? a.c.w16 + 4 * base : nullptr;
  const size_t stride = (size_t)(a.blk0[r + 1] - a.blk0[r]) * blockDim.x;
  constexpr int Q = ADAM_Q;
  for (size_t i0 = (size_t)((int)blockIdx.x - a.blk0[r]) * blockDim.x + threadIdx.x; i0 < n4; i0 += Q * stride) {
    f32x4 p[Q], g[Q], m[Q], v[Q];
#pragma unroll
    for (int u = 0; u < Q; ++u) {
      const size_t i = i0 + u * stride;
      if (u == 0 || i < n4) {
        p[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(P + 4 * i));
        g[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(G + 4 * i));
        m[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(M + 4 * i));
        v[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(V + 4 * i));
      }
    }
#pragma unroll
    for (int u = 0; u < Q; ++u) {
      const size_t i = i0 + u * stride;
      if (u == 0 || i < n4) {
        const f32x4 gc = g[u] * coef;
        const f32x4 mn = m[u] * a.c.beta1 + gc * ob1;
        const f32x4 vn = v[u] * a.c.beta2 + gc * gc * ob2;
        f32x4 pn = p[u];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float denom = sqrtf(vn[j]) + a.c.eps;
          if (wdl != 0.f) pn[j] -= wdl * pn[j];
          pn[j] -= step_size * (mn[j] / denom);
        }
        __builtin_nontemporal_store(pn, reinterpret_cast<f32x4*>(P + 4 * i));
        __builtin_nontemporal_store(mn, reinterpret_cast<f32x4*>(M + 4 * i));
        __builtin_nontemporal_store(vn, reinterpret_cast<f32x4*>(V + 4 * i));
        if (W) Vec4<bf16>::store(W + 4 * i, pn);
        if (zero) __builtin_nontemporal_store(f32x4{0.f, 0.f, 0.f, 0.f}, reinterpret_cast<f32x4*>(G + 4 * i));
      }
    }
  }
}

}  // namespace
extern "C" {

int m3p_adam_step_ranges(float* p, float* g, float* m, float* v, void* w16, const long long* starts, const long long* counts,
                         const float* step_sizes, const int* zero_grad, int n_ranges, float lr, float beta1, float beta2, float eps,
                         float weight_decay, const double* gnorm_sq, float max_norm, float grad_scale, void* stream) {
  return m3p_adam_step_ranges_guarded(p, g, m, v, w16, starts, counts, step_sizes, zero_grad, n_ranges, lr, beta1, beta2, eps,
                                      weight_decay, gnorm_sq, max_norm, grad_scale, nullptr, stream);
}

int m3p_adam_step_ranges_guarded(float* p, float* g, float* m, float* v, void* w16, const long long* starts, const long long* counts,
                                 const float* step_sizes, const int* zero_grad, int n_ranges, float lr, float beta1, float beta2,
                                 float eps, float weight_decay, const double* gnorm_sq, float max_norm, float grad_scale,
                                 const int* skip, void* stream) {
  if ((uintptr_t)skip & 3) return M3P_EINVAL;
  if (!p || !g || !m || !v || !starts || !counts || !step_sizes || !zero_grad || n_ranges <= 0) return M3P_EINVAL;
  if (((uintptr_t)p & 15) || ((uintptr_t)g & 15) || ((uintptr_t)m & 15) || ((uintptr_t)v & 15) || ((uintptr_t)w16 & 7)) return M3P_EINVAL;
  for (int r = 0; r < n_ranges; ++r)
    if (counts[r] < 0 || (counts[r] % 4) != 0 || starts[r] < 0 || (starts[r] % 4) != 0) return M3P_EINVAL;
  int done = 0;
  while (done < n_ranges) {
    AdamRanges a;
    a.c = AdamArgs{p, g, m, v, (bf16*)w16, 0, lr, beta1, beta2, eps, weight_decay, 0.f, gnorm_sq, max_norm,
                   grad_scale == 0.f ? 1.f : grad_scale, 0};
    a.n = 0;
    long long total4 = 0;
    for (; done < n_ranges && a.n < ADAM_MAX_RANGES; ++done) {
      if (counts[done] == 0) continue;
      a.start4[a.n] = (unsigned long long)starts[done] / 4;
      a.n4[a.n] = (unsigned long long)counts[done] / 4;
      a.step_size[a.n] = step_sizes[done];
      a.zero_grad[a.n] = zero_grad[done];
      total4 += counts[done] / 4;
      ++a.n;
    }
    if (a.n == 0) continue;
    long long want = (total4 + 255) / 256;      // one quad per thread and trip like m3p_adam_step, at most 4096 blocks, at least one per piece
    if (want > ADAM_MAXBLK) want = ADAM_MAXBLK;
    if (want < a.n) want = a.n;
    int b = 0;
    for (int r = 0; r < a.n; ++r) {
      a.blk0[r] = b;
      long long share = (long long)((double)a.n4[r] / (double)total4 * (double)want);
      if (share < 1) share = 1;
      b += (int)share;
    }
    a.blk0[a.n] = b;
    if (skip)
      hipLaunchKernelGGL(adam_ranges_kernel<true>, dim3(b), dim3(256), 0, (hipStream_t)stream, a, skip);
    else
      hipLaunchKernelGGL(adam_ranges_kernel<false>, dim3(b), dim3(256), 0, (hipStream_t)stream, a, skip);
    M3P_CHECK_LAUNCH();
  }
  return M3P_OK;
}

int m3p_adam_step(float* p, float* g, float* m, float* v, void* w16, long long n, float lr, float beta1, float beta2,
                  float eps, float weight_decay, float step_size, const double* gnorm_sq, float max_norm,
                  float grad_scale, int zero_grad, void* stream) {
  if (n <= 0 || (n % 4) != 0) return M3P_EINVAL;
  if (((uintptr_t)p & 15) || ((uintptr_t)g & 15) || ((uintptr_t)m & 15) || ((uintptr_t)v & 15) || ((uintptr_t)w16 & 7))
    return M3P_EINVAL;
  AdamArgs a = {p, g, m, v, (bf16*)w16, (size_t)n / 4, lr, beta1, beta2, eps, weight_decay, step_size, gnorm_sq,
                max_norm, grad_scale == 0.f ? 1.f : grad_scale, zero_grad};
  const int blocks = (int)((a.n4 + 255) / 256 < 4096 ? (a.n4 + 255) / 256 : 4096);
  hipLaunchKernelGGL(adam_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

int m3p_transpose_bf16(const void* src, void* dst, int rows, int cols, int ld_src, int ld_dst, void* stream) {
  if (rows <= 0 || cols <= 0 || ld_src < cols || ld_dst < rows) return M3P_EINVAL;
  hipLaunchKernelGGL(transpose_bf16_kernel, dim3((cols + 63) / 64, (rows + 63) / 64), dim3(256), 0, (hipStream_t)stream,
                     (const bf16*)src, (bf16*)dst, rows, cols, ld_src, ld_dst);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// LAMB (include/m3p_hip.h: "LAMB on the flat arenas"): Adam's moments, then a per-tensor trust ratio ||p|| / ||r|| on the
// update r.  Three launches however many tensors are active:
//   update  reads p, g, m, v; writes m, v and r INTO THE GRADIENT'S PLACE (the gradient is dead after this pass), and one
//           (sum p^2, sum r^2) pair per workgroup;
//   norms   adds each tensor's workgroup pairs in a fixed order to one fp64 pair per tensor;
//   apply   reads p, r and the tensor's pair; writes p, the bf16 working copy and - where the piece says so - zeros over r.
// The pieces ([start, start + count) of the arenas, each inside ONE tensor) live in a table in device memory that the caller
// caches (m3p_lamb_table_build fills its host image): the ~200 tensors of a model do not fit a by-value table like
// AdamRanges.  Workgroups are dealt to the pieces in proportion to their sizes as in m3p_adam_step_ranges; a workgroup finds
// its piece by bisection over the pieces' first blocks.  No floating-point atomics anywhere on the way to the norms: the
// factor multiplies every weight of a tensor, and the same state must give the same bits.
// ---------------------------------------------------------------------------------------------------------------------
namespace {

struct LambPiece {            // 32 bytes, the layout m3p_lamb_table_build writes
  long long start4;           // first quad of the piece
  long long n4;               // quads
  int tensor;                 // index of the piece's tensor in the norms table
  int zero_grad;              // apply leaves zeros (1) or r (0) in the gradient's place
  int cls;                    // index into the per-launch class scalars
  int blk0;                   // first workgroup of the piece
};
static_assert(sizeof(LambPiece) == M3P_LAMB_PIECE_BYTES, "LambPiece is the table entry the header documents");

// scalars that differ between tensors of one launch, by value: the bias corrections follow a tensor's own step count
// (heads that sat out steps lag behind), weight decay and the trust ratio are off for excluded tensors
struct LambClasses {
  float rbc1[M3P_LAMB_MAX_CLASSES];     // 1 / (1 - beta1^s)
  float rbc2[M3P_LAMB_MAX_CLASSES];     // 1 / (1 - beta2^s)
  float wd[M3P_LAMB_MAX_CLASSES];
  int adapt[M3P_LAMB_MAX_CLASSES];
};

__device__ __forceinline__ int lamb_find_piece(const LambPiece* __restrict__ pieces, int n_pieces, int blk) {
  int lo = 0, hi = n_pieces - 1;        // the last piece whose first block is <= blk
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (pieces[mid].blk0 <= blk) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct LambUpdateArgs {
  float* p; float* g; float* m; float* v;
  const LambPiece* pieces;
  int n_pieces, n_blocks;
  float beta1, beta2, eps;
  const double* gnorm_sq;
  float max_norm, grad_scale;
  double* partials;           // [n_blocks][2]
};

constexpr int LAMB_Q = 2;            // 16-byte quads per thread and trip, as ADAM_Q
constexpr int LAMB_MAXBLK = 4096;

// GUARD (all three launches): the non-finite guard's forms, as adam_ranges_kernel<true>.  On a skipped step update and norms
// return before their first load - partials and norms keep whatever they held, nothing reads them - and apply is the one
// launch that stores the zeros.
template <bool GUARD>
__global__ __launch_bounds__(256) void lamb_update_kernel(LambUpdateArgs a, LambClasses c, const int* __restrict__ skip) {
  __shared__ double red[4][2];
  if (GUARD && *skip != 0) return;
  const int k = lamb_find_piece(a.pieces, a.n_pieces, (int)blockIdx.x);
  const LambPiece pc = a.pieces[k];
  const int blk_end = k + 1 < a.n_pieces ? a.pieces[k + 1].blk0 : a.n_blocks;
  float coef = a.grad_scale;
  if (a.gnorm_sq && a.max_norm > 0.f) {      // exactly adam_ranges_kernel's clip factor
    const float norm = (float)sqrt(*a.gnorm_sq) * a.grad_scale;
    const float cc = a.max_norm / (norm + 1e-6f);
    coef *= (cc < 1.f) ? cc : 1.f;
  }
  const float ob1 = 1.f - a.beta1, ob2 = 1.f - a.beta2;
  const float rbc1 = c.rbc1[pc.cls], rbc2 = c.rbc2[pc.cls], wd = c.wd[pc.cls];
  const size_t base = (size_t)pc.start4, n4 = (size_t)pc.n4;
  float* const P = a.p + 4 * base; float* const G = a.g + 4 * base; float* const M = a.m + 4 * base; float* const V = a.v + 4 * base;
  const size_t stride = (size_t)(blk_end - pc.blk0) * blockDim.x;
  constexpr int Q = LAMB_Q;
  float spp = 0.f, srr = 0.f;          // one rounding of the running sums per quad (tests: the accumulation bound counts them)
  for (size_t i0 = (size_t)((int)blockIdx.x - pc.blk0) * blockDim.x + threadIdx.x; i0 < n4; i0 += Q * stride) {
    f32x4 p[Q], g[Q], m[Q], v[Q];
#pragma unroll
    for (int u = 0; u < Q; ++u) {
      const size_t i = i0 + u * stride;
      if (u == 0 || i < n4) {
        p[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(P + 4 * i));
        g[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(G + 4 * i));
        m[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(M + 4 * i));
        v[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(V + 4 * i));
      }
    }
#pragma unroll
    for (int u = 0; u < Q; ++u) {
      const size_t i = i0 + u * stride;
      if (u == 0 || i < n4) {
        const f32x4 gc = g[u] * coef;
        const f32x4 mn = m[u] * a.beta1 + gc * ob1;
        const f32x4 vn = v[u] * a.beta2 + gc * gc * ob2;
        f32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = (mn[j] * rbc1) / (sqrtf(vn[j] * rbc2) + a.eps) + wd * p[u][j];
        __builtin_nontemporal_store(mn, reinterpret_cast<f32x4*>(M + 4 * i));
        __builtin_nontemporal_store(vn, reinterpret_cast<f32x4*>(V + 4 * i));
        __builtin_nontemporal_store(r, reinterpret_cast<f32x4*>(G + 4 * i));
        spp += (p[u][0] * p[u][0] + p[u][1] * p[u][1]) + (p[u][2] * p[u][2] + p[u][3] * p[u][3]);
        srr += (r[0] * r[0] + r[1] * r[1]) + (r[2] * r[2] + r[3] * r[3]);
      }
    }
  }
  spp = wave_sum(spp);
  srr = wave_sum(srr);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = (double)spp; red[threadIdx.x >> 6][1] = (double)srr; }
  __syncthreads();
  if (threadIdx.x == 0) {              // every workgroup writes its pair: the workspace needs no zeroing
    a.partials[2 * (size_t)blockIdx.x] = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
    a.partials[2 * (size_t)blockIdx.x + 1] = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
  }
}

// one wave per tensor: lane l adds the pairs of workgroups first + l, first + l + 64, ... in that order, then the lanes
// are folded by the butterfly - the same order every time
template <bool GUARD>
__global__ __launch_bounds__(64) void lamb_norms_kernel(const double* __restrict__ partials, const int* __restrict__ tensor_blk0,
                                                        double* __restrict__ norms, const int* __restrict__ skip) {
  if (GUARD && *skip != 0) return;
  const int t = blockIdx.x;
  const int b0 = tensor_blk0[t], b1 = tensor_blk0[t + 1];
  double pp = 0.0, rr = 0.0;
  for (int b = b0 + (int)threadIdx.x; b < b1; b += 64) {
    pp += partials[2 * (size_t)b];
    rr += partials[2 * (size_t)b + 1];
  }
  pp = wave_sum_f64(pp);
  rr = wave_sum_f64(rr);
  if (threadIdx.x == 0) { norms[2 * (size_t)t] = pp; norms[2 * (size_t)t + 1] = rr; }
}

struct LambApplyArgs {
  float* p; float* r; bf16* w16;
  const LambPiece* pieces;
  int n_pieces, n_blocks;
  const double* norms;        // [n_tensors][2]: sum p^2, sum r^2 (over all ranks' shards)
  float lr;
};

template <bool GUARD>
__global__ __launch_bounds__(256) void lamb_apply_kernel(LambApplyArgs a, LambClasses c, const int* __restrict__ skip) {
  const bool skipped = GUARD && *skip != 0;
  const int k = lamb_find_piece(a.pieces, a.n_pieces, (int)blockIdx.x);
  const LambPiece pc = a.pieces[k];
  const int blk_end = k + 1 < a.n_pieces ? a.pieces[k + 1].blk0 : a.n_blocks;
  if (skipped) {              // (the piece table is the only memory a skipped workgroup reads)
    if (pc.zero_grad == 0) return;
    float* const R = a.r + 4 * (size_t)pc.start4;
    const size_t n4 = (size_t)pc.n4, stride = (size_t)(blk_end - pc.blk0) * blockDim.x;
    for (size_t i = (size_t)((int)blockIdx.x - pc.blk0) * blockDim.x + threadIdx.x; i < n4; i += stride)
      __builtin_nontemporal_store(f32x4{0.f, 0.f, 0.f, 0.f}, reinterpret_cast<f32x4*>(R + 4 * i));
    return;
  }
  const double pp = a.norms[2 * (size_t)pc.tensor], rr = a.norms[2 * (size_t)pc.tensor + 1];
  const float phi = (c.adapt[pc.cls] && pp > 0.0 && rr > 0.0) ? (float)sqrt(pp / rr) : 1.f;
  const float s = a.lr * phi;
  const bool zero = pc.zero_grad != 0;
  const size_t base = (size_t)pc.start4, n4 = (size_t)pc.n4;
  float* const P = a.p + 4 * base; float* const R = a.r + 4 * base;
  bf16* const W = a.w16 ? a.w16 + 4 * base : nullptr;
  const size_t stride = (size_t)(blk_end - pc.blk0) * blockDim.x;
  constexpr int Q = LAMB_Q;
  for (size_t i0 = (size_t)((int)blockIdx.x - pc.blk0) * blockDim.x + threadIdx.x; i0 < n4; i0 += Q * stride) {
    f32x4 p[Q], r[Q];
#pragma unroll
    for (int u = 0; u < Q; ++u) {
      const size_t i = i0 + u * stride;
      if (u == 0 || i < n4) {
        p[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(P + 4 * i));
        r[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(R + 4 * i));
      }
    }
#pragma unroll
    for (int u = 0; u < Q; ++u) {
      const size_t i = i0 + u * stride;
      if (u == 0 || i < n4) {
        const f32x4 pn = p[u] - r[u] * s;
        __builtin_nontemporal_store(pn, reinterpret_cast<f32x4*>(P + 4 * i));
        if (W) Vec4<bf16>::store(W + 4 * i, pn);       // (re-read by the very next forward: default policy)
        if (zero) __builtin_nontemporal_store(f32x4{0.f, 0.f, 0.f, 0.f}, reinterpret_cast<f32x4*>(R + 4 * i));
      }
    }
  }
}

int lamb_classes(LambClasses* c, const float* rbc1, const float* rbc2, const float* wd, const int* adapt, int n_classes) {
  if (!adapt || n_classes <= 0 || n_classes > M3P_LAMB_MAX_CLASSES) return M3P_EINVAL;
  for (int i = 0; i < M3P_LAMB_MAX_CLASSES; ++i) {
    const bool in = i < n_classes;
    c->rbc1[i] = in && rbc1 ? rbc1[i] : 1.f;
    c->rbc2[i] = in && rbc2 ? rbc2[i] : 1.f;
    c->wd[i] = in && wd ? wd[i] : 0.f;
    c->adapt[i] = in ? adapt[i] : 0;
  }
  return M3P_OK;
}

}  // namespace

extern "C" {

int m3p_lamb_table_build(const long long* starts, const long long* counts, const int* tensor_ids, const int* zero_grad,
                         const int* class_ids, int n_pieces, int n_tensors, int n_classes, long long arena_elems, int max_blocks,
                         void* pieces_out, int* tensor_blk0_out, int* n_blocks_out) {
  if (!starts || !counts || !tensor_ids || !zero_grad || !class_ids || !pieces_out || !tensor_blk0_out || !n_blocks_out) return M3P_EINVAL;
  if (n_pieces <= 0 || n_tensors <= 0 || n_classes <= 0 || n_classes > M3P_LAMB_MAX_CLASSES || arena_elems <= 0) return M3P_EINVAL;
  if (max_blocks <= 0) max_blocks = LAMB_MAXBLK;
  long long total4 = 0, prev_end = 0;
  for (int k = 0; k < n_pieces; ++k) {
    // pieces in arena order, disjoint (two workgroups never write one element), inside the arena, on quad borders; the
    // pieces of a tensor adjacent in the table (the norms launch adds ONE run of workgroups per tensor)
    if (counts[k] <= 0 || (counts[k] % 4) != 0 || starts[k] < prev_end || (starts[k] % 4) != 0) return M3P_EINVAL;
    if (counts[k] > arena_elems - starts[k]) return M3P_EINVAL;
    if (tensor_ids[k] < 0 || tensor_ids[k] >= n_tensors || (k > 0 && tensor_ids[k] < tensor_ids[k - 1])) return M3P_EINVAL;
    if (class_ids[k] < 0 || class_ids[k] >= n_classes) return M3P_EINVAL;
    prev_end = starts[k] + counts[k];
    total4 += counts[k] / 4;
  }
  long long want = (total4 + 255) / 256;       // one quad per thread and trip, at most max_blocks, at least one per piece
  if (want > max_blocks) want = max_blocks;
  if (want < n_pieces) want = n_pieces;
  LambPiece* out = static_cast<LambPiece*>(pieces_out);
  long long b = 0;
  for (int t = 0; t <= n_tensors; ++t) tensor_blk0_out[t] = -1;
  for (int k = 0; k < n_pieces; ++k) {
    long long share = (long long)((double)(counts[k] / 4) / (double)total4 * (double)want);
    const long long most = (counts[k] / 4 + 255) / 256;      // no workgroup without a quad
    if (share > most) share = most;
    if (share < 1) share = 1;
    out[k] = LambPiece{starts[k] / 4, counts[k] / 4, tensor_ids[k], zero_grad[k] != 0, class_ids[k], (int)b};
    if (tensor_blk0_out[tensor_ids[k]] < 0) tensor_blk0_out[tensor_ids[k]] = (int)b;
    b += share;
    if (b > 0x3fffffffLL) return M3P_EINVAL;
  }
  tensor_blk0_out[n_tensors] = (int)b;
  for (int t = n_tensors - 1; t >= 0; --t)                   // a tensor without a piece (all of it another rank's): an empty run
    if (tensor_blk0_out[t] < 0) tensor_blk0_out[t] = tensor_blk0_out[t + 1];
  *n_blocks_out = (int)b;
  return M3P_OK;
}

int m3p_lamb_update(float* p, float* g, float* m, float* v, const void* pieces, int n_pieces, int n_blocks, const float* rbc1,
                    const float* rbc2, const float* wd, const int* adapt, int n_classes, float beta1, float beta2, float eps,
                    const double* gnorm_sq, float max_norm, float grad_scale, double* partials, void* stream) {
  return m3p_lamb_update_guarded(p, g, m, v, pieces, n_pieces, n_blocks, rbc1, rbc2, wd, adapt, n_classes, beta1, beta2, eps, gnorm_sq,
                                 max_norm, grad_scale, partials, nullptr, stream);
}

int m3p_lamb_update_guarded(float* p, float* g, float* m, float* v, const void* pieces, int n_pieces, int n_blocks, const float* rbc1,
                            const float* rbc2, const float* wd, const int* adapt, int n_classes, float beta1, float beta2, float eps,
                            const double* gnorm_sq, float max_norm, float grad_scale, double* partials, const int* skip,
                            void* stream) {
  if ((uintptr_t)skip & 3) return M3P_EINVAL;
  if (!p || !g || !m || !v || !pieces || !partials || !rbc1 || !rbc2 || !wd || n_pieces <= 0 || n_blocks < n_pieces) return M3P_EINVAL;
  if (((uintptr_t)p & 15) || ((uintptr_t)g & 15) || ((uintptr_t)m & 15) || ((uintptr_t)v & 15) || ((uintptr_t)pieces & 7) ||
      ((uintptr_t)partials & 7))
    return M3P_EINVAL;
  LambClasses c;
  if (lamb_classes(&c, rbc1, rbc2, wd, adapt, n_classes) != M3P_OK) return M3P_EINVAL;
  LambUpdateArgs a = {p, g, m, v, static_cast<const LambPiece*>(pieces), n_pieces, n_blocks, beta1, beta2, eps, gnorm_sq, max_norm,
                      grad_scale == 0.f ? 1.f : grad_scale, partials};
  if (skip)
    hipLaunchKernelGGL(lamb_update_kernel<true>, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, a, c, skip);
  else
    hipLaunchKernelGGL(lamb_update_kernel<false>, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, a, c, skip);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

int m3p_lamb_norms(const double* partials, const int* tensor_blk0, int n_tensors, double* norms, void* stream) {
  return m3p_lamb_norms_guarded(partials, tensor_blk0, n_tensors, norms, nullptr, stream);
}

int m3p_lamb_norms_guarded(const double* partials, const int* tensor_blk0, int n_tensors, double* norms, const int* skip,
                           void* stream) {
  if ((uintptr_t)skip & 3) return M3P_EINVAL;
  if (!partials || !tensor_blk0 || !norms || n_tensors <= 0) return M3P_EINVAL;
  if (((uintptr_t)partials & 7) || ((uintptr_t)tensor_blk0 & 3) || ((uintptr_t)norms & 7)) return M3P_EINVAL;
  if (skip)
    hipLaunchKernelGGL(lamb_norms_kernel<true>, dim3(n_tensors), dim3(64), 0, (hipStream_t)stream, partials, tensor_blk0, norms, skip);
  else
    hipLaunchKernelGGL(lamb_norms_kernel<false>, dim3(n_tensors), dim3(64), 0, (hipStream_t)stream, partials, tensor_blk0, norms, skip);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

int m3p_lamb_apply(float* p, float* r, void* w16, const void* pieces, int n_pieces, int n_blocks, const double* norms,
                   const int* adapt, int n_classes, float lr, void* stream) {
  return m3p_lamb_apply_guarded(p, r, w16, pieces, n_pieces, n_blocks, norms, adapt, n_classes, lr, nullptr, stream);
}

int m3p_lamb_apply_guarded(float* p, float* r, void* w16, const void* pieces, int n_pieces, int n_blocks, const double* norms,
                           const int* adapt, int n_classes, float lr, const int* skip, void* stream) {
  if ((uintptr_t)skip & 3) return M3P_EINVAL;
  if (!p || !r || !pieces || !norms || n_pieces <= 0 || n_blocks < n_pieces) return M3P_EINVAL;
  if (((uintptr_t)p & 15) || ((uintptr_t)r & 15) || ((uintptr_t)w16 & 7) || ((uintptr_t)pieces & 7) || ((uintptr_t)norms & 7)) return M3P_EINVAL;
  LambClasses c;
  if (lamb_classes(&c, nullptr, nullptr, nullptr, adapt, n_classes) != M3P_OK) return M3P_EINVAL;
  LambApplyArgs a = {p, r, (bf16*)w16, static_cast<const LambPiece*>(pieces), n_pieces, n_blocks, norms, lr};
  if (skip)
    hipLaunchKernelGGL(lamb_apply_kernel<true>, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, a, c, skip);
  else
    hipLaunchKernelGGL(lamb_apply_kernel<false>, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, a, c, skip);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// Exponential moving average of the master weights (include/m3p_hip.h, m3p_ema_update / m3p_ema_swap): two streaming
// kernels over pieces of the flat arenas, laid out like adam_ranges_kernel - pieces by value, workgroups dealt in proportion
// to the pieces' sizes, 16-byte quads, non-temporal accesses, EMA_Q quads per thread and trip.  No atomics, no LDS.
// ---------------------------------------------------------------------------------------------------------------------
namespace {

constexpr int EMA_MAX_RANGES = 32;
constexpr int EMA_Q = 2;             // 16-byte quads per thread and trip, as ADAM_Q
constexpr int EMA_MAXBLK = 4096;     // blocks per launch at most
struct EmaRanges {
  unsigned long long start4[EMA_MAX_RANGES];   // first quad of the piece
  unsigned long long n4[EMA_MAX_RANGES];
  int blk0[EMA_MAX_RANGES + 1];
  int n;
};

// ema = fma(w, p - ema, ema).  Two roundings per element: the difference, then ONE fused multiply-add - written as such, so
// that the rule is the same arithmetic whatever contraction setting the file is built with (the Makefile's -ffp-contract=fast
// fuses a separate product and sum anyway, pragmas notwithstanding).  tests/test_ema_cpu.py holds it as ema_twin(contract=True).
// GUARD: as adam_ranges_kernel<true> - a workgroup that reads a non-zero *skip returns before it loads anything.
template <bool GUARD>
__global__ __launch_bounds__(256) void ema_update_kernel(const float* __restrict__ p, float* __restrict__ ema, EmaRanges a, float w,
                                                         const int* __restrict__ skip) {
  if (GUARD && *skip != 0) return;
  int r = 0;
  while (r + 1 < a.n && (int)blockIdx.x >= a.blk0[r + 1]) ++r;
  const size_t base = (size_t)a.start4[r], n4 = (size_t)a.n4[r];
  const float* const P = p + 4 * base;
  float* const E = ema + 4 * base;
  const size_t stride = (size_t)(a.blk0[r + 1] - a.blk0[r]) * blockDim.x;
  constexpr int Q = EMA_Q;
  for (size_t i0 = (size_t)((int)blockIdx.x - a.blk0[r]) * blockDim.x + threadIdx.x; i0 < n4; i0 += Q * stride) {
    f32x4 x[Q], e[Q];
#pragma unroll
    for (int u = 0; u < Q; ++u) {
      const size_t i = i0 + u * stride;
      if (u == 0 || i < n4) {
        x[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(P + 4 * i));
        e[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(E + 4 * i));
      }
    }
#pragma unroll
    for (int u = 0; u < Q; ++u) {
      const size_t i = i0 + u * stride;
      if (u == 0 || i < n4) {
        const f32x4 d = x[u] - e[u];
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = __builtin_fmaf(w, d[j], e[u][j]);
        __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(E + 4 * i));
      }
    }
  }
}

// p <-> ema element by element, and w16 = bf16(new p) through the Adam kernel's conversion: one pass, two streams read, three
// written.  The values are moved, never computed with: a second swap restores all three buffers to the bit.
__global__ __launch_bounds__(256) void ema_swap_kernel(float* __restrict__ p, float* __restrict__ ema, bf16* __restrict__ w16, EmaRanges a) {
  int r = 0;
  while (r + 1 < a.n && (int)blockIdx.x >= a.blk0[r + 1]) ++r;
  const size_t base = (size_t)a.start4[r], n4 = (size_t)a.n4[r];
  float* const P = p + 4 * base;
  float* const E = ema + 4 * base;
  bf16* const W = w16 ? w16 + 4 * base : nullptr;
  const size_t stride = (size_t)(a.blk0[r + 1] - a.blk0[r]) * blockDim.x;
  constexpr int Q = EMA_Q;
  for (size_t i0 = (size_t)((int)blockIdx.x - a.blk0[r]) * blockDim.x + threadIdx.x; i0 < n4; i0 += Q * stride) {
    f32x4 x[Q], e[Q];
#pragma unroll
    for (int u = 0; u < Q; ++u) {
      const size_t i = i0 + u * stride;
      if (u == 0 || i < n4) {
        x[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(P + 4 * i));
        e[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(E + 4 * i));
      }
    }
#pragma unroll
    for (int u = 0; u < Q; ++u) {
      const size_t i = i0 + u * stride;
      if (u == 0 || i < n4) {
        __builtin_nontemporal_store(e[u], reinterpret_cast<f32x4*>(P + 4 * i));
        __builtin_nontemporal_store(x[u], reinterpret_cast<f32x4*>(E + 4 * i));
        if (W) Vec4<bf16>::store(W + 4 * i, e[u]);       // (re-read by the very next forward: default policy)
      }
    }
  }
}

// the pieces [starts[r], starts[r] + counts[r]) validated as a whole: nothing is launched for a list with a bad piece
bool ema_pieces_ok(const long long* starts, const long long* counts, int n_ranges) {
  if (!starts || !counts || n_ranges <= 0) return false;
  for (int r = 0; r < n_ranges; ++r)
    if (counts[r] < 0 || (counts[r] % 4) != 0 || starts[r] < 0 || (starts[r] % 4) != 0) return false;
  return true;
}

// the next launch's share of the list from *done on: up to EMA_MAX_RANGES non-empty pieces, blocks dealt in proportion to
// their sizes (one quad per thread and trip wanted, at most EMA_MAXBLK, at least one block per piece, none without a quad).
// -> blocks of the launch, 0 when the rest of the list is empty
int ema_deal(const long long* starts, const long long* counts, int n_ranges, int* done, EmaRanges* a) {
  a->n = 0;
  long long total4 = 0;
  for (; *done < n_ranges && a->n < EMA_MAX_RANGES; ++*done) {
    if (counts[*done] == 0) continue;
    a->start4[a->n] = (unsigned long long)starts[*done] / 4;
    a->n4[a->n] = (unsigned long long)counts[*done] / 4;
    total4 += counts[*done] / 4;
    ++a->n;
  }
  if (a->n == 0) return 0;
  long long want = (total4 + 255) / 256;
  if (want > EMA_MAXBLK) want = EMA_MAXBLK;
  if (want < a->n) want = a->n;
  int b = 0;
  for (int r = 0; r < a->n; ++r) {
    a->blk0[r] = b;
    long long share = (long long)((double)a->n4[r] / (double)total4 * (double)want);
    const long long most = ((long long)a->n4[r] + 255) / 256;
    if (share > most) share = most;
    if (share < 1) share = 1;
    b += (int)share;
  }
  a->blk0[a->n] = b;
  return b;
}

}  // namespace

extern "C" {

int m3p_ema_update(const float* p, float* ema, const long long* starts, const long long* counts, int n_ranges, float w,
                   const int* skip, void* stream) {
  if (!p || !ema || ((uintptr_t)p & 15) || ((uintptr_t)ema & 15) || ((uintptr_t)skip & 3)) return M3P_EINVAL;
  if (!ema_pieces_ok(starts, counts, n_ranges)) return M3P_EINVAL;
  int done = 0;
  while (done < n_ranges) {
    EmaRanges a;
    const int b = ema_deal(starts, counts, n_ranges, &done, &a);
    if (b == 0) continue;
    if (skip)
      hipLaunchKernelGGL(ema_update_kernel<true>, dim3(b), dim3(256), 0, (hipStream_t)stream, p, ema, a, w, skip);
    else
      hipLaunchKernelGGL(ema_update_kernel<false>, dim3(b), dim3(256), 0, (hipStream_t)stream, p, ema, a, w, skip);
    M3P_CHECK_LAUNCH();
  }
  return M3P_OK;
}

int m3p_ema_swap(float* p, float* ema, void* w16, const long long* starts, const long long* counts, int n_ranges, void* stream) {
  if (!p || !ema || ((uintptr_t)p & 15) || ((uintptr_t)ema & 15) || ((uintptr_t)w16 & 7)) return M3P_EINVAL;
  if (!ema_pieces_ok(starts, counts, n_ranges)) return M3P_EINVAL;
  int done = 0;
  while (done < n_ranges) {
    EmaRanges a;
    const int b = ema_deal(starts, counts, n_ranges, &done, &a);
    if (b == 0) continue;
    hipLaunchKernelGGL(ema_swap_kernel, dim3(b), dim3(256), 0, (hipStream_t)stream, p, ema, (bf16*)w16, a);
    M3P_CHECK_LAUNCH();
  }
  return M3P_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// Non-finite guard (include/m3p_hip.h, m3p_step_guard): the decision and its bookkeeping, one thread, plain stores.
// ---------------------------------------------------------------------------------------------------------------------
namespace {

struct GuardArgs {
  const double* sums[M3P_GUARD_MAX_ARENAS];
  int n;
  float grad_scale;
  int slot;                   // attempt & (M3P_GUARD_RING - 1)
  int* skip; int* ring; double* norm_ring; long long* counters;
};

__global__ __launch_bounds__(64) void step_guard_kernel(GuardArgs a) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double total = 0.0;
  int bad = 0;
  for (int i = 0; i < a.n; ++i) {
    const double s = *a.sums[i];
    // NaN or +-inf: every exponent bit set (a test on the bits: no compiler flag can reason it away)
    if (((unsigned long long)__double_as_longlong(s) & 0x7ff0000000000000ULL) == 0x7ff0000000000000ULL) bad = 1;
    total += s;
  }
  *a.skip = bad;
  a.ring[a.slot] = bad;
  a.norm_ring[a.slot] = sqrt(total) * (double)a.grad_scale;
  a.counters[0] += 1;
  a.counters[1] += bad;
  a.counters[2] = bad ? a.counters[2] + 1 : 0;
}

}  // namespace

extern "C" int m3p_step_guard(const double* const* gnorm_sq, int n_arenas, float grad_scale, long long attempt, int* skip, int* ring,
                              double* norm_ring, long long* counters, void* stream) {
  if (!gnorm_sq || !skip || !ring || !norm_ring || !counters || n_arenas <= 0 || attempt < 0) return M3P_EINVAL;
  if (n_arenas > M3P_GUARD_MAX_ARENAS) return M3P_ENOTIMPL;
  if (((uintptr_t)skip & 3) || ((uintptr_t)ring & 3) || ((uintptr_t)norm_ring & 7) || ((uintptr_t)counters & 7)) return M3P_EINVAL;
  GuardArgs a;
  for (int i = 0; i < M3P_GUARD_MAX_ARENAS; ++i) {
    a.sums[i] = i < n_arenas ? gnorm_sq[i] : nullptr;
    if (i < n_arenas && (!gnorm_sq[i] || ((uintptr_t)gnorm_sq[i] & 7))) return M3P_EINVAL;
  }
  a.n = n_arenas;
  a.grad_scale = grad_scale == 0.f ? 1.f : grad_scale;
  a.slot = (int)(attempt & (M3P_GUARD_RING - 1));
  a.skip = skip; a.ring = ring; a.norm_ring = norm_ring; a.counters = counters;
  hipLaunchKernelGGL(step_guard_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}
