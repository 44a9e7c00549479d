// Label smoothing of the tied vocabulary head without a pass over the logits (include/m3p_hip.h: m3p_vocab_mean, m3p_ls_*;
// DESIGN.md section 4).  With z = h E^T + b, e_bar = mean_v E[v, :], b_bar = mean_v b[v] and c = eps / n:
//   loss_eps = loss + c sum_r (z[r, y_r] - h_r . e_bar - b_bar)
//   dh_r    += c (E[y_r] - e_bar)        dE[v, :] += c (sum_{r: y_r = v} h_r - (1 / V) sum_r h_r)        db[v] += c (count_v - n / V)
// Everything here works on [n, d] and [V, d] operands: the mean row of E (once per optimizer step), the rows' dot products
// with it, the data gradient's closing pass with the extra operand, and one streaming add of a constant row over dE.
#include "common.hpp"

namespace {

// ---- ordered column sums of a bf16 [n, d] matrix: out[c] = scale * sum_r x[r, c], the same bits on every run.
// The matrix is read as a flat run of 16-byte chunks.  A period = lcm(d, 8) elements = 8 / gcd(d, 8) rows holds a whole
// number of chunks, so the thread that takes chunk t of every period it visits always holds the same eight columns in its
// eight accumulators.  Stage 1: thread (group g, chunk t) adds the periods g, g + G, g + 2 G, ... in that order (at any moment
// the grid reads one contiguous span) and leaves part[g][8 t + j]; stage 2: column c adds part[g][c + k d] over the rows k of a
// period and the groups g in a fixed order - sixteen slices of groups, each in sequence, then a pairwise fold.  No atomics.
// A vector riding along (the output bias, for its mean) is summed the same way: up to 64 blocks behind stage 1's leave one
// partial sum each, one block behind stage 2's folds them.
constexpr int LS_STAGE1_THREADS = 131072;     // 2 waves per SIMD of 256 CUs, four 16-byte loads in flight each
constexpr int LS_PERIODS_PER_GROUP = 32;      // a second group only once the first has this many periods to add
constexpr int LS_VEC_BLOCKS = 64;             // most partial sums of the vector
constexpr int LS_COLS = 16, LS_SLICES = 16;   // stage 2: a block's columns x slices of the groups

struct ColPlan {
  int rows_per;        // rows in a period
  int chunks;          // 16-byte chunks in a period
  long long periods;   // ceil(n / rows_per)
  int groups;          // G: partial sums per (period row, column)
};

static int gcd8(int d) { return (d % 8 == 0) ? 8 : (d % 4 == 0) ? 4 : (d % 2 == 0) ? 2 : 1; }

static ColPlan col_plan(int n, int d) {
  ColPlan p;
  const int g = gcd8(d);
  p.rows_per = 8 / g;
  p.chunks = d / g;
  p.periods = ((long long)n + p.rows_per - 1) / p.rows_per;
  long long groups = (p.periods + LS_PERIODS_PER_GROUP - 1) / LS_PERIODS_PER_GROUP;
  const long long cap = LS_STAGE1_THREADS / p.chunks > 1 ? LS_STAGE1_THREADS / p.chunks : 1;
  p.groups = (int)(groups < cap ? groups : cap);
  return p;
}
static size_t col_plan_bytes(const ColPlan& p) { return ((size_t)p.groups * p.chunks * 8 + LS_VEC_BLOCKS) * sizeof(float); }
static int vec_blocks(int n) { return (n + 1023) / 1024 < LS_VEC_BLOCKS ? (n + 1023) / 1024 : LS_VEC_BLOCKS; }

// the block's 256 values folded pairwise in a fixed order; the sum is in sh[0] (all threads call)
__device__ __forceinline__ void block_fold(float* sh) {
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void ls_colsum_partial_kernel(const bf16* __restrict__ x, long long total, int chunks, long long periods,
                                                                int groups, float* __restrict__ part, int main_blocks,
                                                                const float* __restrict__ vec, int n_vec, float* __restrict__ vec_part) {
  if ((int)blockIdx.x >= main_blocks) {
    // the vector's blocks: a contiguous slice each, thread i adds its elements i, i + 256, ...
    __shared__ float sh[256];
    const int nb = gridDim.x - main_blocks, j = blockIdx.x - main_blocks;
    const int per = (n_vec + nb - 1) / nb;
    const int v0 = j * per, v1 = min(n_vec, v0 + per);
    float s = 0.f;
    for (int v = v0 + threadIdx.x; v < v1; v += 256) s += vec[v];
    sh[threadIdx.x] = s;
    block_fold(sh);
    if (threadIdx.x == 0) vec_part[j] = sh[0];
    return;
  }
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  if (id >= (long long)chunks * groups) return;
  const int t = (int)(id % chunks), g = (int)(id / chunks);
  const long long lp = (long long)chunks * 8;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  long long p = g;
  constexpr int U = 4;
  // (every period but the last is whole: its chunks lie inside the matrix)
  for (; p + (long long)(U - 1) * groups < periods - 1; p += (long long)U * groups) {
    bf16x8 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
      v[u] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(x + (p + (long long)u * groups) * lp + 8 * t));
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += (float)v[u][j];
  }
  for (; p < periods; p += groups) {
    const long long i0 = p * lp + 8 * t;
    if (i0 + 8 <= total) {
      const bf16x8 v = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(x + i0));
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += (float)v[j];
    } else {
      // the matrix ends inside this chunk (or before it): element by element, nothing behind row n - 1 is read
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (i0 + j < total) acc[j] += (float)x[i0 + j];
    }
  }
  float* out = part + ((long long)g * chunks + t) * 8;
  *reinterpret_cast<f32x4*>(out) = f32x4{acc[0], acc[1], acc[2], acc[3]};
  *reinterpret_cast<f32x4*>(out + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
}

// blocks 0 .. ceil(d / 16) - 1: 16 columns x 16 slices of the groups (a thread adds its slice's partials in sequence: a few
// dozen dependent loads, where four slices of 1365 groups took longer than stage 1 itself).  One more block when the vector's
// partial sums are given: out[d] = scale * their sum.
__global__ __launch_bounds__(256) void ls_colsum_final_kernel(const float* __restrict__ part, int d, int rows_per, int chunks, int groups,
                                                              float scale, const float* __restrict__ vec_part, int n_vec_part,
                                                              float* __restrict__ out) {
  __shared__ float sh[256];
  const int col_blocks = (d + LS_COLS - 1) / LS_COLS;
  if ((int)blockIdx.x >= col_blocks) {
    sh[threadIdx.x] = (int)threadIdx.x < n_vec_part ? vec_part[threadIdx.x] : 0.f;
    block_fold(sh);
    if (threadIdx.x == 0) out[d] = sh[0] * scale;
    return;
  }
  const int lane = threadIdx.x % LS_COLS, q = threadIdx.x / LS_COLS;
  const int c = blockIdx.x * LS_COLS + lane;
  const long long lp = (long long)chunks * 8;
  const int per = (groups + LS_SLICES - 1) / LS_SLICES;
  const int g0 = q * per, g1 = min(groups, g0 + per);
  float s = 0.f;
  if (c < d) {
#pragma unroll 4
    for (int g = g0; g < g1; ++g)
      for (int k = 0; k < rows_per; ++k) s += part[(long long)g * lp + c + (long long)k * d];
  }
  sh[threadIdx.x] = s;
  __syncthreads();
  // slices q and q + w of a column sit w * LS_COLS apart
  for (int w = LS_SLICES / 2; w > 0; w >>= 1) {
    if (q < w) sh[threadIdx.x] += sh[threadIdx.x + w * LS_COLS];
    __syncthreads();
  }
  if (q == 0 && c < d) out[c] = sh[lane] * scale;
}

static int colsum_ordered(const void* x, int n, int d, float scale, const float* vec, float* out, void* ws, size_t ws_bytes,
                          hipStream_t st) {
  if (n <= 0 || d <= 0 || !x || !out || !ws || ((uintptr_t)x & 15) || ((uintptr_t)ws & 15)) return M3P_EINVAL;
  const ColPlan p = col_plan(n, d);
  if (ws_bytes < col_plan_bytes(p)) return M3P_EINVAL;
  const long long threads = (long long)p.chunks * p.groups;
  const int main_blocks = (int)((threads + 255) / 256), nvb = vec ? vec_blocks(n) : 0;
  float* vec_part = (float*)ws + (size_t)p.groups * p.chunks * 8;
  hipLaunchKernelGGL(ls_colsum_partial_kernel, dim3(main_blocks + nvb), dim3(256), 0, st, (const bf16*)x, (long long)n * d, p.chunks,
                     p.periods, p.groups, (float*)ws, main_blocks, vec, n, vec_part);
  hipLaunchKernelGGL(ls_colsum_final_kernel, dim3((d + LS_COLS - 1) / LS_COLS + (vec ? 1 : 0)), dim3(256), 0, st, (const float*)ws, d,
                     p.rows_per, p.chunks, p.groups, scale, vec_part, nvb, out);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

// ---- aux_r = t_r - h_r . e_bar - b_bar, one wave per row (the form of ce_shift_target_kernel); mean = e_bar [d], b_bar
__global__ __launch_bounds__(256) void ls_row_aux_kernel(const bf16* __restrict__ h, const float* __restrict__ mean, const float* __restrict__ row_t,
                                                         float* __restrict__ aux, int n_rows, int d) {
  const int lane = threadIdx.x & 63;
  const int row = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if (row >= n_rows) return;
  const bf16* hr = h + (size_t)row * d;
  float acc = 0.f;
  for (int c = lane * 4; c < d; c += 256) {
    const f32x4 a = Vec4<bf16>::load(hr + c), b = Vec4<float>::load(mean + c);
    acc += (a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3]);
  }
  acc = wave_sum(acc);
  if (lane == 0) aux[row] = (row_t[row] - acc) - mean[d];
}

// ---- out[0] = scale * sum_r v[r] in a fixed order: one block, thread i adds elements i, i + 256, ..., then the pairwise fold
// (the rows' terms into the loss: a few thousand numbers)
__global__ __launch_bounds__(256) void ls_sum_ordered_kernel(const float* __restrict__ v, int n, float scale, float* __restrict__ out) {
  __shared__ float sh[256];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += v[i];
  sh[threadIdx.x] = s;
  block_fold(sh);
  if (threadIdx.x == 0) out[0] = sh[0] * scale;
}

// ---- dh[n, :] = bf16(g (s_n dh32[n, :] + (q_n + c) E[y_n, :] - c e_bar)): ce_shift_dh_kernel with the smoothing operand; the
// plain routes (dh32 = dlogits x E, already normalised) pass no row_s / row_q: s = 1, q = 0.  One rounding per element.
__global__ __launch_bounds__(256) void ce_shift_dh_smooth_kernel(const float* __restrict__ dh32, const bf16* __restrict__ emb,
                                                                 const int64_t* __restrict__ target, const float* __restrict__ row_s,
                                                                 const float* __restrict__ row_q, const float* __restrict__ g,
                                                                 const float* __restrict__ mean, float cs, bf16* __restrict__ dh, int n, int d) {
  const int nchunk = d >> 2;
  const size_t total = (size_t)n * nchunk;
  const float gv = *g;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / nchunk), c = (int)(i - (size_t)r * nchunk);
    const f32x4 a = Vec4<float>::load(dh32 + 4 * i);
    const f32x4 b = Vec4<bf16>::load(emb + (size_t)target[r] * d + 4 * c);
    const f32x4 m = Vec4<float>::load(mean + 4 * c);
    const float s = row_s ? row_s[r] : 1.f, q = (row_q ? row_q[r] : 0.f) + cs;
    Vec4<bf16>::store(dh + 4 * i, ((a * s + b * q) - m * cs) * gv);
  }
}

// ---- dst[v, :] += g u[:] and dbias[v] += g db for v < V: one read-modify-write stream over the fp32 [V, d] gradient in
// 16-byte chunks (d % 4 == 0: a chunk never straddles two rows), grid-stride.  Nothing at or behind row V is touched - in the
// arena those "rows" are the head of the bias gradient.
constexpr int LS_ADD_BLOCKS = 2048;

static int uniform_add_blocks(long long chunks) {
  const long long b = (chunks + 255) / 256;
  return (int)(b < LS_ADD_BLOCKS ? (b > 0 ? b : 1) : LS_ADD_BLOCKS);
}

__global__ __launch_bounds__(256) void ls_uniform_add_kernel(float* __restrict__ dst, float* __restrict__ dbias, const float* __restrict__ u,
                                                             const float* __restrict__ g, float db, int V, int d) {
  const long long total = (long long)V * (d >> 2);
  const long long stride = (long long)gridDim.x * blockDim.x;
  const float gv = *g;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int col = (int)((4 * i) % d);
    const f32x4 a = Vec4<float>::load(dst + 4 * i);
    Vec4<float>::store(dst + 4 * i, a + Vec4<float>::load(u + col) * gv);
  }
  const float add = gv * db;
  for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += stride) dbias[v] += add;
}

}  // namespace

extern "C" {

int m3p_vocab_mean_plan(int V, int d) {
  if (V <= 0 || d <= 0) return 0;
  return col_plan(V, d).groups;
}

size_t m3p_vocab_mean_workspace_bytes(int V, int d) {
  if (V <= 0 || d <= 0) return 0;
  return col_plan_bytes(col_plan(V, d));
}

int m3p_vocab_mean(const void* emb, const float* bias, int V, int d, float* mean, void* workspace, size_t workspace_bytes, void* stream) {
  if (!bias) return M3P_EINVAL;
  return colsum_ordered(emb, V, d, 1.0f / (float)V, bias, mean, workspace, workspace_bytes, (hipStream_t)stream);
}

int m3p_ls_colsum_rows(const void* h, int n_rows, int d, float scale, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  return colsum_ordered(h, n_rows, d, scale, nullptr, out, workspace, workspace_bytes, (hipStream_t)stream);
}

int m3p_ls_row_aux(const void* h, const float* mean, const float* row_t, float* aux, int n_rows, int d, void* stream) {
  if (n_rows <= 0 || d <= 0 || (d % 4) != 0 || !h || !mean || !row_t || !aux || ((uintptr_t)h & 7) || ((uintptr_t)mean & 15))
    return M3P_EINVAL;
  hipLaunchKernelGGL(ls_row_aux_kernel, dim3((n_rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const bf16*)h, mean, row_t, aux,
                     n_rows, d);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

int m3p_ls_sum_rows(const float* v, int n, float scale, float* out, void* stream) {
  if (n <= 0 || !v || !out) return M3P_EINVAL;
  hipLaunchKernelGGL(ls_sum_ordered_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, v, n, scale, out);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

int m3p_ce_shift_dh_smooth(const float* dh32, const void* emb, const int64_t* target, const float* row_s, const float* row_q,
                           const float* g, const float* mean, float c, void* dh, int n_rows, int d, void* stream) {
  if (n_rows <= 0 || d <= 0 || (d % 4) != 0 || !dh32 || !emb || !target || !g || !mean || !dh || ((uintptr_t)dh32 & 15) ||
      ((uintptr_t)emb & 7) || ((uintptr_t)mean & 15) || ((uintptr_t)dh & 7))
    return M3P_EINVAL;
  const size_t total = (size_t)n_rows * (d / 4);
  const int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
  hipLaunchKernelGGL(ce_shift_dh_smooth_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dh32, (const bf16*)emb, target, row_s,
                     row_q, g, mean, c, (bf16*)dh, n_rows, d);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

int m3p_ls_uniform_add_plan(int V, int d) {
  if (V <= 0 || d <= 0 || (d % 4) != 0) return 0;
  return uniform_add_blocks((long long)V * (d / 4));
}

int m3p_ls_uniform_add(float* dst, float* dbias, const float* u, const float* g, float db, int V, int d, void* stream) {
  if (V <= 0 || d <= 0 || (d % 4) != 0 || !dst || !dbias || !u || !g || ((uintptr_t)dst & 15) || ((uintptr_t)u & 15)) return M3P_EINVAL;
  hipLaunchKernelGGL(ls_uniform_add_kernel, dim3(uniform_add_blocks((long long)V * (d / 4))), dim3(256), 0, (hipStream_t)stream, dst,
                     dbias, u, g, db, V, d);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

}  // extern "C"
