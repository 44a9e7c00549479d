// MFMA GEMMs for the M3P hot path on gfx950 (MI355X).
//
//   gemm_nt   : C[M,N] = epi(A[M,K] x W[N,K]^T)    both operands K-contiguous (nn.Linear)
//   gemm_wgrad: dW[N,K] += dY[M,N]^T x X[M,K]      both operands contraction-strided,
//               fragments come out of LDS through ds_read_b64_tr_b16 (hardware transpose)
//
// Kernels, in the order the launchers prefer them:
//   gemm_nt_w4_kernel / gemm_wgrad_w4_kernel   four waves, 256x256 tile, 128x128 per wave with the
//       256 accumulators pinned in AGPRs, 64-deep K-tiles in two 64-KB LDS stages; full-tile shapes.
//       They live in gemm_nt_w4.hpp / gemm_wgrad_w4.hpp, included below; the two halves of their K-tiles (the MFMA /
//       memory-instruction schedule) are generated: tools/gen/gen_w4.py -> gen/*.inc.
//   gemm_nt_ring_kernel / gemm_wgrad_ring_kernel   eight waves, 256x128 tile, 64x64 per wave,
//       three-stage 48-KB ring; ragged shapes, the dGELU epilogue, the vocabulary matrices.
//   gemm_nt_streamk_kernel   contraction-split NT with fp32 atomics (vocabulary data gradient).
//   gemm_nt_kernel / gemm_wgrad_kernel   128x128, two stages: small-M fallbacks.
// Common: v_mfma_f32_16x16x32_bf16 with swapped operands (a lane owns 4 consecutive output
// columns), HBM -> LDS by global_load_lds_dwordx4 (no VGPR round trip).  The LDS image of a
// K-contiguous tile is [rows][64] bf16 (128 B rows); because an LDS-DMA writes lane-linear,
// the bank swizzle (16-B chunk ^= row & 7) is applied to the per-lane SOURCE address and
// again on the ds_read_b128 (cdna guide rule 21), which makes the fragment reads
// conflict-free.  Persistent kernels deal tiles so that each XCD (private L2) walks a
// strip-blocked run of tiles that share their operand panels.
#include <mutex>
#include <type_traits>
#include "common.hpp"
#include "../../include/m3p_hip.h"
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

// debug: 1 = the dispatch tables (nt_plan / wgrad_plan), 2 = force the four-wave 256x256 NT kernel where it applies, 6 = force
// the eight-wave 256x256 NT kernel; any other value means 1
static int g_variant = 1;
extern "C" void m3p_debug_set_variant(int v) { g_variant = (v == 2 || v == 6) ? v : 1; }     // (declared in the header's developer section)

namespace {

constexpr int BK = 64;            // contraction elements per LDS stage
constexpr int ROWB = BK * 2;      // bytes per LDS row of a K-contiguous tile (128)

// Inline-asm LDS reads, counted waits and the barrier of the hand-scheduled K loops.  The reads are ones the compiler does
// not see as loads: their destinations hold data only after OUR wait.  A wait or barrier is fenced with sched_barrier on
// both sides so that nothing is scheduled across it.  (tests/test_kernel_isa.py checks what the compiler makes of them.)
#define M3P_DSR(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:" #off : "=v"(dst) : "v"(addr))
#define M3P_TR(dst, addr, off) asm volatile("ds_read_b64_tr_b16 %0, %1 offset:" #off : "=v"(dst) : "v"(addr))
#define M3P_WAIT_LGKM(N) do { __builtin_amdgcn_sched_barrier(0); asm volatile("s_waitcnt lgkmcnt(" #N ")" ::: "memory"); __builtin_amdgcn_sched_barrier(0); } while (0)
#define M3P_WAIT_VM(N) do { __builtin_amdgcn_sched_barrier(0); asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); __builtin_amdgcn_sched_barrier(0); } while (0)
#define M3P_BAR() do { __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); __builtin_amdgcn_sched_barrier(0); } while (0)

// Place of this workgroup in a persistent grid of nwg workgroups (a multiple of 8, one per CU): consecutive slots sit on one
// XCD (workgroup b runs on XCD b & 7), so that what neighbouring slots share stays in that XCD's private L2.
__device__ __forceinline__ int xcd_slot(int nwg) {
  const int per_xcd = nwg >> 3;
  return (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
}
// The tile walk of the persistent NT kernels: workgroup `slot` takes tiles slot, slot + nwg, ...  Tile id -> (tm, tn) is
// n-fastest - neighbours share the A row-panel - or, from `from` n-tiles on, where a full row of n-tiles no longer fits the L2
// beside the A panels, in strips of about `width` n-tiles walked m-major: the run of tiles an XCD holds in one round is then
// a block of a few A row-panels x `width` W panels.  (from / width are each kernel's own measurement: see there.)
// strip_width gives the strips' actual width, split_tile the place of tile t.
__device__ __forceinline__ int strip_width(int tiles_n, int from, int width) {
  const int n_strips = (tiles_n >= from) ? (tiles_n + width - 1) / width : 1;
  return (tiles_n + n_strips - 1) / n_strips;
}
__device__ __forceinline__ void split_tile(int t, int tiles_m, int tiles_n, int strip_w, int& tm, int& tn) {
  const int strip = t / (tiles_m * strip_w);
  const int rem = t - strip * tiles_m * strip_w;
  const int bn = min(strip_w, tiles_n - strip * strip_w);
  tm = rem / bn;
  tn = strip * strip_w + (rem - tm * bn);
}

// ---------------------------------------------------------------------------------
// NT kernel
// ---------------------------------------------------------------------------------
template <int EPI>
__device__ __forceinline__ void epilogue_store(const M3PEpilogue& ep, bf16* __restrict__ C, int ldc,
                                               int M, int N, int m, int n, f32x4 acc, f32x4& csum) {
  if (m >= M || n >= N) return;
  const bool full = (n + 3 < N);
  float v[4] = {acc[0], acc[1], acc[2], acc[3]};
  const float alpha = (ep.alpha == 0.f) ? 1.f : ep.alpha;
  if (EPI == M3P_EPI_NONE || EPI == M3P_EPI_BIAS || EPI == M3P_EPI_RES) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] *= alpha;
  }
  if (EPI == M3P_EPI_BIAS || EPI == M3P_EPI_BIAS_GELU || EPI == M3P_EPI_BIAS_DROP_RES) {
    if (ep.bias) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (n + r < N) v[r] += ep.bias[n + r];
    }
  }
  if (EPI == M3P_EPI_BIAS) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (n + r < ep.scale_cols) v[r] *= ep.scale;
  }
  if (EPI == M3P_EPI_BIAS_GELU) {
    bf16* U = reinterpret_cast<bf16*>(ep.out2) + (size_t)m * ep.ld_out2 + n;
    bf16 ur[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { ur[r] = (bf16)v[r]; v[r] = gelu_erf_f((float)ur[r]); }
    if (full) *reinterpret_cast<bf16x4*>(U) = bf16x4{ur[0], ur[1], ur[2], ur[3]};
    else
      for (int r = 0; r < 4; ++r) if (n + r < N) U[r] = ur[r];
  }
  if (EPI == M3P_EPI_BIAS_DROP_RES) {
    if (ep.thresh24) {
      const uint32_t mr = ep.rng_rows ? (uint32_t)ep.rng_rows[m] : (uint32_t)m;      // (row of the full tensor: M3PEpilogue)
      const uint32_t base = mr * (uint32_t)N + (uint32_t)n;
      bool kp[4];
      m3p_keep_run<4>(base, ep.seed, ep.thresh24, kp);        // (any N: the run may start on an odd element)
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = kp[r] ? v[r] * ep.inv_keep : 0.f;
    }
  }
  if (EPI == M3P_EPI_BIAS_DROP_RES || EPI == M3P_EPI_RES || EPI == M3P_EPI_DGELU || EPI == M3P_EPI_MUL) {
    const bf16* X = reinterpret_cast<const bf16*>(ep.aux) + (size_t)m * ep.ld_aux + n;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    if (full) { bf16x4 t = *reinterpret_cast<const bf16x4*>(X); a[0] = (float)t[0]; a[1] = (float)t[1]; a[2] = (float)t[2]; a[3] = (float)t[3]; }
    else
      for (int r = 0; r < 4; ++r) if (n + r < N) a[r] = (float)X[r];
    if (EPI == M3P_EPI_DGELU) {
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] *= gelu_erf_grad_f(a[r]);
    } else if (EPI == M3P_EPI_MUL) {
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] *= a[r];
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] += a[r];
    }
  }
  bf16 o[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) o[r] = (bf16)v[r];
  bf16* Cp = C + (size_t)m * ldc + n;
  if (full) *reinterpret_cast<bf16x4*>(Cp) = bf16x4{o[0], o[1], o[2], o[3]};
  else
    for (int r = 0; r < 4; ++r) if (n + r < N) Cp[r] = o[r];
  if (EPI == M3P_EPI_DGELU || EPI == M3P_EPI_MUL) {
#pragma unroll
    for (int r = 0; r < 4; ++r) csum[r] += (n + r < N) ? (float)o[r] : 0.f;
  }
}

template <int BM, int BN, int EPI>
__global__ __launch_bounds__(64 * (BM / 64) * (BN / 64))
void gemm_nt_kernel(const bf16* __restrict__ A, int lda, const bf16* __restrict__ W, int ldw,
                    bf16* __restrict__ C, int ldc, int M, int N, int K, M3PEpilogue ep,
                    int tiles_m, int tiles_n) {
  constexpr int WAVES_M = BM / 64, WAVES_N = BN / 64, NWAVES = WAVES_M * WAVES_N;
  constexpr int A_BYTES = BM * ROWB, B_BYTES = BN * ROWB, STAGE = A_BYTES + B_BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int id = xcd_remap(blockIdx.x, tiles_m * tiles_n);
  const int tm = id / tiles_n, tn = id - tm * tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;

  // ---- staging: one wave instruction = 8 rows x 128 B, lane -> (row l>>3, LDS chunk l&7),
  //      global chunk = LDS chunk ^ (row & 7)
  const int sr = lane >> 3, sc = (lane & 7) ^ sr;
  const bf16* a_src[BM / 8 / NWAVES];
  const bf16* w_src[BN / 8 / NWAVES];
#pragma unroll
  for (int i = 0; i < BM / 8 / NWAVES; ++i) {
    int row = (wid + i * NWAVES) * 8 + sr;
    int gm = min(m0 + row, M - 1);
    a_src[i] = A + (size_t)gm * lda + sc * 8;
  }
#pragma unroll
  for (int i = 0; i < BN / 8 / NWAVES; ++i) {
    int row = (wid + i * NWAVES) * 8 + sr;
    int gn = min(n0 + row, N - 1);
    w_src[i] = W + (size_t)gn * ldw + sc * 8;
  }
  auto stage = [&](int kt, int s) {
    char* sa = smem + s * STAGE;
    char* sb = sa + A_BYTES;
    const int k0 = kt * BK;
#pragma unroll
    for (int i = 0; i < BM / 8 / NWAVES; ++i)
      __builtin_amdgcn_global_load_lds(GLB_PTR(a_src[i] + k0), LDS_PTR(sa + (wid + i * NWAVES) * 1024), 16, 0, 0);
#pragma unroll
    for (int i = 0; i < BN / 8 / NWAVES; ++i)
      __builtin_amdgcn_global_load_lds(GLB_PTR(w_src[i] + k0), LDS_PTR(sb + (wid + i * NWAVES) * 1024), 16, 0, 0);
  };

  // ---- fragment addressing
  const int wm = wid / WAVES_N, wn = wid - wm * WAVES_N;
  const int fr = lane & 15, fg = lane >> 4;
  int a_off[2], b_off[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const int ch = ((fg + 4 * ks) ^ (fr & 7)) * 16;
    a_off[ks] = (wm * 64 + fr) * ROWB + ch;
    b_off[ks] = A_BYTES + (wn * 64 + fr) * ROWB + ch;
  }

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = K / BK;
  stage(0, 0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) stage(kt + 1, cur ^ 1);
    const char* sbase = smem + cur * STAGE;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 af[4], wf[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = *reinterpret_cast<const bf16x8*>(sbase + a_off[ks] + i * 16 * ROWB);
#pragma unroll
      for (int j = 0; j < 4; ++j) wf[j] = *reinterpret_cast<const bf16x8*>(sbase + b_off[ks] + j * 16 * ROWB);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          // first operand = W rows (n), second = A rows (m): D[n][m] -> lane holds
          // m = l&15 and four consecutive n = 4*(l>>4)+r  (8-byte bf16 stores along N)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], af[i], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }

  // ---- epilogue
  f32x4 csum[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) csum[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + wm * 64 + i * 16 + fr;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + wn * 64 + j * 16 + fg * 4;
      epilogue_store<EPI>(ep, C, ldc, M, N, m, n, acc[i][j], csum[j]);
    }
  }
  if ((EPI == M3P_EPI_DGELU || EPI == M3P_EPI_MUL) && ep.colsum) {
    // reduce over the 16 lanes that share fg (different rows), then one atomic per column
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float s = csum[j][r];
        s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64);
        s += __shfl_xor(s, 4, 64); s += __shfl_xor(s, 8, 64);
        const int n = n0 + wn * 64 + j * 16 + fg * 4 + r;
        if (fr == 0 && n < N) unsafeAtomicAdd(ep.colsum + n, s);
      }
    }
  }
}

// ---------------------------------------------------------------------------------
// NT kernel, ring version (the production path for large M): 256x128 output tile, 8 waves
// (4 x 2, 64x64 each), three 48-KB LDS stages (144 of the CU's 160 KB).  HBM -> LDS loads run
// TWO K-tiles ahead of the MFMAs and are retired with a COUNTED s_waitcnt vmcnt(6) (one
// tile = 6 LDS-DMA instructions per wave stays in flight across the barrier), so the
// workgroup never drains its memory pipeline inside the K loop; one raw s_barrier per K-tile.
// MFMA operand fragments are double-buffered per 32-deep k-step: the ds_read_b128s of the
// next k-step are issued before the 16 MFMAs of the current one.
// ---------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------
// Epilogue of an interior wave tile through LDS: the MFMA result layout gives a lane 4
// consecutive columns of one row (8-byte pieces, 32-B row segments per store instruction);
// staging 32 rows x 64 columns in LDS turns that into 16 bytes per lane and whole 128-B lines
// per 8 lanes.  `rows` are two 16-row MFMA tile rows (x 4 column tiles) starting at global row mrow0.
// ---------------------------------------------------------------------------------
constexpr int EP_PITCH = 144;                 // bytes per staged row: 128 + 16 (16-B aligned, rotates banks)
constexpr int EP_HALF = 32 * EP_PITCH;        // 4608 B per wave half-tile
// byte offset of (row, byte column) inside a wave's staging rows.  SW: 128-byte pitch with the 16-byte chunk index XORed
// with row & 7 instead of the padded pitch - 32 rows are exactly 4 KB, so eight waves' staging fits the 32 KB a CU has left
// beside two 64-KB stages (the eight-wave kernel then never touches a stage in its epilogue)
template <bool SW>
__device__ __forceinline__ int ep_off(int row, int bcol) {
  return SW ? row * 128 + ((((bcol >> 4) ^ (row & 7)) << 4) | (bcol & 15)) : row * EP_PITCH + bcol;
}
// The 8-byte accesses in the accumulator layout (lane = row fr of 16, four columns) put rows r and r + 8 of a 16-row block on
// the same banks (the chunk swizzle only knows row & 7): a two-way conflict on every such instruction (r03 counters: LDS bank
// conflicts in 5-9 % of the eight-wave kernel's cycles, all of them in the epilogue).  In the swizzled layout the 8-byte half
// inside the 16-byte chunk is therefore flipped for rows with bit 3 set (ep_off8); the 16-byte row-layout side of the same
// staging rows swaps the halves in registers (flip_halves - its rows are it * 8 + lane / 8, so bit 3 is a compile-time fact).
template <bool SW>
__device__ __forceinline__ int ep_off8(int row, int bcol) {
  return ep_off<SW>(row, bcol) ^ (SW ? (row & 8) : 0);
}
template <class V4>
__device__ __forceinline__ V4 flip_halves(const V4& t, bool flip) {
  return flip ? V4{t[2], t[3], t[0], t[1]} : t;
}

// LDS accesses the compiler does not see (ALDS = true in the epilogue helpers below).  Why: a kernel whose K loop keeps
// buffer_load ... lds transfers in flight makes the compiler put s_waitcnt vmcnt(0) in front of EVERY LDS access it knows of
// (the transfer might alias it) - and vmcnt(0) also waits for the previous piece's global stores, a full memory round trip
// per staged piece.  The staging buffers never alias the stages; with these the waits are ours (lgkm_wait ties the wait to
// the values it is for, so that their uses cannot be scheduled in front of it).
typedef unsigned int u32x4_lds __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint32_t lds_addr(const void* p) { return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const char*)p; }
__device__ __forceinline__ void lds_w64(uint32_t a, const bf16x4& v) { asm volatile("ds_write_b64 %0, %1" :: "v"(a), "v"(v)); }
__device__ __forceinline__ void lds_w128(uint32_t a, const u32x4_lds& v) { asm volatile("ds_write_b128 %0, %1" :: "v"(a), "v"(v)); }
__device__ __forceinline__ void lds_r64(uint32_t a, bf16x4& v) { asm volatile("ds_read_b64 %0, %1" : "=v"(v) : "v"(a)); }
__device__ __forceinline__ void lds_r128(uint32_t a, u32x4_lds& v) { asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(a)); }

// gelu_erf'(u) of a bf16 u is a function of 16 bits: the dGELU epilogue looks it up instead of
// evaluating erf/exp (~20 exposed VALU instructions per element).  The table covers |u| in
// [2^-15, 8) (exponents -15..2 x 128 mantissas = 2304 fp32 entries, 9 KB of LDS), built from what
// gelu_erf_grad_f returns for that bf16 value; gelu'(-u) = 1 - gelu'(u).
constexpr int GELU_TAB_LO = 0x3800, GELU_TAB_HI = 0x4100, GELU_TAB_N = GELU_TAB_HI - GELU_TAB_LO;
// The table holds gelu'(|u|) - 1/2, an odd function of u: gelu'(u) = 1/2 + copysign(tab[|u|], u).  Seven VALU
// instructions and one LDS read per element (and, sub, med3, lshl_add, bfi, add, + the multiply); the first table
// entry serves every |u| < 2^-15 (error 2.4e-5, a tenth of a bf16 ulp of 1/2), the last every |u| >= 8 (gelu' = 1).
__device__ __forceinline__ void gelu_grad_table_fill(float* tab, int tid, int nthreads) {
  for (int i = tid; i < GELU_TAB_N; i += nthreads) {
    const uint16_t bits = (uint16_t)(GELU_TAB_LO + i);
    tab[i] = gelu_erf_grad_f((float)__builtin_bit_cast(bf16, bits)) - 0.5f;
  }
}
__device__ __forceinline__ float gelu_grad_lookup(const float* tab, bf16 u) {
  const uint32_t b = __builtin_bit_cast(uint16_t, u);
  const int idx = min(max((int)(b & 0x7FFFu) - GELU_TAB_LO, 0), GELU_TAB_N - 1);   // (compiles to v_med3_i32)
  const uint32_t t = __builtin_bit_cast(uint32_t, tab[idx]);
  return 0.5f + __builtin_bit_cast(float, (t & 0x7FFFFFFFu) | ((b << 16) & 0x80000000u));
}

// bias values of the four 16-column tiles starting at column nw for this lane (columns nw + 16 j + 4 (lane >> 4) ..+3)
template <int EPI>
__device__ __forceinline__ void load_bias4(const M3PEpilogue& ep, int nw, int lane, f32x4 (&biasv)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    biasv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if ((EPI == M3P_EPI_BIAS || EPI == M3P_EPI_BIAS_GELU || EPI == M3P_EPI_BIAS_DROP_RES) && ep.bias)
      biasv[j] = *reinterpret_cast<const f32x4*>(ep.bias + nw + j * 16 + (lane >> 4) * 4);
  }
}

// this lane's share of the 32 x 64 aux tile (residual / pre-activation) at (mrow0, nw)
template <int EPI>
__device__ __forceinline__ void load_aux(const M3PEpilogue& ep, int mrow0, int nw, int lane, bf16x4 (&auxv)[2][4]) {
  constexpr bool kAux = (EPI == M3P_EPI_BIAS_DROP_RES || EPI == M3P_EPI_RES || EPI == M3P_EPI_DGELU || EPI == M3P_EPI_MUL);
  if (!kAux) return;
  const bf16* X = reinterpret_cast<const bf16*>(ep.aux) + (size_t)(mrow0 + (lane & 15)) * ep.ld_aux + nw + (lane >> 4) * 4;
#pragma unroll
  for (int ii = 0; ii < 2; ++ii)
#pragma unroll
    for (int j = 0; j < 4; ++j) auxv[ii][j] = *reinterpret_cast<const bf16x4*>(X + (size_t)(ii * 16) * ep.ld_aux + j * 16);
}

// The same aux half-tile fetched as whole 128-byte row segments (16 B per lane, 8 lanes per row, 4 instructions
// instead of 8) and transposed into the accumulator layout through the wave-private staging rows `r1`; load_aux's
// direct form touches sixteen 32-byte row pieces per instruction.  Measured: dGELU 0.349 -> 0.340 ms, the
// residual epilogues unchanged (the aux tile costs ~60 us per 41984 x 3072 GEMM either way - see DESIGN.md).
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));   // (HIP's uint4 is a struct: arrays of it passed by reference end up in scratch)

// 16-byte output-row store (plain: the store policies sc1 / sc0 sc1 / sc1 nt were measured against it)
template <class P>
__device__ __forceinline__ void st16(P* p, const u32x4& v) {
  *reinterpret_cast<u32x4*>(p) = v;
}
template <bool NT>
__device__ __forceinline__ void st16p(void* p, const u32x4& v) {
  if (NT) __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p));
  else *reinterpret_cast<u32x4*>(p) = v;
}
template <int EPI>
__device__ __forceinline__ void load_aux_rows_issue(const M3PEpilogue& ep, int mrow0, int nw, int lane, u32x4 (&t)[4]) {
  constexpr bool kAux = (EPI == M3P_EPI_BIAS_DROP_RES || EPI == M3P_EPI_RES || EPI == M3P_EPI_DGELU || EPI == M3P_EPI_MUL);
  if (!kAux) return;
  const int srow = lane >> 3, sch = lane & 7;
  const bf16* X = reinterpret_cast<const bf16*>(ep.aux) + (size_t)(mrow0 + srow) * ep.ld_aux + nw + sch * 8;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    t[it] = *reinterpret_cast<const u32x4*>(X + (size_t)(it * 8) * ep.ld_aux);
  }
}
template <int EPI, bool SW = false, bool ALDS = false>
__device__ __forceinline__ void load_aux_rows_finish(int lane, char* r1, const u32x4 (&t)[4], bf16x4 (&auxv)[2][4]) {
  constexpr bool kAux = (EPI == M3P_EPI_BIAS_DROP_RES || EPI == M3P_EPI_RES || EPI == M3P_EPI_DGELU || EPI == M3P_EPI_MUL);
  if (!kAux) return;
  const int srow = lane >> 3, sch = lane & 7;
  const int fr = lane & 15, fg = lane >> 4;
  if (ALDS) {
    const uint32_t la = lds_addr(r1);
#pragma unroll
    for (int it = 0; it < 4; ++it) lds_w128(la + ep_off<SW>(it * 8 + srow, sch * 16), flip_halves(t[it], SW && (it & 1)));
#pragma unroll
    for (int ii = 0; ii < 2; ++ii)
#pragma unroll
      for (int j = 0; j < 4; ++j) lds_r64(la + ep_off8<SW>(ii * 16 + fr, (j * 16 + fg * 4) * 2), auxv[ii][j]);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(auxv[0][0]), "+v"(auxv[0][1]), "+v"(auxv[0][2]), "+v"(auxv[0][3]),
                                         "+v"(auxv[1][0]), "+v"(auxv[1][1]), "+v"(auxv[1][2]), "+v"(auxv[1][3]));
    return;
  }
#pragma unroll
  for (int it = 0; it < 4; ++it) *reinterpret_cast<u32x4*>(r1 + ep_off<SW>(it * 8 + srow, sch * 16)) = flip_halves(t[it], SW && (it & 1));
#pragma unroll
  for (int ii = 0; ii < 2; ++ii)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      auxv[ii][j] = *reinterpret_cast<const bf16x4*>(r1 + ep_off8<SW>(ii * 16 + fr, (j * 16 + fg * 4) * 2));
}
template <int EPI, bool SW = false>
__device__ __forceinline__ void load_aux_rows(const M3PEpilogue& ep, int mrow0, int nw, int lane, char* r1, bf16x4 (&auxv)[2][4]) {
  u32x4 t[4];
  load_aux_rows_issue<EPI>(ep, mrow0, nw, lane, t);
  load_aux_rows_finish<EPI, SW>(lane, r1, t, auxv);
}

// epilogue_half in two parts: the arithmetic on a 32 x 64 piece and its staging writes (accumulator layout -> r1) ...
// (internal epilogue number of the four-wave kernel's row-mapped BIAS_DROP_RES instantiation: see gemm_nt_w4_kernel)
constexpr int M3P_EPI_DROP_RES_ROWS = 10;
// NOROWS: M3PEpilogue::rng_rows is known to be NULL at compile time (no lookup, no branch)
template <int EPI, bool SW = false, bool ALDS = false, bool NOROWS = false>
__device__ __forceinline__ void epilogue_half_write(const M3PEpilogue& ep, int N, int mrow0, int nw, char* r1, const f32x4 (&rows)[2][4],
                                                    const f32x4 (&biasv)[4], const bf16x4 (&auxv)[2][4], int lane, f32x4 (&csum)[4],
                                                    bf16x4 (&ukeep)[2][4], const float* gtab = nullptr) {
  const int fr = lane & 15, fg = lane >> 4;
  constexpr bool kAux = (EPI == M3P_EPI_BIAS_DROP_RES || EPI == M3P_EPI_RES || EPI == M3P_EPI_DGELU || EPI == M3P_EPI_MUL);
  const float alpha = (ep.alpha == 0.f) ? 1.f : ep.alpha;
  // dropout: the two rows of this lane as the stream numbers them - the row itself, or with M3PEpilogue::rng_rows (a launch
  // over gathered rows) its number in the full tensor: one uniform branch in front of the piece.  Precondition of every
  // caller (as for their row-wise aux loads): the piece's 32 rows mrow0 .. mrow0 + 31 lie inside M - whole tiles in the
  // eight-wave kernel, the whole-tile branches of the four-wave, ring and fp8 kernels; ragged tiles go through epilogue_store,
  // which checks m < M before it reads the map
  uint32_t drow[2] = {(uint32_t)(mrow0 + fr), (uint32_t)(mrow0 + 16 + fr)};
  if (EPI == M3P_EPI_BIAS_DROP_RES && !NOROWS && ep.rng_rows != nullptr) {
    drow[0] = (uint32_t)ep.rng_rows[mrow0 + fr];
    drow[1] = (uint32_t)ep.rng_rows[mrow0 + 16 + fr];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = nw + j * 16 + fg * 4;
    f32x4 bias4 = biasv[j];        // (zeros when the epilogue has no bias; fetched by the caller ahead of time)
    // alpha, bias and the per-column scale fold into ONE fma per element: the constants are per
    // column, i.e. per (j, r), not per row (the epilogue runs with the MFMA pipe idle - every
    // instruction in it is exposed)
    f32x4 mulc = {alpha, alpha, alpha, alpha};
    if (EPI == M3P_EPI_BIAS) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (n + r < ep.scale_cols) { mulc[r] *= ep.scale; bias4[r] *= ep.scale; }
    }
#pragma unroll
    for (int ii = 0; ii < 2; ++ii) {
      const int rl = ii * 16 + fr;                  // row inside the staged half
      const int mrow = mrow0 + rl;                  // global row
      const int lo = ep_off8<SW>(rl, (j * 16 + fg * 4) * 2);
      f32x4 v = rows[ii][j];
      if (EPI == M3P_EPI_NONE || EPI == M3P_EPI_BIAS || EPI == M3P_EPI_RES) v = v * mulc + bias4;
      else if (EPI != M3P_EPI_DGELU && EPI != M3P_EPI_MUL) v += bias4;      // (those two have no bias: 32 exposed adds per half)
      if (EPI == M3P_EPI_BIAS_GELU) {
        ukeep[ii][j] = bf16x4{(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = gelu_erf_f((float)ukeep[ii][j][r]);
      }
      if (EPI == M3P_EPI_BIAS_DROP_RES && ep.thresh24) {
        const uint32_t base = drow[ii] * (uint32_t)N + (uint32_t)n;      // (whole tiles: N and n are multiples of 4)
        bool kp[4];
        m3p_keep_even<4>(base, ep.seed, ep.thresh24, kp);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = kp[r] ? v[r] * ep.inv_keep : 0.f;
      }
      if (kAux) {
        const bf16x4 t = auxv[ii][j];       // residual / pre-activation tile, fetched by the caller ahead of time
        const f32x4 a = f32x4{(float)t[0], (float)t[1], (float)t[2], (float)t[3]};
        if (EPI == M3P_EPI_DGELU) {
          if (gtab) {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] *= gelu_grad_lookup(gtab, t[r]);
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] *= gelu_erf_grad_f(a[r]);
          }
        } else if (EPI == M3P_EPI_MUL) {
          v *= a;
        } else {
          v += a;
        }
      }
      const bf16x4 ob = bf16x4{(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
      if (ALDS) lds_w64(lds_addr(r1) + lo, ob);
      else *reinterpret_cast<bf16x4*>(r1 + lo) = ob;
      if (EPI == M3P_EPI_DGELU || EPI == M3P_EPI_MUL) csum[j] += f32x4{(float)ob[0], (float)ob[1], (float)ob[2], (float)ob[3]};
    }
  }
}
// ... the staged piece read back as rows (16 bytes per lane, 8 lanes per 128-byte row segment) with asm accesses, issued
// only: the caller waits - lgkm_wait_rows - and flips the halves of rows 8-15, 24-31 then ...
template <bool SW>
__device__ __forceinline__ void epilogue_rows_read(const char* r1, int lane, u32x4 (&R)[4]) {
  const int srow = lane >> 3, sch = lane & 7;
  const uint32_t la = lds_addr(r1);
#pragma unroll
  for (int it = 0; it < 4; ++it) lds_r128(la + ep_off<SW>(it * 8 + srow, sch * 16), R[it]);
}
// the wait that belongs to epilogue_rows_read: `younger` (8 or 0) LDS instructions of this wave may stay in flight
template <bool SW>
__device__ __forceinline__ void lgkm_wait_rows(u32x4 (&R)[4], bool younger8) {
  if (younger8) asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(R[0]), "+v"(R[1]), "+v"(R[2]), "+v"(R[3]));
  else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(R[0]), "+v"(R[1]), "+v"(R[2]), "+v"(R[3]));
#pragma unroll
  for (int it = 0; it < 4; ++it) R[it] = flip_halves(R[it], SW && (it & 1));
}
// ... and stored.  (Apart so that a kernel with nobody else on its SIMD can keep a piece's LDS round trip in flight under
// the next piece's accumulator reads and arithmetic: gemm_nt_w4_kernel.)
__device__ __forceinline__ void epilogue_rows_store(bf16* __restrict__ C, int ldc, int mrow0, int nw, int lane, const u32x4 (&R)[4]) {
  const int srow = lane >> 3, sch = lane & 7;
  bf16* Cp = C + (size_t)mrow0 * ldc + nw + sch * 8;
#pragma unroll
  for (int it = 0; it < 4; ++it) st16(Cp + (size_t)(it * 8 + srow) * ldc, R[it]);
}
template <int EPI, bool SW = false>
__device__ __forceinline__ void epilogue_half(const M3PEpilogue& ep, bf16* __restrict__ C, int ldc, int N,
                                              int mrow0, int nw, char* r1, const f32x4 (&rows)[2][4],
                                              const f32x4 (&biasv)[4], const bf16x4 (&auxv)[2][4], int lane, f32x4 (&csum)[4],
                                              const float* gtab = nullptr) {
  const int fr = lane & 15, fg = lane >> 4;
  const int srow = lane >> 3, sch = lane & 7;
  bf16x4 ukeep[2][4];
  epilogue_half_write<EPI, SW>(ep, N, mrow0, nw, r1, rows, biasv, auxv, lane, csum, ukeep, gtab);
  bf16* Cp = C + (size_t)mrow0 * ldc + nw + sch * 8;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int row = it * 8 + srow;
    st16(Cp + (size_t)row * ldc, flip_halves(*reinterpret_cast<const u32x4*>(r1 + ep_off<SW>(row, sch * 16)), SW && (it & 1)));
  }
  if (EPI == M3P_EPI_BIAS_GELU) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int ii = 0; ii < 2; ++ii)
        *reinterpret_cast<bf16x4*>(r1 + ep_off8<SW>(ii * 16 + fr, (j * 16 + fg * 4) * 2)) = ukeep[ii][j];
    bf16* Up = reinterpret_cast<bf16*>(ep.out2) + (size_t)mrow0 * ep.ld_out2 + nw + sch * 8;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int row = it * 8 + srow;
      st16(Up + (size_t)row * ep.ld_out2, flip_halves(*reinterpret_cast<const u32x4*>(r1 + ep_off<SW>(row, sch * 16)), SW && (it & 1)));
    }
  }
}


// 16-row pieces of the multiply epilogues (dGELU / MUL: out = acc * f(aux), column sums) for the eight-wave kernel: the
// aux rows of piece h + 1 are requested while piece h is computed (8 registers per piece), staging is 2 KB per wave in
// the swizzled layout - eight waves' staging and the 9-KB derivative table fit the 32 KB beside the two stages.
__device__ __forceinline__ void aux16_issue(const M3PEpilogue& ep, int mrow0, int nw, int lane, u32x4 (&t)[2]) {
  const int srow = lane >> 3, sch = lane & 7;
  const bf16* X = reinterpret_cast<const bf16*>(ep.aux) + (size_t)(mrow0 + srow) * ep.ld_aux + nw + sch * 8;
  t[0] = *reinterpret_cast<const u32x4*>(X);
  t[1] = *reinterpret_cast<const u32x4*>(X + (size_t)8 * ep.ld_aux);
}
template <int EPI>
__device__ __forceinline__ void epilogue_piece16(const M3PEpilogue& ep, bf16* __restrict__ C, int ldc, int mrow0, int nw, char* r1,
                                                 const f32x4 (&rows)[4], const u32x4 (&t)[2], int lane, f32x4 (&csum)[4],
                                                 const float* gtab) {
  const int fr = lane & 15, fg = lane >> 4;
  const int srow = lane >> 3, sch = lane & 7;
  // aux rows -> accumulator layout through the staging rows
  *reinterpret_cast<u32x4*>(r1 + ep_off<true>(srow, sch * 16)) = t[0];
  *reinterpret_cast<u32x4*>(r1 + ep_off<true>(8 + srow, sch * 16)) = flip_halves(t[1], true);
  bf16x4 auxv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) auxv[j] = *reinterpret_cast<const bf16x4*>(r1 + ep_off8<true>(fr, (j * 16 + fg * 4) * 2));
  // the sixteen table reads of a piece are independent: all addresses first, all reads in flight together, one wait (left
  // inside the per-element expression the compiler chains address -> read -> wait -> multiply sixteen times: ~130 clocks each)
  float tv[4][4];
  if (EPI == M3P_EPI_DGELU && gtab) {
    int idx[4][4];
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const u32x2 raw = __builtin_bit_cast(u32x2, auxv[j]);      // four bf16 bit patterns in two dwords
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t b = (raw[r >> 1] >> (16 * (r & 1))) & 0x7FFFu;
        idx[j][r] = min(max((int)b - GELU_TAB_LO, 0), GELU_TAB_N - 1);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) tv[j][r] = gtab[idx[j][r]];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f32x4 v = rows[j];
    const bf16x4 a = auxv[j];
    if (EPI == M3P_EPI_DGELU) {
      if (gtab) {
        {
          typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
          const u32x2 raw = __builtin_bit_cast(u32x2, a);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const uint32_t sign = (raw[r >> 1] << (16 * (1 - (r & 1)))) & 0x80000000u;
            const uint32_t tb = __builtin_bit_cast(uint32_t, tv[j][r]);
            v[r] *= 0.5f + __builtin_bit_cast(float, (tb & 0x7FFFFFFFu) | sign);
          }
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] *= gelu_erf_grad_f((float)a[r]);
      }
    } else {
      v *= f32x4{(float)a[0], (float)a[1], (float)a[2], (float)a[3]};
    }
    const bf16x4 ob = bf16x4{(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
    *reinterpret_cast<bf16x4*>(r1 + ep_off8<true>(fr, (j * 16 + fg * 4) * 2)) = ob;
    csum[j] += f32x4{(float)ob[0], (float)ob[1], (float)ob[2], (float)ob[3]};
  }
  bf16* Cp = C + (size_t)mrow0 * ldc + nw + sch * 8;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int row = it * 8 + srow;
    st16(Cp + (size_t)row * ldc, flip_halves(*reinterpret_cast<const u32x4*>(r1 + ep_off<true>(row, sch * 16)), it & 1));
  }
}

// 16-row piece of the byte-derivative epilogue (M3P_EPI_MULQ): out = acc * decode(code), column sums.  `q` holds this
// lane's sixteen codes of the piece in accumulator order (dword j = columns 16 j + 4 fg .. + 3 of row fr: the fragment-order
// layout of common.hpp, fetched by the caller with one 16-byte load) - no aux trip through LDS, three VALU per element.

// Round 6: the 8-bit copy of a 16 x 64 output piece for the fp8 product that consumes this output (M3PEpilogue::out8): four
// values of a lane -> one dword (v_cvt_pk_fp8 / _bf8 on the scaled, saturated fp32 values), 16 x 64 bytes through the wave's
// staging rows (64-byte pitch, the 16-byte chunk index XORed with (row >> 1) & 3: two lanes per bank on the way in, the
// minimum for 64 four-byte writes) and out as ONE 16-byte store per lane (4 lanes per 64-byte row segment).  The staging rows
// are the ones the bf16 piece just left: LDS instructions of a wave execute in order, so the writes below cannot pass the
// row reads in front of them.  `amax` = this lane's running max |value| (folded into *amax8 once, at the end of the kernel).
template <bool BF8>
__device__ __forceinline__ uint32_t pack8(const f32x4& v, float scale, float& amax) {
  constexpr float kMax = BF8 ? 57344.f : 448.f;
  float f[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    amax = fmaxf(amax, fabsf(v[r]));
    f[r] = __builtin_amdgcn_fmed3f(v[r] * scale, -kMax, kMax);
  }
  int w = 0;
  if (BF8) { w = __builtin_amdgcn_cvt_pk_bf8_f32(f[0], f[1], w, false); w = __builtin_amdgcn_cvt_pk_bf8_f32(f[2], f[3], w, true); }
  else { w = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], w, false); w = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], w, true); }
  return (uint32_t)w;
}
__device__ __forceinline__ void lds_w32(uint32_t a, uint32_t v) { asm volatile("ds_write_b32 %0, %1" :: "v"(a), "v"(v)); }
__device__ __forceinline__ void piece8_write(char* r8, const uint32_t (&w8)[4], int lane) {
  const int fr = lane & 15, fg = lane >> 4;
  const uint32_t la = lds_addr(r8);
  asm volatile("" ::: "memory");      // (callers that stage the bf16 piece with plain C++ accesses: none of those may sink below here)
#pragma unroll
  for (int j = 0; j < 4; ++j) lds_w32(la + fr * 64 + ((j ^ ((fr >> 1) & 3)) << 4) + fg * 4, w8[j]);
}
__device__ __forceinline__ void piece8_store(uint8_t* __restrict__ o8, int ld8, int mrow0, int nw, char* r8, int lane) {
  const uint32_t la = lds_addr(r8);
  const int row = lane >> 2, c = lane & 3;
  u32x4_lds R;
  lds_r128(la + row * 64 + (c << 4), R);
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(R) :: "memory");      // (... and none of the next piece's may rise above here)
  st16p<true>(o8 + (size_t)(mrow0 + row) * ld8 + nw + ((c ^ ((row >> 1) & 3)) << 4), u32x4{R[0], R[1], R[2], R[3]});
}
__device__ __forceinline__ void piece8_flush(uint8_t* __restrict__ o8, int ld8, int mrow0, int nw, char* r1, const uint32_t (&w8)[4], int lane) {
  piece8_write(r1, w8, lane);
  piece8_store(o8, ld8, mrow0, nw, r1, lane);
}
template <int O8 = 0>      // 0: no 8-bit copy, 1: e4m3, 2: e5m2
__device__ __forceinline__ void epilogue_pieceq(bf16* __restrict__ C, int ldc, int mrow0, int nw, char* r1, const f32x4 (&rows)[4],
                                                const u32x4& q, int lane, f32x4 (&csum)[4], uint8_t* __restrict__ o8 = nullptr, int ld8 = 0,
                                                float scale8 = 1.f, float* amax = nullptr, char* r8 = nullptr) {
  const int fr = lane & 15, fg = lane >> 4;
  const int srow = lane >> 3, sch = lane & 7;
  uint32_t w8[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t w = q[j];
    f32x4 g = f32x4{(float)(w & 0xFFu), (float)((w >> 8) & 0xFFu), (float)((w >> 16) & 0xFFu), (float)(w >> 24)};   // v_cvt_f32_ubyte0..3
    g = g * GQ_STEP - GQ_OFF;
    const f32x4 v = rows[j] * g;
    const bf16x4 ob = bf16x4{(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
    if (O8) lds_w64(lds_addr(r1) + ep_off8<true>(fr, (j * 16 + fg * 4) * 2), ob);
    else *reinterpret_cast<bf16x4*>(r1 + ep_off8<true>(fr, (j * 16 + fg * 4) * 2)) = ob;
    // column sums (lin1's bias gradient) of the fp32 products: one add per element (round 6; summing the bf16-rounded values
    // cost an unpack per element on top and is no closer to the fp32 reference's sum)
    csum[j] += v;
    if (O8) w8[j] = (O8 == 2) ? pack8<true>(v, scale8, *amax) : pack8<false>(v, scale8, *amax);
  }
  if (O8) piece8_write(r8, w8, lane);
  bf16* Cp = C + (size_t)mrow0 * ldc + nw + sch * 8;
  if (O8) {
    // every staging access of this form is one the compiler does not see (no vmcnt(0) in front of each: with the 8-bit rows'
    // stores in flight as well, those waits cost ~50 us per launch); both pieces' row reads share one wait
    const uint32_t la = lds_addr(r1), l8 = lds_addr(r8);
    const int row8 = lane >> 2, c8 = lane & 3;
    u32x4_lds Ra, Rb, R8;
    lds_r128(la + ep_off<true>(srow, sch * 16), Ra);
    lds_r128(la + ep_off<true>(8 + srow, sch * 16), Rb);
    lds_r128(l8 + row8 * 64 + (c8 << 4), R8);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(Ra), "+v"(Rb), "+v"(R8));
    st16p<true>(Cp + (size_t)srow * ldc, u32x4{Ra[0], Ra[1], Ra[2], Ra[3]});
    st16p<true>(Cp + (size_t)(8 + srow) * ldc, u32x4{Rb[2], Rb[3], Rb[0], Rb[1]});
    st16p<true>(o8 + (size_t)(mrow0 + row8) * ld8 + nw + ((c8 ^ ((row8 >> 1) & 3)) << 4), u32x4{R8[0], R8[1], R8[2], R8[3]});
    return;
  }
  u32x4 R2[2];
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int row = it * 8 + srow;
    R2[it] = flip_halves(*reinterpret_cast<const u32x4*>(r1 + ep_off<true>(row, sch * 16)), it & 1);
  }
  // (the 8-bit piece has staging rows of its own, r8: its writes were issued with the bf16 piece's - below - and its row read
  //  shares the wait of theirs; the first version took a second, serialised trip through r1: 277 against 207 us per launch)
#pragma unroll
  for (int it = 0; it < 2; ++it) st16p<true>(Cp + (size_t)(it * 8 + srow) * ldc, R2[it]);
  if (O8) piece8_store(o8, ld8, mrow0, nw, r8, lane);
}

// 32-row piece of the vocabulary projection's epilogue (M3P_EPI_BIAS_LSE): logits = acc + bias as for M3P_EPI_BIAS, plus what
// the cross-entropy needs of them while they are still in registers - per (row, 64-column block of this wave) the block's
// maximum and sum of exp(logit - max) over the columns < V, written to stats[block][row] (consecutive rows of a block are
// consecutive: 16 lanes store 128 bytes).  A row's log-sum-exp is then a reduction over N / 64 pairs instead of a second
// pass over the 2.4 GB of logits.  The statistics are taken on the fp32 values (the stored logits are their bf16 rounding).
__device__ __forceinline__ void epilogue_half_lse(bf16* __restrict__ C, int ldc, float2* __restrict__ stats, int V, int mrow0, int nw,
                                                  char* r1, const f32x4 (&rows0)[4], const f32x4 (&rows1)[4],
                                                  const f32x4 (&biasv)[4], int lane, bool edge) {
  constexpr float kLog2e = 1.4426950408889634f;
  const int fr = lane & 15, fg = lane >> 4;
  const int srow = lane >> 3, sch = lane & 7;
#pragma unroll
  for (int ii = 0; ii < 2; ++ii) {
    f32x4 x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[j] = (ii ? rows1[j] : rows0[j]) + biasv[j];
      const bf16x4 xb = bf16x4{(bf16)x[j][0], (bf16)x[j][1], (bf16)x[j][2], (bf16)x[j][3]};
      *reinterpret_cast<bf16x4*>(r1 + ep_off8<true>(ii * 16 + fr, (j * 16 + fg * 4) * 2)) = xb;
      // the statistics are taken on the ROUNDED logits - the very values the cross-entropy's gradient pass and its target term
      // read back - so that softmax rows sum to one and the gradient rows to zero exactly as with a statistics pass over the
      // stored logits (one shift per element)
#pragma unroll
      for (int r = 0; r < 4; ++r) x[j][r] = (float)xb[r];
    }
    if (edge) {        // (wave-uniform: only the last column tile holds columns >= V)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (nw + j * 16 + fg * 4 + r >= V) x[j][r] = -INFINITY;
    }
    f32x4 m4 = x[0];
#pragma unroll
    for (int j = 1; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) m4[r] = fmaxf(m4[r], x[j][r]);
    float m = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    const float mb = (m == -INFINITY) ? 0.f : m * kLog2e;
    f32x4 s4 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 a = x[j] * kLog2e - mb;
#pragma unroll
      for (int r = 0; r < 4; ++r) s4[r] += __builtin_amdgcn_exp2f(a[r]);
    }
    float sm = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    sm += __shfl_xor(sm, 16, 64);
    sm += __shfl_xor(sm, 32, 64);
    if (fg == 0) stats[mrow0 + ii * 16 + fr] = float2{m, sm};
  }
  bf16* Cp = C + (size_t)mrow0 * ldc + nw + sch * 8;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int row = it * 8 + srow;
    st16p<true>(Cp + (size_t)row * ldc, flip_halves(*reinterpret_cast<const u32x4*>(r1 + ep_off<true>(row, sch * 16)), it & 1));
  }
}

// The shifted-exponential form of that epilogue (M3P_EPI_BIAS_LSE with M3PEpilogue::row_ref set; inside the library an
// instantiation of its own, like M3P_EPI_DROP_RES_ROWS).  The softmax normaliser is a per-row scalar: it factors out of both
// gradient products and of the bias gradient, so what the cross-entropy's backward needs of the logits is
//   e[n, v] = bf16(exp(x[n, v] - c_n))
// for ANY per-row shift c_n known before the launch - row_ref[n] = {c_n, y_n}, c_n = the target's own logit + CE_SHIFT
// (csrc/heads.hip) - and the 2.4-GB tensor is never rewritten.  e is an exact 0 at the target column y_n (its term is handled in
// fp32 by the row kernels: a bf16 p_y - 1 is all rounding error on a confident row) and at the pad columns >= V (the weight
// gradient's pad rows alias the bias gradient in the arena and rely on += 0).  stats[block][row] = the fp32 sum of the ROUNDED
// values of the block: what summing the stored tensor gives.  No maximum pass, one shuffle pair, one float per (block, row).
constexpr int M3P_EPI_BIAS_EXP = 11;
struct CeRowRef { float c; int32_t y; };
__device__ __forceinline__ void epilogue_half_exp(bf16* __restrict__ C, int ldc, float* __restrict__ stats, const CeRowRef* __restrict__ ref,
                                                  int V, int mrow0, int nw, char* r1, const f32x4 (&rows0)[4], const f32x4 (&rows1)[4],
                                                  const f32x4 (&biasv)[4], int lane, bool edge) {
  constexpr float kLog2e = 1.4426950408889634f;
  const int fr = lane & 15, fg = lane >> 4;
  const int srow = lane >> 3, sch = lane & 7;
  const float2 rf[2] = {*reinterpret_cast<const float2*>(ref + mrow0 + fr), *reinterpret_cast<const float2*>(ref + mrow0 + 16 + fr)};
#pragma unroll
  for (int ii = 0; ii < 2; ++ii) {
    const float cb = rf[ii].x * kLog2e;
    const int tc = __builtin_bit_cast(int, rf[ii].y) - nw - fg * 4;      // the target's place among this lane's columns j * 16 + r
    f32x4 x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 a = ((ii ? rows1[j] : rows0[j]) + biasv[j]) * kLog2e - cb;
#pragma unroll
      for (int r = 0; r < 4; ++r) x[j][r] = __builtin_amdgcn_exp2f(a[r]);
    }
    if (edge) {        // (wave-uniform: only the last column tile holds columns >= V)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (nw + j * 16 + fg * 4 + r >= V) x[j][r] = 0.f;
    }
    if (__any((unsigned)(tc + fg * 4) < 64u)) {      // (wave-uniform: one of these 16 rows has its target in this 64-column block)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (j * 16 + r == tc) x[j][r] = 0.f;
    }
    f32x4 s4 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bf16x4 xb = bf16x4{(bf16)x[j][0], (bf16)x[j][1], (bf16)x[j][2], (bf16)x[j][3]};
      *reinterpret_cast<bf16x4*>(r1 + ep_off8<true>(ii * 16 + fr, (j * 16 + fg * 4) * 2)) = xb;
#pragma unroll
      for (int r = 0; r < 4; ++r) s4[r] += (float)xb[r];
    }
    float sm = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    sm += __shfl_xor(sm, 16, 64);
    sm += __shfl_xor(sm, 32, 64);
    if (fg == 0) stats[mrow0 + ii * 16 + fr] = sm;
  }
  bf16* Cp = C + (size_t)mrow0 * ldc + nw + sch * 8;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int row = it * 8 + srow;
    st16p<true>(Cp + (size_t)row * ldc, flip_halves(*reinterpret_cast<const u32x4*>(r1 + ep_off<true>(row, sch * 16)), it & 1));
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The lin1 + GELU + byte epilogue (M3P_EPI_BIAS_GELUQ) from ONE table read per element (round 6).  h = gelu_erf(u) is staged
// to row order like any output tile; gelu_erf'(u) leaves as one byte per element straight from the accumulator layout in
// fragment order - what M3P_EPI_MULQ reads back the same way; u itself is never stored.
// The round-4 form evaluated erf and the Gaussian on the VALU - ~17 issue slots and two quarter-rate
// transcendentals per element, with the matrix pipe idle: measured (profiles/r06_gq_ablation.txt) the arithmetic alone is
// 46-64 us of the 232-us launch.  Both results are functions of x, and to the accuracy a bf16 output and a one-byte code can
// carry they are functions of the upper 16 bits of x:
//     h(x)     = max(x, 0) - |x| T(|x|)          T = 1 - Phi, the upper Gaussian tail
//     code(x)  = c(|x|) ^ (x < 0 ? 0xFF : 0)     c = the byte code of gelu'(|x|) (common.hpp: the grid is symmetric about 1/2)
// so one 32-bit table word per bf16 magnitude holds T as an fp32 whose low mantissa byte is replaced by c (T keeps 15
// mantissa bits: relative error 2^-16, far below the bf16 rounding of h).  The index is the TRUNCATED bf16 magnitude of the
// fp32 x (one v_bfe - no rounding instruction), clamped to |x| in [2^-11, 8) (one v_med3); the entry is evaluated at the
// MIDDLE of its truncation bucket, which makes the index error that of round-to-nearest (|dx| <= 2^-9 |x|, what a bf16
// pre-activation would carry anyway).  x itself enters h in full fp32 (fma(-|x|, T, max(x, 0))).
// Per element: v_bfe, v_med3, v_lshl_add (address), ds_read_b32, v_max, v_fma, half a v_cvt_pk_bf16 and 7/4 of an
// instruction for the code (v_perm gathers the four code bytes and - selectors 9 / 11 - the four sign masks) = ~7 VALU + 1 LDS
// read; the bias rides in the accumulators (they start an output tile at the bias instead of zero), so there is no add.
// 16-row pieces: staging 2 KB per wave + 1 KB for the 8-bit copy, the 7-KB table beside them (31 of the 32 KB the two stages leave).
// ---------------------------------------------------------------------------------------------------------------------
// |x| in [2^-11, 8): 14 exponents x 128 mantissas = 1792 words, 7 KB (below 2^-11 the first entry serves: T = 0.4998 against
// 1/2 - 0.4 |x|, an error of 4e-4 relative in h, a fifth of its bf16 rounding; gelu' = 1/2 +- 4e-4 -> codes 128 / 127 either way).
// The 2 KB this saves against the dGELU table's range [2^-15, 8) are what lets the 8-bit copy of h have staging rows of its own.
constexpr int GQ_TAB_LO = 0x3A00, GQ_TAB_HI = 0x4100, GQ_TAB_N = GQ_TAB_HI - GQ_TAB_LO;
constexpr int GQ_TAB_BYTES = GQ_TAB_N * 4;
__device__ __forceinline__ void geluq_table_fill(uint32_t* tab, int tid, int nthreads) {
  for (int i = tid; i < GQ_TAB_N; i += nthreads) {
    // middle of the truncation bucket of bf16 magnitude GQ_TAB_LO + i (the last bucket stands for every |x| >= 8, the first
    // for every |x| < 2^-11: T = 1/2 there, code 128 - half a step from gelu'(0) = 1/2 like its mirror image 127)
    const float xm = __builtin_bit_cast(float, ((uint32_t)(GQ_TAB_LO + i) << 16) | 0x8000u);
    const float tail = 0.5f * erfcf(xm * 0.70710678118654752440f);
    const float gd = (1.0f - tail) + xm * 0.39894228040143267794f * __expf(-0.5f * xm * xm);
    tab[i] = (__builtin_bit_cast(uint32_t, tail) & 0xFFFFFF00u) | gelu_grad_code(gd);
  }
}
__device__ __forceinline__ void lds_r32(uint32_t a, uint32_t& v) { asm volatile("ds_read_b32 %0, %1" : "=v"(v) : "v"(a)); }
// one 16-row piece (this wave's 16 x 64 block at (mrow0, nw)): `rows` = accumulators INCLUDING the bias, tab_off = LDS byte
// address of the table minus 4 * GQ_TAB_LO, r1 = the wave's 2 KB of staging rows, qout = where the piece's 1024 code bytes go
template <int O8 = 0>      // 0: no 8-bit copy of h, 1: e4m3
__device__ __forceinline__ void epilogue_piece_geluq_lut(bf16* __restrict__ C, int ldc, uint8_t* __restrict__ qout, int mrow0, int nw,
                                                         char* r1, const f32x4 (&rows)[4], int lane, uint32_t tab_off,
                                                         uint8_t* __restrict__ o8 = nullptr, int ld8 = 0, float scale8 = 1.f, float* amax = nullptr,
                                                         char* r8 = nullptr) {
  const int fr = lane & 15, fg = lane >> 4;
  const int srow = lane >> 3, sch = lane & 7;
  uint32_t w8[4];
  uint32_t w[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float xf = rows[j][r];       // (through a scalar: __builtin_bit_cast applied to a vector ELEMENT reads element 0 - seen in the ISA)
      const uint32_t xb = __builtin_bit_cast(uint32_t, xf);
      const uint32_t mag = __builtin_amdgcn_ubfe(xb, 16, 15);
      const uint32_t idx = min(max(mag, (uint32_t)GQ_TAB_LO), (uint32_t)(GQ_TAB_HI - 1));     // (v_med3_u32)
      lds_r32((idx << 2) + tab_off, w[j][r]);
    }
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(w[0][0]), "+v"(w[0][1]), "+v"(w[0][2]), "+v"(w[0][3]), "+v"(w[1][0]), "+v"(w[1][1]), "+v"(w[1][2]), "+v"(w[1][3]),
                                        "+v"(w[2][0]), "+v"(w[2][1]), "+v"(w[2][2]), "+v"(w[2][3]), "+v"(w[3][0]), "+v"(w[3][1]), "+v"(w[3][2]), "+v"(w[3][3]));
  const uint32_t la = lds_addr(r1);
  u32x4 code;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f32x4 hv;
    float xs[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      xs[r] = rows[j][r];
      // two instructions, written out: from C the compiler canonicalises the MFMA result first (v_max x, x) and forms -|x| with
      // an extra v_or to feed a packed fma (5 issue slots per element instead of 2)
      float mx;
      asm("v_max_f32 %0, 0, %1" : "=v"(mx) : "v"(xs[r]));
      asm("v_fma_f32 %0, -|%1|, %2, %3" : "=v"(hv[r]) : "v"(xs[r]), "v"(w[j][r]), "v"(mx));
    }
    // code bytes 0 / 1 / 2 / 3 = low byte of w[j][0..3]; sign masks (0xFF where x < 0) by the sign-replicating selectors
    const uint32_t x0 = __builtin_bit_cast(uint32_t, xs[0]), x1 = __builtin_bit_cast(uint32_t, xs[1]);
    const uint32_t x2 = __builtin_bit_cast(uint32_t, xs[2]), x3 = __builtin_bit_cast(uint32_t, xs[3]);
    const uint32_t blo = __builtin_amdgcn_perm(w[j][1], w[j][0], 0x0c0c0400u), bhi = __builtin_amdgcn_perm(w[j][3], w[j][2], 0x04000c0cu);
    const uint32_t slo = __builtin_amdgcn_perm(x1, x0, 0x0c0c0b09u), shi = __builtin_amdgcn_perm(x3, x2, 0x0b090c0cu);
    code[j] = (blo | bhi) ^ (slo | shi);
    lds_w64(la + ep_off8<true>(fr, (j * 16 + fg * 4) * 2), bf16x4{(bf16)hv[0], (bf16)hv[1], (bf16)hv[2], (bf16)hv[3]});
    if (O8) w8[j] = pack8<false>(hv, scale8, *amax);
  }
  st16p<true>(qout + lane * 16, code);
  if (O8) piece8_write(r8, w8, lane);      // (staging rows of its own: its round trip shares the bf16 piece's wait)
  u32x4 R[2];
  u32x4_lds R8;
  lds_r128(la + ep_off<true>(srow, sch * 16), R[0]);
  lds_r128(la + ep_off<true>(8 + srow, sch * 16), R[1]);
  const int row8 = lane >> 2, c8 = lane & 3;
  if (O8) {
    lds_r128(lds_addr(r8) + row8 * 64 + (c8 << 4), R8);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(R[0]), "+v"(R[1]), "+v"(R8));
  } else {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(R[0]), "+v"(R[1]));
  }
  bf16* Cp = C + (size_t)mrow0 * ldc + nw + sch * 8;
  st16p<true>(Cp + (size_t)srow * ldc, R[0]);
  st16p<true>(Cp + (size_t)(8 + srow) * ldc, flip_halves(R[1], true));
  if (O8) st16p<true>(o8 + (size_t)(mrow0 + row8) * ld8 + nw + ((c8 ^ ((row8 >> 1) & 3)) << 4), u32x4{R8[0], R8[1], R8[2], R8[3]});
}


// ---------------------------------------------------------------------------------
// NT kernel, persistent ring version (the production path): one 8-wave workgroup per CU walks
// a list of 256x128 output tiles; the K-tiles of all its output tiles form ONE continuous
// stream through three 48-KB LDS stages (144 of the CU's 160 KB):
//   * HBM -> LDS loads (global_load_lds) run TWO K-tiles ahead of the MFMAs — across output
//     tile boundaries too, so the next tile's operands arrive during this tile's epilogue —
//     and are retired with a COUNTED s_waitcnt vmcnt(6) (one K-tile = 6 LDS-DMA instructions
//     per wave stays in flight across the barrier); one raw s_barrier per K-tile;
//   * MFMA operand fragments are double-buffered per 32-deep k-step with inline-asm
//     ds_read_b128 (our wait, not the compiler's): 8 reads are issued, the 16 MFMAs of the
//     other fragment set hide them (cdna guide 5.7 form iii);
//   * no per-tile workgroup launch (measured: 3.2 us of a 17 us tile), no drained pipeline;
//   * the epilogue stages its bf16 tile in the LDS stage that was just consumed.
// Tile order: round r of the persistent loop gives XCD x the 32 consecutive tile ids
// [256 r + 32 x, +32): n-tiles of the same A row-panel share that XCD's L2.
// ---------------------------------------------------------------------------------
template <int EPI>
__global__ __launch_bounds__(512)
void gemm_nt_ring_kernel(const bf16* __restrict__ A, int lda, const bf16* __restrict__ W, int ldw,
                         bf16* __restrict__ C, int ldc, int M, int N, int K, M3PEpilogue ep,
                         int tiles_m, int tiles_n) {
  constexpr int BM = 256, BN = 128, NWAVES = 8;
  constexpr int A_BYTES = BM * ROWB, B_BYTES = BN * ROWB, STAGE = A_BYTES + B_BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ntiles = tiles_m * tiles_n;
  // tile id -> (tm, tn): n-fastest shares the A row-panel between neighbours (weights small
  // enough for L2/MALL); strips pay off once a full row of n-tiles no longer fits beside the A panels (measured:
  // 24 n-tiles 805 -> 914 TF with 8-wide strips; 18 n-tiles lose ~5 %, so those stay n-fastest)
  const int strip_w = strip_width(tiles_n, 24, 8);
  // (default order: strips of ~8 n-tiles walked m-major, so the 32 consecutive tiles an XCD
  //  holds in one round form a ~4 x 8 block: 4 A row-panels + 8 W panels are live per XCD
  //  instead of 1.3 + 24 -> fewer unique bytes per step in the 4-MB L2.  m-fastest order for a huge W used to win; with the
  //  strips the vocabulary projection went 2.20 -> 2.05 ms, 9.3 -> ~2 GB of reads)
  const int nwg = gridDim.x;
  // persistent schedule: sequence index q -> tile id
  const int slot = xcd_slot(nwg);
  auto tile_of = [&](int q) { return q * nwg + slot; };
  const int my_tiles = (ntiles > slot) ? (ntiles - slot + nwg - 1) / nwg : 0;
  if (my_tiles == 0) return;
  // dGELU: derivative table behind the three stages (visible to everyone after the first K-tile barrier)
  float* gtab = (EPI == M3P_EPI_DGELU) ? reinterpret_cast<float*>(smem + 3 * STAGE) : nullptr;
  if (EPI == M3P_EPI_DGELU) gelu_grad_table_fill(gtab, tid, 512);
  const int nk = K / BK;
  const int total = my_tiles * nk;

  // ---- load cursor
  const int sr = lane >> 3, sc = (lane & 7) ^ sr;
  const bf16* a_src[4];
  const bf16* w_src[2];
  int l_q = 0, l_kt = 0;
  auto set_load_tile = [&](int q) {
    const int t = tile_of(q);
    int tm, tn;
    split_tile(t, tiles_m, tiles_n, strip_w, tm, tn);
#pragma unroll
    for (int i = 0; i < 4; ++i) a_src[i] = A + (size_t)min(tm * BM + (wid + i * NWAVES) * 8 + sr, M - 1) * lda + sc * 8;
#pragma unroll
    for (int i = 0; i < 2; ++i) w_src[i] = W + (size_t)min(tn * BN + (wid + i * NWAVES) * 8 + sr, N - 1) * ldw + sc * 8;
  };
  // one K-tile of the stream = 6 LDS-DMA instructions per wave (4 of A, 2 of W).  They are
  // issued ONE AT A TIME between groups of MFMAs (issue_load(s, 0..5)): the CU's texture path
  // takes ~16 cycles per 1-KiB instruction, and a wave that sits in a burst of six cannot
  // issue its own MFMAs meanwhile (measured: 19 % of wave time in the issue burst, 21 % at the
  // barrier waiting for the waves still issuing).
  auto issue_load = [&](int s, int piece) {
    char* sa = smem + s * STAGE;
    const int k0 = l_kt * BK;
    if (piece < 4)
      __builtin_amdgcn_global_load_lds(GLB_PTR(a_src[piece] + k0), LDS_PTR(sa + (wid + piece * NWAVES) * 1024), 16, 0, 0);
    else
      __builtin_amdgcn_global_load_lds(GLB_PTR(w_src[piece - 4] + k0), LDS_PTR(sa + A_BYTES + (wid + (piece - 4) * NWAVES) * 1024), 16, 0, 0);
  };
  auto load_done = [&]() {
    if (++l_kt == nk) { l_kt = 0; ++l_q; if (l_q < my_tiles) set_load_tile(l_q); }
  };
  auto stage_next = [&](int s) {
#pragma unroll
    for (int pc = 0; pc < 6; ++pc) issue_load(s, pc);
    load_done();
  };

  // ---- fragment addressing
  const int wm = wid >> 1, wn = wid & 1;
  const int fr = lane & 15, fg = lane >> 4;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  uint32_t a_addr[2], b_addr[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const int ch = ((fg + 4 * ks) ^ (fr & 7)) * 16;
    a_addr[ks] = lds0 + (wm * 64 + fr) * ROWB + ch;
    b_addr[ks] = lds0 + A_BYTES + (wn * 64 + fr) * ROWB + ch;
  }
  auto read_set = [&](uint32_t aa, uint32_t ba, bf16x8 (&af)[4], bf16x8 (&wf)[4]) {
    M3P_DSR(wf[0], ba, 0); M3P_DSR(af[0], aa, 0);
    M3P_DSR(wf[1], ba, 2048); M3P_DSR(wf[2], ba, 4096); M3P_DSR(wf[3], ba, 6144);
    M3P_DSR(af[1], aa, 2048); M3P_DSR(af[2], aa, 4096); M3P_DSR(af[3], aa, 6144);
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto mfma_batch = [&](const bf16x8 (&af)[4], const bf16x8 (&wf)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], af[i], acc[i][j], 0, 0, 0);
  };
  // (Tried and measured neutral-to-negative on MI355X, kept out: issuing the six LDS-DMAs one
  //  at a time between MFMAs; giving the two waves of a SIMD different burst positions —
  //  before/after MFMA batch 1, or after the mid-step barrier; a 256x256 tile with 32-deep
  //  stages.  See DESIGN.md §4 "what did not work".)

  // ---- prologue of the stream
  set_load_tile(0);
  stage_next(0);
  if (total > 1) {
    stage_next(1);
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  bf16x8 af0[4], wf0[4], af1[4], wf1[4];
  read_set(a_addr[0], b_addr[0], af0, wf0);
  M3P_WAIT_LGKM(0);
  int cur = 0;      // stage of the current K-tile
  int c_q = 0, c_kt = 0;
  const bool io_aligned = ((ldc & 7) == 0) && (((uintptr_t)C & 15) == 0) &&
                          (!(EPI == M3P_EPI_BIAS_GELU) || (((ep.ld_out2 & 7) == 0) && (((uintptr_t)ep.out2 & 15) == 0))) &&
                          (!ep.bias || (((uintptr_t)ep.bias & 15) == 0)) &&
                          (!ep.aux || (((ep.ld_aux & 7) == 0) && (((uintptr_t)ep.aux & 15) == 0)));
  f32x4 csum[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) csum[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  int csum_nw = -1;            // first column of the 64-wide block the sums belong to
  auto flush_csum = [&]() {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float sfl = csum[j][r];
        sfl += __shfl_xor(sfl, 1, 64); sfl += __shfl_xor(sfl, 2, 64);
        sfl += __shfl_xor(sfl, 4, 64); sfl += __shfl_xor(sfl, 8, 64);
        const int n = csum_nw + j * 16 + fg * 4 + r;
        if (fr == 0 && n < N) unsafeAtomicAdd(ep.colsum + n, sfl);
        csum[j][r] = 0.f;
      }
  };
  for (int step = 0; step < total; ++step) {
    const int nxt = (cur == 2) ? 0 : cur + 1;
    const int nx2 = (nxt == 2) ? 0 : nxt + 1;
    const bool more2 = (step + 2 < total);
    if (more2) stage_next(nx2);
    read_set(a_addr[1] + cur * STAGE, b_addr[1] + cur * STAGE, af1, wf1);
    __builtin_amdgcn_sched_barrier(0);   // reads first, then the MFMAs that hide them
    mfma_batch(af0, wf0);
    // k-step-1 fragments are in; every LDS read of this K-tile is complete; the next K-tile
    // has landed for this wave (the 6 LDS-DMAs just issued stay in flight) -> publish
    M3P_WAIT_LGKM(0);
    if (more2) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    read_set(a_addr[0] + nxt * STAGE, b_addr[0] + nxt * STAGE, af0, wf0);   // stale after the last K-tile: unused
    __builtin_amdgcn_sched_barrier(0);
    mfma_batch(af1, wf1);
    M3P_WAIT_LGKM(0);

    if (++c_kt == nk) {
      // ---- epilogue of output tile c_q; stage `cur` is free (all waves passed the barrier above)
      c_kt = 0;
      const int t = tile_of(c_q);
      ++c_q;
      int tm, tn;
      split_tile(t, tiles_m, tiles_n, strip_w, tm, tn);
      const int m0 = tm * BM, n0 = tn * BN;
      const int mw = m0 + wm * 64, nw = n0 + wn * 64;
      // column sums (bias gradient of the dGELU / MUL epilogues) stay in registers across this workgroup's tiles
      // and are flushed when its column block changes: with the strip order that is once per strip, not once
      // per tile (per tile the 64 shuffles + 16 atomics cost 5.4 k cycles, and the atomics - older than the next
      // K-tile's LDS-DMAs in the vmcnt order - stalled the K loop: +29 % on the whole launch)
      if ((EPI == M3P_EPI_DGELU || EPI == M3P_EPI_MUL) && ep.colsum && csum_nw != nw) {
        if (csum_nw >= 0) flush_csum();
        csum_nw = nw;
      }
      const bool fast = io_aligned && (m0 + BM <= M) && (n0 + BN <= N);
      if (fast) {
        char* r1 = smem + cur * STAGE + wid * 6144;
        // both halves' aux rows are requested up front: the second half's round trip hides behind the first half's work
        u32x4 auxt0[4], auxt1[4];
        load_aux_rows_issue<EPI>(ep, mw, nw, lane, auxt0);
        load_aux_rows_issue<EPI>(ep, mw + 32, nw, lane, auxt1);
        auto do_half = [&](const int hf, const u32x4 (&auxt)[4]) {
          f32x4 rows[2][4];
#pragma unroll
          for (int ii = 0; ii < 2; ++ii)
#pragma unroll
            for (int j = 0; j < 4; ++j) rows[ii][j] = acc[2 * hf + ii][j];
          f32x4 biasv[4];
          bf16x4 auxv[2][4];
          load_bias4<EPI>(ep, nw, lane, biasv);
          load_aux_rows_finish<EPI>(lane, r1, auxt, auxv);
          epilogue_half<EPI>(ep, C, ldc, N, mw + 32 * hf, nw, r1, rows, biasv, auxv, lane, csum, gtab);
        };
        do_half(0, auxt0);
        do_half(1, auxt1);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            epilogue_store<EPI>(ep, C, ldc, M, N, mw + i * 16 + fr, nw + j * 16 + fg * 4, acc[i][j], csum[j]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (step + 1 < total) {
        // the staging region is the slot the next iteration's loads go into: nobody may issue
        // them before every wave has finished its LDS round trip
        M3P_WAIT_LGKM(0);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
      }
    }
    cur = nxt;
  }
  if ((EPI == M3P_EPI_DGELU || EPI == M3P_EPI_MUL) && ep.colsum && csum_nw >= 0) flush_csum();
}


// ---------------------------------------------------------------------------------
// NT kernel, "w8" version: 256x256 output tile, EIGHT waves (2 x 4), 128x64 per wave, two 64-KB LDS stages.
// The four-wave kernel's timeline: a wave alone on its SIMD loses ~32 clocks of matrix pipe to each of its
// 16 LDS-DMA instructions per K-tile and issues 16x16x32 MFMAs every ~18 clocks instead of 16 - 29 % of the K loop - and
// pays the whole epilogue (20 % of a K = 768 launch) with the pipe idle; neither depends on the MFMA shape.  With two
// waves per SIMD the partner's MFMAs fill those holes.  What made the earlier eight-wave kernels LDS-bound was 64x64 per
// wave (256 KB of fragment reads per K-tile and CU); 128x64 per wave reads 192 KB (94 B/clk/CU over the 2048 clocks of a
// K-tile) and halves the LDS-DMAs per wave (8 per K-tile).  This is the geometry the CDNA4 guide's 256^2 template runs.
// Pipeline per K-tile (one barrier): read k-step 1 | 32 MFMAs on k-step 0 | lgkm, vmcnt(0) (K-tile +1 was requested one
// full K-tile ago), s_barrier | request K-tile +2 into the stage just vacated | read k-step 0 of K-tile +1 | 32 MFMAs on
// k-step 1.  The epilogue stages through the vacated stage (the request for K-tile +2 waits for it on an output tile's
// last K-tile).  128 accumulator + 96 fragment registers per lane: the compiler's allocation (no literal AGPR numbers).
// ---------------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ const T* uniform_ptr(const T* p) {      // a wave-uniform pointer the compiler may not know to be one
  const uint64_t v = reinterpret_cast<uint64_t>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return reinterpret_cast<const T*>(((uint64_t)hi << 32) | lo);
}

template <int EPI, bool DYN = false, bool O8 = false>      // O8: BIAS_GELUQ / MULQ also leave the 8-bit copy (M3PEpilogue::out8)
__global__ __launch_bounds__(512)
void gemm_nt_w8_kernel(const bf16* __restrict__ A, int lda, const bf16* __restrict__ W, int ldw,
                       bf16* __restrict__ C, int ldc, int M, int N, int K, M3PEpilogue ep,
                       int tiles_m, int tiles_n, int* __restrict__ tile_ctr) {
  constexpr int BM = 256, BN = 256, NWAVES = 8;
  constexpr int A_BYTES = BM * ROWB, STAGE = (BM + BN) * ROWB;      // 32 KB, 64 KB
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ntiles = tiles_m * tiles_n;
  // (round 6: nine n-tiles - the QKV projection - in three strips of three instead of one row of nine: 131.4 -> 124.1 us on
  //  one box, 132 -> 131 on two others - never slower; profiles/r06_qkv_strips.txt)
  const int strip_w = strip_width(tiles_n, 9, 4);
  // (its own copy of split_tile: with the shared one the byte / statistics instantiations come out scheduled differently)
  auto split_tile = [&](int t, int& tm, int& tn) {
    const int strip = t / (tiles_m * strip_w);
    const int rem = t - strip * tiles_m * strip_w;
    const int bn = min(strip_w, tiles_n - strip * strip_w);
    tm = rem / bn;
    tn = strip * strip_w + (rem - tm * bn);
  };
  const int nwg = gridDim.x;
  const int per_xcd = nwg >> 3;
  const int xcd = blockIdx.x & 7;
  const int slot = xcd_slot(nwg);
  if (slot >= ntiles) return;
  // Tile schedule.  Static: workgroup `slot` takes tiles slot, slot + nwg, ...  Dynamic (tile_ctr != NULL, data parallelism):
  // the first tile is the static one, every further tile is popped from its XCD's queue - the same tiles in the same order
  // (position p of XCD x = tile (p / per_xcd) * nwg + x * per_xcd + p % per_xcd), but a workgroup whose CU is shared with a
  // collective's kernel simply pops fewer of them instead of holding the whole launch back (profiles/r03_dynamic_tiles.txt).
  // One lane pops (an L2 atomic) while the loader is three K-tiles into a tile, hands the result to the other waves through
  // four bytes of wave 0's epilogue staging rows (idle inside the K loop) across two K-tile barriers, and the loader picks
  // it up when it moves on nk - 3 K-tiles later: nothing waits for the atomic.
  const int nk = K / BK;
  constexpr bool dyn = DYN;       // (a separate instantiation: the queue's bookkeeping costs a dozen registers)
  auto tile_of = [&](int q) { return q * nwg + slot; };
  const int my_tiles = (ntiles - slot + nwg - 1) / nwg;      // (static schedule)
  const int total = my_tiles * nk;
  int t_ld = slot, t_cmp = slot, t_next = -1;               // (dynamic schedule: tiles being loaded / computed, the popped one)
  int pop_state = 0;        // 1: popped this K-tile (wave 0 publishes after the barrier), 2: published (everyone reads after the next)
  unsigned popped = 0;
  // The epilogue stages through the 32 KB beside the two stages (swizzled 128-byte rows: 4 KB per wave, or 2 KB for the
  // 16-row pieces of the multiply epilogues, whose derivative table lives there too) instead of the stage the output tile's
  // last K-tile vacated: the next tile's K-tile 1 is then requested on schedule and nobody has to meet at a barrier after
  // the epilogue.
  constexpr bool kMulE = (EPI == M3P_EPI_DGELU || EPI == M3P_EPI_MUL || EPI == M3P_EPI_MULQ);
  constexpr bool kAuxE = (EPI == M3P_EPI_BIAS_DROP_RES || EPI == M3P_EPI_RES || kMulE);
  constexpr bool kGqLut = (EPI == M3P_EPI_BIAS_GELUQ);
  constexpr int kTabBytes = (EPI == M3P_EPI_DGELU) ? GELU_TAB_N * (int)sizeof(float) : (kGqLut ? GQ_TAB_BYTES : 0);
  float* gtab = (EPI == M3P_EPI_DGELU) ? reinterpret_cast<float*>(smem + 2 * STAGE) : nullptr;
  if (EPI == M3P_EPI_DGELU) gelu_grad_table_fill(gtab, tid, 512);
  if (kGqLut) geluq_table_fill(reinterpret_cast<uint32_t*>(smem + 2 * STAGE), tid, 512);      // (the prologue's barrier publishes it)
  int* const mbox = reinterpret_cast<int*>(smem + 2 * STAGE + kTabBytes);

  // ---- load cursor: one LDS-DMA = 8 rows x 128 B (lane -> row l >> 3, LDS slot l & 7, source chunk slot ^ (row & 7)).  A wave
  //      stages 32 CONSECUTIVE rows of each operand (pieces 1 KB apart in LDS) as buffer_load_dwordx4 ... lds: resource = the
  //      wave's slice of the operand tile, scalar offset = K-tile + piece, one 32-bit lane offset per operand, the destination
  //      picked by the immediate offset, which moves the source by the same bytes (tools/probe_dma_offset.py; the four-wave
  //      kernels do the same).  Per LDS-DMA that saves the M0 write and its hazard nop (probe_issue.py: ~32 of the ~70 ticks a
  //      piece costs).
  const int sr = lane >> 3, sc = (lane & 7) ^ sr;
  int l_kt = 0, l_q = 0;
  bool l_alive = true;      // (dynamic) the load cursor points at a K-tile of this workgroup's stream
  __amdgpu_buffer_rsrc_t a_rsrc, w_rsrc;
  auto set_load_tile = [&](int t) {
    int tm, tn;
    split_tile(t, tm, tn);
    const bf16* a_src = A + (size_t)(tm * BM + wid * 32) * lda;
    const bf16* w_src = W + (size_t)(tn * BN + wid * 32) * ldw;
    a_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(uniform_ptr(a_src)), 0, 0xffffffff, 0x00020000);
    w_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(uniform_ptr(w_src)), 0, 0xffffffff, 0x00020000);
  };
  const uint32_t a_lane = (uint32_t)(sr * lda + sc * 8) * 2u, w_lane = (uint32_t)(sr * ldw + sc * 8) * 2u;
  auto issue_load = [&](int s, int piece) {
    char* sa = smem + s * STAGE;
    const int k0 = l_kt * BK;
    const int pc = piece & 3;
    char* base = sa + (piece < 4 ? 0 : A_BYTES) + wid * 4096;
    const uint32_t soff = __builtin_amdgcn_readfirstlane((uint32_t)k0 * 2u + (uint32_t)pc * (uint32_t)((piece < 4 ? lda : ldw) * 16) - (uint32_t)pc * 1024u);
#define W8_LDB(IMM) __builtin_amdgcn_raw_ptr_buffer_load_lds(piece < 4 ? a_rsrc : w_rsrc, LDS_PTR(base), 16, piece < 4 ? a_lane : w_lane, soff, IMM, 0)
    switch (pc) {
      case 0: W8_LDB(0); break;
      case 1: W8_LDB(1024); break;
      case 2: W8_LDB(2048); break;
      default: W8_LDB(3072); break;
    }
#undef W8_LDB
  };
  auto load_done = [&]() {
    if constexpr (!dyn) {
      if (++l_kt == nk) { l_kt = 0; ++l_q; if (l_q < my_tiles) set_load_tile(tile_of(l_q)); }
    } else {
      ++l_kt;
      if (l_kt == 3) {
        pop_state = 1;
        if (wid == 0 && lane == 0) popped = __hip_atomic_fetch_add(reinterpret_cast<unsigned*>(tile_ctr) + xcd, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      if (l_kt == nk) {
        l_kt = 0;
        t_ld = t_next;
        t_next = -1;
        if (t_ld >= 0) set_load_tile(t_ld); else l_alive = false;
      }
    }
  };
  auto stage_next = [&](int s) {
#pragma unroll
    for (int pc = 0; pc < 8; ++pc) issue_load(s, pc);
    load_done();
  };

  // ---- fragment addressing (128-B rows, chunk ^= row & 7): A fragment i at + i * 2048, W fragment j at + j * 2048
  const int wm = wid >> 2, wn = wid & 3;
  const int fr = lane & 15, fg = lane >> 4;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  uint32_t a_addr[2], b_addr[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const int ch = ((fg + 4 * ks) ^ (fr & 7)) * 16;
    a_addr[ks] = lds0 + (wm * 128 + fr) * ROWB + ch;
    b_addr[ks] = lds0 + A_BYTES + (wn * 64 + fr) * ROWB + ch;
  }
  // fragments are fetched a QUARTER K-tile (16 MFMAs) ahead: four W fragments per k-step, four A fragments per half
  // (64 fragment registers instead of the 96 of a whole k-step ahead - with 128 accumulators that is the difference
  // between fitting the 256 registers two waves per SIMD leave and spilling inside the K loop)
  auto read_w = [&](uint32_t ba, bf16x8 (&wf)[4]) {
    M3P_DSR(wf[0], ba, 0); M3P_DSR(wf[1], ba, 2048); M3P_DSR(wf[2], ba, 4096); M3P_DSR(wf[3], ba, 6144);
  };
  auto read_a_lo = [&](uint32_t aa, bf16x8 (&af)[4]) {
    M3P_DSR(af[0], aa, 0); M3P_DSR(af[1], aa, 2048); M3P_DSR(af[2], aa, 4096); M3P_DSR(af[3], aa, 6144);
  };
  auto read_a_hi = [&](uint32_t aa, bf16x8 (&af)[4]) {
    M3P_DSR(af[0], aa, 8192); M3P_DSR(af[1], aa, 10240); M3P_DSR(af[2], aa, 12288); M3P_DSR(af[3], aa, 14336);
  };

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (kGqLut) {      // the accumulators of an output tile start at its bias (this lane's columns nw + 16 j + 4 fg .. + 3)
    int tm0, tn0;
    split_tile(slot, tm0, tn0);
    const float* bp = ep.bias + tn0 * BN + wn * 64 + fg * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 b = *reinterpret_cast<const f32x4*>(bp + j * 16);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i][j] = b;
    }
  }
  // (raised priority around every MFMA cluster; a static priority for the younger half of the workgroup was the
  //  alternative measured - DESIGN.md)
  auto mfma_q = [&](auto half_c, const bf16x8 (&af)[4], const bf16x8 (&wf)[4]) {
    constexpr int I0 = 4 * decltype(half_c)::value;
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[I0 + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], af[i], acc[I0 + i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  };
  using H0 = std::integral_constant<int, 0>;
  using H1 = std::integral_constant<int, 1>;

  // ---- prologue: K-tiles 0 and 1 into stages 0 and 1
  set_load_tile(slot);
  stage_next(0);
#define W8_H1 (dyn ? h1d : (step + 1 < total))
#define W8_MORE2 (dyn ? l_alive : more2)
  bool h1d = l_alive;        // (dynamic) K-tile step + 1 of the stream exists (was, or is being, requested)
  if (dyn ? h1d : (total > 1)) {
    stage_next(1);
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  bf16x8 fa0[4], fa1[4], fw0[4], fw1[4];
  read_w(b_addr[0], fw0);
  read_a_lo(a_addr[0], fa0);
  M3P_WAIT_LGKM(0);
  int c_kt = 0, c_q = 0;
  const bool io_aligned = ((ldc & 7) == 0) && (((uintptr_t)C & 15) == 0) &&
                          (!(EPI == M3P_EPI_BIAS_GELU) || (((ep.ld_out2 & 7) == 0) && (((uintptr_t)ep.out2 & 15) == 0))) &&
                          (!ep.bias || (((uintptr_t)ep.bias & 15) == 0)) &&
                          (!ep.aux || (((ep.ld_aux & 7) == 0) && (((uintptr_t)ep.aux & 15) == 0)));
  f32x4 csum[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) csum[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  int csum_nw = -1;
  auto flush_csum = [&]() {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float sfl = csum[j][r];
        sfl += __shfl_xor(sfl, 1, 64); sfl += __shfl_xor(sfl, 2, 64);
        sfl += __shfl_xor(sfl, 4, 64); sfl += __shfl_xor(sfl, 8, 64);
        const int n = csum_nw + j * 16 + fg * 4 + r;
        if (fr == 0 && n < N) unsafeAtomicAdd(ep.colsum + n, sfl);
        csum[j][r] = 0.f;
      }
  };
  float amax_run = 0.f;       // (BIAS_GELUQ with an 8-bit copy: this lane's max |output| over the launch; MULQ keeps it in LDS)
  if constexpr (O8 && EPI == M3P_EPI_MULQ) reinterpret_cast<float*>(smem + 2 * STAGE + 8 * 2048)[tid] = 0.f;
  bool spread_pending = false;
  for (int step = 0; dyn || step < total; ++step) {
    const int cur = step & 1, nxt = cur ^ 1;
    const bool last_kt = (c_kt + 1 == nk);
    // K-tile step + 2 exists (it is requested during this step).  Dynamic: known once quarter 1 has advanced the load cursor
    const bool more2 = dyn ? false : (step + 2 < total);
    const uint32_t so = cur * STAGE;
    const bool pend = spread_pending;      // the request for K-tile +1 started in the previous quarter 3
    // quarter 0: k-step 0, rows 0-63 | fetch k-step 0, rows 64-127
    if (pend) { issue_load(nxt, 3); issue_load(nxt, 4); issue_load(nxt, 5); }
    read_a_hi(a_addr[0] + so, fa1);
    __builtin_amdgcn_sched_barrier(0);
    mfma_q(H0{}, fa0, fw0);
    M3P_WAIT_LGKM(0);
    // quarter 1: k-step 0, rows 64-127 | fetch k-step 1: W and rows 0-63
    if (pend) { issue_load(nxt, 6); issue_load(nxt, 7); }
    read_w(b_addr[1] + so, fw1);
    read_a_lo(a_addr[1] + so, fa0);
    __builtin_amdgcn_sched_barrier(0);
    mfma_q(H1{}, fa1, fw0);
    if (pend) { load_done(); spread_pending = false; }
    M3P_WAIT_LGKM(0);
    // quarter 2: k-step 1, rows 0-63 | fetch k-step 1, rows 64-127 (the last LDS read of this K-tile)
    read_a_hi(a_addr[1] + so, fa1);
    __builtin_amdgcn_sched_barrier(0);
    mfma_q(H0{}, fa0, fw1);
    // every LDS read of this K-tile is complete and K-tile +1, requested one K-tile ago, has landed for this wave
    M3P_WAIT_LGKM(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (dyn && pop_state) {
      if (pop_state == 1) {
        if (wid == 0 && lane == 0) {
          const int p = per_xcd + (int)popped, q = p / per_xcd;
          const int t = q * nwg + xcd * per_xcd + (p - q * per_xcd);
          *mbox = (t < ntiles) ? t : -1;
        }
        pop_state = 2;
      } else {
        t_next = __builtin_amdgcn_readfirstlane(*mbox);
        pop_state = 0;
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // quarter 3: k-step 1, rows 64-127 | request K-tile +2 into the vacated stage | fetch K-tile +1's first fragments
    // (on an output tile's last K-tile both wait for the epilogue, which stages through that stage and wants the registers)
    // (epilogues with an aux tile ask for it FIRST: vmcnt retires in order, so a load issued behind the three LDS-DMAs
    //  would wait for them too - on an output tile's last K-tile the request moves into the epilogue, behind the aux loads)
    const bool req = W8_MORE2 && (!last_kt || !kAuxE);
    if (req) {
      issue_load(cur, 0); issue_load(cur, 1); issue_load(cur, 2);
      spread_pending = true;
    }
    if (W8_H1 && !last_kt) {
      read_w(b_addr[0] + nxt * STAGE, fw0);
      read_a_lo(a_addr[0] + nxt * STAGE, fa0);
    }
    __builtin_amdgcn_sched_barrier(0);
    mfma_q(H1{}, fa1, fw1);
    M3P_WAIT_LGKM(0);

    if (++c_kt == nk) {
      // ---- epilogue of output tile c_q through the vacated stage `cur`
      c_kt = 0;
      // (dynamic, nk >= 8: the loader moved on to the next tile two K-tiles ago; -1 behind the last one)
      const int t = dyn ? t_cmp : tile_of(c_q);
      if (dyn) t_cmp = t_ld; else ++c_q;
      int tm, tn;
      split_tile(t, tm, tn);
      const int m0 = tm * BM, n0 = tn * BN;
      const int mw = m0 + wm * 128, nw = n0 + wn * 64;
      if (kMulE && ep.colsum && csum_nw != nw) {
        if (csum_nw >= 0) flush_csum();
        csum_nw = nw;
      }
      const bool fast = io_aligned && (m0 + BM <= M) && (n0 + BN <= N);
      if constexpr (EPI == M3P_EPI_BIAS_LSE || EPI == M3P_EPI_BIAS_EXP) {
        if (fast) {
          char* r1 = smem + 2 * STAGE + wid * 4096;
          f32x4 biasv[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) biasv[j] = *reinterpret_cast<const f32x4*>(ep.bias + nw + j * 16 + (lane >> 4) * 4);
          const int V = ep.ld_out2;
          const bool edge = (nw + 64 > V);
          if constexpr (EPI == M3P_EPI_BIAS_EXP) {
            float* st = reinterpret_cast<float*>(ep.out2) + (size_t)(tn * 4 + wn) * M;
            const CeRowRef* ref = reinterpret_cast<const CeRowRef*>(ep.row_ref);
#pragma unroll
            for (int hf = 0; hf < 4; ++hf) {
              epilogue_half_exp(C, ldc, st, ref, V, mw + 32 * hf, nw, r1, acc[2 * hf], acc[2 * hf + 1], biasv, lane, edge);
              __builtin_amdgcn_sched_barrier(0);
            }
          } else {
            float2* st = reinterpret_cast<float2*>(ep.out2) + (size_t)(tn * 4 + wn) * M;
#pragma unroll
            for (int hf = 0; hf < 4; ++hf) {
              epilogue_half_lse(C, ldc, st, V, mw + 32 * hf, nw, r1, acc[2 * hf], acc[2 * hf + 1], biasv, lane, edge);
              __builtin_amdgcn_sched_barrier(0);
            }
          }
        }
      } else if constexpr (kGqLut) {
        // (the launcher admits whole, aligned tiles only: `fast` always holds)
        f32x4 bnext[4];
        {
          const bool more_tiles = dyn ? (t_cmp >= 0) : (c_q < my_tiles);       // (c_q / t_cmp already name the NEXT output tile)
          int tm2 = tm, tn2 = tn;
          if (more_tiles) split_tile(dyn ? t_cmp : tile_of(c_q), tm2, tn2);
          const float* bp = ep.bias + tn2 * BN + wn * 64 + fg * 4;
#pragma unroll
          for (int j = 0; j < 4; ++j) bnext[j] = *reinterpret_cast<const f32x4*>(bp + j * 16);
        }
        {
          char* r1 = smem + 2 * STAGE + kTabBytes + wid * 2048;
          const uint32_t tab_off = lds0 + 2 * STAGE - 4 * GQ_TAB_LO;
          uint8_t* qo = reinterpret_cast<uint8_t*>(ep.out2) + gq_block_offset(tm, tn, tiles_n, wid, 0);
          if constexpr (O8) {      // + the e4m3 copy of h for an fp8 lin2
            const float sc8 = ep.scale8 ? *ep.scale8 : 1.f;
#pragma unroll
            for (int hp = 0; hp < 8; ++hp) {
              epilogue_piece_geluq_lut<1>(C, ldc, qo + 1024 * hp, mw + 16 * hp, nw, r1, acc[hp], lane, tab_off,
                                          reinterpret_cast<uint8_t*>(ep.out8), ep.ld_out8, sc8, &amax_run,
                                          smem + 2 * STAGE + kTabBytes + 8 * 2048 + wid * 1024);
              __builtin_amdgcn_sched_barrier(0);
            }
          } else {
#pragma unroll
            for (int hp = 0; hp < 8; ++hp) {
              epilogue_piece_geluq_lut(C, ldc, qo + 1024 * hp, mw + 16 * hp, nw, r1, acc[hp], lane, tab_off);
              __builtin_amdgcn_sched_barrier(0);
            }
          }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = bnext[j];
      } else if constexpr (EPI == M3P_EPI_MULQ) {
        // byte derivative in fragment order: one 16-byte load per lane and 16-row piece, two pieces ahead (the launcher admits
        // whole tiles only, so `fast` always holds).  Measured and removed: all eight code loads
        // up front with all eight LDS-DMA pieces of K-tile +2 behind them; 32-row pieces; the codes prefetched by LDS-DMA a
        // whole K-tile ahead into the idle staging rows - all within 1 % of this form, while a build that reads no codes at
        // all is 23 us faster: what the codes cost is their 129 MB on the fabric, not their latency.
        if (fast) {
          const uint8_t* qp = reinterpret_cast<const uint8_t*>(ep.aux) + gq_block_offset(tm, tn, tiles_n, wid, 0) + lane * 16;
          char* r1 = smem + 2 * STAGE + wid * 2048;
#define MQ_LD(off) (*reinterpret_cast<const u32x4*>(qp + (off)))
          u32x4 qa = MQ_LD(0), qb = MQ_LD(1024);
          __builtin_amdgcn_sched_barrier(0);
          if (W8_MORE2) { issue_load(cur, 0); issue_load(cur, 1); issue_load(cur, 2); spread_pending = true; }
          __builtin_amdgcn_sched_barrier(0);
          if constexpr (O8) {      // + the 8-bit copy of dU for an fp8 dx1 product
            const float sc8 = ep.scale8 ? *ep.scale8 : 1.f;
            uint8_t* o8 = reinterpret_cast<uint8_t*>(ep.out8);
            // (this lane's running max |dU| lives in LDS between output tiles: one more register across the K loop spills here)
            float* amax_slot = reinterpret_cast<float*>(smem + 2 * STAGE + 8 * 2048) + tid;
            float amax_t = *amax_slot;
#pragma unroll
            for (int hp = 0; hp < 8; ++hp) {
              u32x4 qc = qb;
              if (hp + 2 < 8) qc = MQ_LD((hp + 2) * 1024);
              char* r8 = smem + 2 * STAGE + 8 * 2048 + 2048 + wid * 1024;
              // (e5m2 only: the copy of a GRADIENT - the launcher refuses anything else, one code path in the instantiation)
              epilogue_pieceq<2>(C, ldc, mw + 16 * hp, nw, r1, acc[hp], qa, lane, csum, o8, ep.ld_out8, sc8, &amax_t, r8);
              __builtin_amdgcn_sched_barrier(0);
              qa = qb; qb = qc;
            }
            *amax_slot = amax_t;
          } else {
#pragma unroll
          for (int hp = 0; hp < 8; hp += 2) {
            u32x4 qc = qa, qd = qb;
            if (hp + 2 < 8) qc = MQ_LD((hp + 2) * 1024);
            epilogue_pieceq(C, ldc, mw + 16 * hp, nw, r1, acc[hp], qa, lane, csum);
            __builtin_amdgcn_sched_barrier(0);
            if (hp + 3 < 8) qd = MQ_LD((hp + 3) * 1024);
            epilogue_pieceq(C, ldc, mw + 16 * (hp + 1), nw, r1, acc[hp + 1], qb, lane, csum);
            __builtin_amdgcn_sched_barrier(0);
            qa = qc; qb = qd;
          }
          }
#undef MQ_LD
        }
      } else if (fast && kMulE) {
        // 16-row pieces, the aux rows of the next piece in flight while this one is computed
        char* r1 = smem + 2 * STAGE + kTabBytes + wid * 2048;
        u32x4 ta[2], tb[2];
        aux16_issue(ep, mw, nw, lane, ta);
        __builtin_amdgcn_sched_barrier(0);
        if (W8_MORE2) { issue_load(cur, 0); issue_load(cur, 1); issue_load(cur, 2); spread_pending = true; }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int hp = 0; hp < 8; hp += 2) {
          aux16_issue(ep, mw + 16 * (hp + 1), nw, lane, tb);
          epilogue_piece16<EPI>(ep, C, ldc, mw + 16 * hp, nw, r1, acc[hp], ta, lane, csum, gtab);
          __builtin_amdgcn_sched_barrier(0);
          if (hp + 2 < 8) aux16_issue(ep, mw + 16 * (hp + 2), nw, lane, ta);
          epilogue_piece16<EPI>(ep, C, ldc, mw + 16 * (hp + 1), nw, r1, acc[hp + 1], tb, lane, csum, gtab);
          __builtin_amdgcn_sched_barrier(0);
        }
      } else if (fast) {
        char* r1 = smem + 2 * STAGE + wid * 4096;
        f32x4 biasv[4];
        load_bias4<EPI>(ep, nw, lane, biasv);
        u32x4 aux0[4];
        if (kAuxE) {
          load_aux_rows_issue<EPI>(ep, mw, nw, lane, aux0);
          __builtin_amdgcn_sched_barrier(0);
          if (W8_MORE2) { issue_load(cur, 0); issue_load(cur, 1); issue_load(cur, 2); spread_pending = true; }
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int hf = 0; hf < 4; ++hf) {
          f32x4 rows[2][4];
#pragma unroll
          for (int ii = 0; ii < 2; ++ii)
#pragma unroll
            for (int j = 0; j < 4; ++j) rows[ii][j] = acc[2 * hf + ii][j];
          bf16x4 auxv[2][4];
          if (kAuxE && hf == 0) load_aux_rows_finish<EPI, true>(lane, r1, aux0, auxv);
          else load_aux_rows<EPI, true>(ep, mw + 32 * hf, nw, lane, r1, auxv);
          epilogue_half<EPI, true>(ep, C, ldc, N, mw + 32 * hf, nw, r1, rows, biasv, auxv, lane, csum, gtab);
          __builtin_amdgcn_sched_barrier(0);      // one piece at a time: hoisted loads of the next piece cost registers
        }
      } else {
        if (kAuxE && W8_MORE2) { issue_load(cur, 0); issue_load(cur, 1); issue_load(cur, 2); spread_pending = true; }
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            epilogue_store<EPI>(ep, C, ldc, M, N, mw + i * 16 + fr, nw + j * 16 + fg * 4, acc[i][j], csum[j]);
      }
      if constexpr (!kGqLut) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      if (W8_H1) {
        read_w(b_addr[0] + nxt * STAGE, fw0);
        read_a_lo(a_addr[0] + nxt * STAGE, fa0);
        M3P_WAIT_LGKM(0);
      }
    }
    if (dyn) {
      if (!h1d) break;
      h1d = l_alive;
    }
  }
  if (kMulE && ep.colsum && csum_nw >= 0) flush_csum();
  if constexpr (O8 && (EPI == M3P_EPI_BIAS_GELUQ || EPI == M3P_EPI_MULQ)) {
    if (ep.amax8) {
      // one candidate per workgroup, and only if it beats what is there (same-address atomics serialise at the memory side:
      // optim.hip, quant_fp8_kernel); the staging rows are free now
      float* wmax = reinterpret_cast<float*>(smem + 2 * STAGE + kTabBytes);
      if constexpr (EPI == M3P_EPI_MULQ) amax_run = reinterpret_cast<float*>(smem + 2 * STAGE + 8 * 2048)[tid];
      const float mxw = wave_max(amax_run);
      __syncthreads();
      if (lane == 0) wmax[wid] = mxw;
      __syncthreads();
      if (tid == 0) {
        float mx = wmax[0];
#pragma unroll
        for (int w = 1; w < NWAVES; ++w) mx = fmaxf(mx, wmax[w]);
        unsigned int* slot = reinterpret_cast<unsigned int*>(ep.amax8);
        if (__float_as_uint(mx) > __builtin_nontemporal_load(slot)) atomicMax(slot, __float_as_uint(mx));
      }
    }
  }
#undef W8_H1
#undef W8_MORE2
}

// ---------------------------------------------------------------------------------
// fp8 NT kernel (BASELINE configs[3]: fp8 MFMA GEMMs): the eight-wave 256x256 kernel above with 8-bit operands on
// v_mfma_scale_f32_16x16x128_f8f6f4 (block scales fixed at 1: gfx950 has no unscaled K = 128 form; per-tensor scales are
// applied to the accumulators).  C (bf16) = epilogue(descale_a * descale_b * A8[M,K] x W8[N,K]^T).
// An LDS row is again 128 bytes - now 128 contraction elements - so staging, swizzle and fragment addresses are the
// bf16 kernel's; what was two 16-byte k-steps there is ONE MFMA operand here: lane group g = lane >> 4 holds the 16-byte
// chunks g and g + 4 of its row (the contraction order is permuted identically for both operands, which a sum does not
// see).  32 MFMAs of 32 clocks per K-tile and wave; quarters of 8 MFMAs (two A tiles x four W tiles) with the next
// quarter's A fragments - and, in the last quarter, the next K-tile's W fragments - fetched underneath: 96 fragment registers.
// A_BF8: the A operand is bf8 (e5m2, gradients); W is fp8 (e4m3) always.
// ---------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) int i32x4;
template <int EPI, bool A_BF8>
__global__ __launch_bounds__(512)
void gemm_nt_w8f8_kernel(const uint8_t* __restrict__ A, int lda, const uint8_t* __restrict__ W, int ldw,
                         bf16* __restrict__ C, int ldc, int M, int N, int K, M3PEpilogue ep,
                         int tiles_m, int tiles_n) {
  constexpr int BM = 256, BN = 256, NWAVES = 8, BK8 = 128;
  constexpr int A_BYTES = BM * ROWB, STAGE = (BM + BN) * ROWB;      // 32 KB, 64 KB
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ntiles = tiles_m * tiles_n;
  const int strip_w = strip_width(tiles_n, 12, 4);
  const int nwg = gridDim.x;
  const int slot = xcd_slot(nwg);
  auto tile_of = [&](int q) { return q * nwg + slot; };
  const int my_tiles = (ntiles > slot) ? (ntiles - slot + nwg - 1) / nwg : 0;
  if (my_tiles == 0) return;
  // the epilogue stages through the 32 KB beside the two stages, like the bf16 kernel (see there)
  constexpr bool kMulE = (EPI == M3P_EPI_DGELU || EPI == M3P_EPI_MUL);
  constexpr bool kAuxE = (EPI == M3P_EPI_BIAS_DROP_RES || EPI == M3P_EPI_RES || kMulE);
  constexpr bool kGqLut = (EPI == M3P_EPI_BIAS_GELUQ);
  constexpr int kTabBytes = (EPI == M3P_EPI_DGELU) ? GELU_TAB_N * (int)sizeof(float) : (kGqLut ? GQ_TAB_BYTES : 0);
  float* gtab = (EPI == M3P_EPI_DGELU) ? reinterpret_cast<float*>(smem + 2 * STAGE) : nullptr;
  if (EPI == M3P_EPI_DGELU) gelu_grad_table_fill(gtab, tid, 512);
  if (kGqLut) geluq_table_fill(reinterpret_cast<uint32_t*>(smem + 2 * STAGE), tid, 512);      // (the prologue's barrier publishes it)
  const int nk = K / BK8;
  const int total = my_tiles * nk;
  // per-tensor scales of the two operands (device scalars: delayed scaling keeps them on the device)
  const float dsc = (ep.descale_a ? *ep.descale_a : 1.f) * (ep.descale_b ? *ep.descale_b : 1.f);

  const int sr = lane >> 3, sc = (lane & 7) ^ sr;
  const uint8_t* a_src;
  const uint8_t* w_src;
  const size_t a_step = (size_t)64 * lda, w_step = (size_t)64 * ldw;
  int l_q = 0, l_kt = 0;
  auto set_load_tile = [&](int q) {
    int tm, tn;
    split_tile(tile_of(q), tiles_m, tiles_n, strip_w, tm, tn);
    a_src = A + (size_t)(tm * BM + wid * 8 + sr) * lda + sc * 16;
    w_src = W + (size_t)(tn * BN + wid * 8 + sr) * ldw + sc * 16;
  };
  auto issue_load = [&](int s, int piece) {
    char* sa = smem + s * STAGE;
    const int k0 = l_kt * BK8;
    if (piece < 4)
      __builtin_amdgcn_global_load_lds(GLB_PTR(a_src + piece * a_step + k0), LDS_PTR(sa + (wid + piece * NWAVES) * 1024), 16, 0, 0);
    else
      __builtin_amdgcn_global_load_lds(GLB_PTR(w_src + (piece - 4) * w_step + k0), LDS_PTR(sa + A_BYTES + (wid + (piece - 4) * NWAVES) * 1024), 16, 0, 0);
  };
  auto load_done = [&]() {
    if (++l_kt == nk) { l_kt = 0; ++l_q; if (l_q < my_tiles) set_load_tile(l_q); }
  };
  auto stage_next = [&](int s) {
#pragma unroll
    for (int pc = 0; pc < 8; ++pc) issue_load(s, pc);
    load_done();
  };

  const int wm = wid >> 2, wn = wid & 3;
  const int fr = lane & 15, fg = lane >> 4;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  uint32_t a_addr[2], b_addr[2];        // the two 16-byte chunks (fg, fg + 4) of this lane's row
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const int ch = ((fg + 4 * ks) ^ (fr & 7)) * 16;
    a_addr[ks] = lds0 + (wm * 128 + fr) * ROWB + ch;
    b_addr[ks] = lds0 + A_BYTES + (wn * 64 + fr) * ROWB + ch;
  }
  // an 8-register MFMA operand = two 16-byte LDS reads into the halves of one register tuple (plain loads: the
  // register allocator then places the halves adjacently; inline-asm reads into two 4-register values cost a copy each)
  typedef i32x8 Frag;
  auto frag = [&](uint32_t o0, uint32_t o1) {
    const i32x4 lo = *reinterpret_cast<const i32x4*>(smem + o0), hi = *reinterpret_cast<const i32x4*>(smem + o1);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  };
  auto read_w = [&](uint32_t so, Frag (&wf)[4]) {
    const uint32_t b0 = b_addr[0] - lds0 + so, b1 = b_addr[1] - lds0 + so;
#pragma unroll
    for (int j = 0; j < 4; ++j) wf[j] = frag(b0 + j * 2048, b1 + j * 2048);
  };
  auto read_a = [&](auto q_c, uint32_t so, Frag (&af)[2]) {       // A tiles 2q, 2q + 1
    constexpr int Q = decltype(q_c)::value;
    const uint32_t a0 = a_addr[0] - lds0 + so + Q * 4096, a1 = a_addr[1] - lds0 + so + Q * 4096;
    af[0] = frag(a0, a1);
    af[1] = frag(a0 + 2048, a1 + 2048);
  };

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // (ld_s, ld_p0, ld_n): LDS-DMA pieces issued in front of the cluster (spread over the quarters like the bf16 kernel)
  auto mfma_q = [&](auto q_c, const Frag (&af)[2], const Frag (&wf)[4]) {
    constexpr int I0 = 2 * decltype(q_c)::value;
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[I0 + i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[j], af[i], acc[I0 + i][j], 0, A_BF8 ? 1 : 0,
                                                                          0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
    __builtin_amdgcn_s_setprio(0);
  };
  using Q0 = std::integral_constant<int, 0>;
  using Q1 = std::integral_constant<int, 1>;
  using Q2 = std::integral_constant<int, 2>;
  using Q3 = std::integral_constant<int, 3>;

  set_load_tile(0);
  stage_next(0);
  if (total > 1) {
    stage_next(1);
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  Frag fa0[2], fa1[2], fw[4];
  read_w(0, fw);
  read_a(Q0{}, 0, fa0);
  M3P_WAIT_LGKM(0);
  int c_q = 0;
  const bool io_aligned = ((ldc & 7) == 0) && (((uintptr_t)C & 15) == 0) &&
                          (!ep.bias || (((uintptr_t)ep.bias & 15) == 0)) &&
                          (!ep.aux || (((ep.ld_aux & 7) == 0) && (((uintptr_t)ep.aux & 15) == 0)));
  f32x4 csum[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) csum[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  int csum_nw = -1;
  auto flush_csum = [&]() {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float sfl = csum[j][r];
        sfl += __shfl_xor(sfl, 1, 64); sfl += __shfl_xor(sfl, 2, 64);
        sfl += __shfl_xor(sfl, 4, 64); sfl += __shfl_xor(sfl, 8, 64);
        const int n = csum_nw + j * 16 + fg * 4 + r;
        if (fr == 0 && n < N) unsafeAtomicAdd(ep.colsum + n, sfl);
        csum[j][r] = 0.f;
      }
  };
  bool spread_pending = false;
  int step = 0;
  // One K-tile.  LAST (compile time): the output tile's last K-tile - no request for K-tile +2 and no fragment prefetch
  // (the epilogue stages through the vacated stage and wants the registers); peeling it keeps both bodies straight-line
  // code (a run-time condition around the prefetch makes phi copies of 48 fragment registers and lets MFMAs sink).
  auto ktile = [&](auto last_c) __attribute__((always_inline)) {
    constexpr bool LAST = decltype(last_c)::value;
    const int cur = step & 1, nxt = cur ^ 1;
    const bool more2 = (step + 2 < total);
    const uint32_t so = cur * STAGE;
    const bool pend = spread_pending;
    if (pend) { issue_load(nxt, 3); issue_load(nxt, 4); issue_load(nxt, 5); }
    read_a(Q1{}, so, fa1);
    __builtin_amdgcn_sched_barrier(0);
    mfma_q(Q0{}, fa0, fw);
    M3P_WAIT_LGKM(0);
    if (pend) { issue_load(nxt, 6); issue_load(nxt, 7); load_done(); spread_pending = false; }
    read_a(Q2{}, so, fa0);
    __builtin_amdgcn_sched_barrier(0);
    mfma_q(Q1{}, fa1, fw);
    M3P_WAIT_LGKM(0);
    read_a(Q3{}, so, fa1);
    __builtin_amdgcn_sched_barrier(0);
    mfma_q(Q2{}, fa0, fw);
    M3P_WAIT_LGKM(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (!LAST || !kAuxE) {
      if (more2) { issue_load(cur, 0); issue_load(cur, 1); issue_load(cur, 2); spread_pending = true; }
    }
    if (!LAST) read_a(Q0{}, nxt * STAGE, fa0);           // (stale bytes after the very last K-tile: never used)
    __builtin_amdgcn_sched_barrier(0);
    // last quarter W-tile-major: the W fragments are single-buffered (a second set of 32 registers does not exist
    // beside 128 accumulators), so W tile j of the next K-tile is fetched as soon as the two MFMAs that read tile j
    // have been issued
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc[6][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw[j], fa1[0], acc[6][j], 0, A_BF8 ? 1 : 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
      acc[7][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw[j], fa1[1], acc[7][j], 0, A_BF8 ? 1 : 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
      if (!LAST) {
        const uint32_t b0 = b_addr[0] - lds0 + nxt * STAGE + j * 2048, b1 = b_addr[1] - lds0 + nxt * STAGE + j * 2048;
        fw[j] = frag(b0, b1);
      }
    }
    __builtin_amdgcn_s_setprio(0);
    M3P_WAIT_LGKM(0);
    ++step;
  };
  for (int tq = 0; tq < my_tiles; ++tq) {
    for (int kt = 0; kt + 1 < nk; ++kt) ktile(std::false_type{});
    ktile(std::true_type{});
    {
      const int cur = (step - 1) & 1, nxt = cur ^ 1;
      const bool more2 = (step + 1 < total);       // (step was advanced past the tile's last K-tile)
      const bool more1 = (step < total);
      const int t = tile_of(c_q);
      ++c_q;
      int tm, tn;
      split_tile(t, tiles_m, tiles_n, strip_w, tm, tn);
      const int m0 = tm * BM, n0 = tn * BN;
      const int mw = m0 + wm * 128, nw = n0 + wn * 64;
      if ((EPI == M3P_EPI_DGELU || EPI == M3P_EPI_MUL) && ep.colsum && csum_nw != nw) {
        if (csum_nw >= 0) flush_csum();
        csum_nw = nw;
      }
      const bool fast = io_aligned && (m0 + BM <= M) && (n0 + BN <= N);
      if (fast && kMulE) {
        char* r1 = smem + 2 * STAGE + kTabBytes + wid * 2048;
        u32x4 ta[2], tb[2];
        aux16_issue(ep, mw, nw, lane, ta);
        __builtin_amdgcn_sched_barrier(0);
        if (more2) { issue_load(cur, 0); issue_load(cur, 1); issue_load(cur, 2); spread_pending = true; }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int hp = 0; hp < 8; hp += 2) {
          f32x4 rows[4];
          aux16_issue(ep, mw + 16 * (hp + 1), nw, lane, tb);
#pragma unroll
          for (int j = 0; j < 4; ++j) rows[j] = acc[hp][j] * dsc;
          epilogue_piece16<EPI>(ep, C, ldc, mw + 16 * hp, nw, r1, rows, ta, lane, csum, gtab);
          __builtin_amdgcn_sched_barrier(0);
          if (hp + 2 < 8) aux16_issue(ep, mw + 16 * (hp + 2), nw, lane, ta);
#pragma unroll
          for (int j = 0; j < 4; ++j) rows[j] = acc[hp + 1][j] * dsc;
          epilogue_piece16<EPI>(ep, C, ldc, mw + 16 * (hp + 1), nw, r1, rows, tb, lane, csum, gtab);
          __builtin_amdgcn_sched_barrier(0);
        }
      } else if (fast) {
        char* r1 = smem + 2 * STAGE + wid * 4096;
        f32x4 biasv[4];
        load_bias4<EPI>(ep, nw, lane, biasv);
        u32x4 aux0[4];
        if (kAuxE) {
          load_aux_rows_issue<EPI>(ep, mw, nw, lane, aux0);
          __builtin_amdgcn_sched_barrier(0);
          if (more2) { issue_load(cur, 0); issue_load(cur, 1); issue_load(cur, 2); spread_pending = true; }
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int hf = 0; hf < 4; ++hf) {
          f32x4 rows[2][4];
#pragma unroll
          for (int ii = 0; ii < 2; ++ii)
#pragma unroll
            for (int j = 0; j < 4; ++j) rows[ii][j] = acc[2 * hf + ii][j] * dsc;
          bf16x4 auxv[2][4];
          if (kAuxE && hf == 0) load_aux_rows_finish<EPI, true>(lane, r1, aux0, auxv);
          else load_aux_rows<EPI, true>(ep, mw + 32 * hf, nw, lane, r1, auxv);
          epilogue_half<EPI, true>(ep, C, ldc, N, mw + 32 * hf, nw, r1, rows, biasv, auxv, lane, csum, gtab);
          __builtin_amdgcn_sched_barrier(0);
        }
      } else {
        if (kAuxE && more2) { issue_load(cur, 0); issue_load(cur, 1); issue_load(cur, 2); spread_pending = true; }
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            epilogue_store<EPI>(ep, C, ldc, M, N, mw + i * 16 + fr, nw + j * 16 + fg * 4, acc[i][j] * dsc, csum[j]);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (more1) {
        read_w(nxt * STAGE, fw);
        read_a(Q0{}, nxt * STAGE, fa0);
        M3P_WAIT_LGKM(0);
      }
    }
  }
  if ((EPI == M3P_EPI_DGELU || EPI == M3P_EPI_MUL) && ep.colsum && csum_nw >= 0) flush_csum();
}


struct WgCursor {
  int c, t, mt, len;   // chunk, tile, K-tile inside the chunk, K-tiles in this chunk
};
// second product of a paired weight-gradient launch (tiles_i * tiles_j == 0: none)
struct WgradProblem {
  const bf16* dY; const bf16* X; float* dW;
  int lddy, ldx, lddw, tiles_i, tiles_j;
};
// the products and the placement of a grouped whole-tile launch, passed by kernel argument (1.5 KB): workgroup w computes tile
// (place[w] >> 8 & 255, place[w] & 255) of item place[w] >> 16; 0xffffffff = nothing (wgrad_group_place)
struct WgradGroup {
  struct Item {
    const bf16* dY; const bf16* X; float* dW;
    int lddy, ldx, lddw, tiles_j;
  } item[M3P_WGRAD_GROUP_MAX];
  uint32_t place[256];
};
__device__ __forceinline__ const WgradGroup& wgrad_group_of(const WgradGroup& g) { return g; }      // (the kernel's trailing pack)
// bias sums of a whole-tile launch (m3p_gemm_wgrad_bias_bf16): bsum[i] = sum_m w[m] dY[m, i], w fp32 [M], bsum fp32 [N]
struct WgradBias {
  const float* w; float* bsum;
};
__device__ __forceinline__ const WgradBias& wgrad_bias_of(const WgradBias& b) { return b; }

// ---------------------------------------------------------------------------------
// NT kernel, stream-K version with fp32 atomic output: Cf[M,N] += alpha * A[M,K] W[N,K]^T for
// few-tile / very-long-K problems (the data gradient of the vocabulary projection:
// M = n_pred = 4864, N = 768, K = V_pad = 250 048 -> only 114 tiles of 256x128 but 3907
// K-tiles each).  The (k-chunk, tile, K-tile) stream is dealt out exactly like the
// weight-gradient kernel's: chunk = one workgroup's share, so all 256 CUs are busy and the six
// N-tiles that share an A panel walk the same K range at the same time (A — the 2.4 GB
// dlogits — is then read from HBM once instead of six times).  Same ring pipeline as
// gemm_nt_ring_kernel; partial tiles are flushed with fp32 atomics.
// ---------------------------------------------------------------------------------
// W_KN: the second operand is given as W[K, N] (row = contraction index, N contiguous) instead of
// W[N, K]: its 64 x 128 tile is staged with 256-B rows and read through ds_read_b64_tr_b16 like the X
// operand of the weight-gradient kernel, so the vocabulary data gradient dH = dlogits . E reads the
// embedding matrix as it is (no transposed copy; rows >= k_valid - the padding of V - are clamped:
// their dlogits columns are exact zeros).
template <bool W_KN>
__global__ __launch_bounds__(512)
void gemm_nt_streamk_kernel(const bf16* __restrict__ A, int lda, const bf16* __restrict__ W, int ldw,
                            float* __restrict__ Cf, int ldc, int M, int N, int K, float alpha,
                            int tiles_m, int tiles_n, int CHUNK, int k_valid) {
  constexpr int BM = 256, BN = 128, NWAVES = 8;
  constexpr int A_BYTES = BM * ROWB, B_BYTES = BN * ROWB, STAGE = A_BYTES + B_BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ntile = tiles_m * tiles_n;
  const int nk = K / BK;
  const long long total_all = (long long)ntile * nk;
  const int nwg = gridDim.x;
  const int slot = xcd_slot(nwg);
  const long long share = (total_all + nwg - 1) / nwg;
  const long long g0l = share * slot;
  if (g0l >= total_all) return;
  const int total = (int)((g0l + share <= total_all ? g0l + share : total_all) - g0l);

  auto locate = [&](long long g) {
    WgCursor cu;
    const long long full = (long long)ntile * CHUNK;
    cu.c = (int)(g / full);
    const int rem = (int)(g - cu.c * full);
    cu.len = min(CHUNK, nk - cu.c * CHUNK);
    cu.t = rem / cu.len;
    cu.mt = rem - cu.t * cu.len;
    return cu;
  };
  auto advance = [&](WgCursor& cu) {
    if (++cu.mt == cu.len) {
      cu.mt = 0;
      if (++cu.t == ntile) { cu.t = 0; ++cu.c; cu.len = min(CHUNK, nk - cu.c * CHUNK); }
    }
  };

  const int sr = lane >> 3, sc = (lane & 7) ^ sr;
  WgCursor lc = locate(g0l);
  auto stage_next = [&](int s) {
    char* sa = smem + s * STAGE;
    char* sb = sa + A_BYTES;
    const int tm = lc.t / tiles_n, tn = lc.t - tm * tiles_n;
    const int k0 = (lc.c * CHUNK + lc.mt) * BK + sc * 8;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = min(tm * BM + (wid + i * NWAVES) * 8 + sr, M - 1);
      __builtin_amdgcn_global_load_lds(GLB_PTR(A + (size_t)row * lda + k0), LDS_PTR(sa + (wid + i * NWAVES) * 1024), 16, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (W_KN) {
        const int rb = wid + i * NWAVES;            // 4-row group of the 64 x 128 tile
        const int row = rb * 4 + (lane >> 4);
        const int f = (row & 3) | (((row >> 3) & 1) << 2);
        const int gc = (lane & 15) ^ (f << 1);
        const int col = min(tn * (BN / 8) + gc, (N + 7) / 8 - 1) * 8;
        const int krow = min((lc.c * CHUNK + lc.mt) * BK + row, k_valid - 1);
        __builtin_amdgcn_global_load_lds(GLB_PTR(W + (size_t)krow * ldw + col), LDS_PTR(sb + rb * 1024), 16, 0, 0);
      } else {
        const int row = min(tn * BN + (wid + i * NWAVES) * 8 + sr, N - 1);
        __builtin_amdgcn_global_load_lds(GLB_PTR(W + (size_t)row * ldw + k0), LDS_PTR(sb + (wid + i * NWAVES) * 1024), 16, 0, 0);
      }
    }
    advance(lc);
  };

  const int wm = wid >> 1, wn = wid & 1;
  const int fr = lane & 15, fg = lane >> 4;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  uint32_t a_addr[2], b_addr[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const int ch = ((fg + 4 * ks) ^ (fr & 7)) * 16;
    a_addr[ks] = lds0 + (wm * 64 + fr) * ROWB + ch;
    b_addr[ks] = lds0 + A_BYTES + (wn * 64 + fr) * ROWB + ch;
  }
  // W_KN fragments: tr16 addressing of the weight-gradient kernel's X operand (256-B rows)
  const int t_row = fg * 8 + (fr >> 2);
  const int t_sw = ((fr >> 2) | ((fg & 1) << 2)) << 1;
  uint32_t x_addr[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int qx = wn * 8 + 2 * c + ((fr & 3) >> 1);
    x_addr[c] = lds0 + A_BYTES + t_row * 256 + ((qx ^ t_sw) << 4) + ((fr & 1) << 3);
  }
  // ks = 0 / 1 selects the 32-deep k-step; so = byte offset of the stage
  auto read_set = [&](int ks, uint32_t so, bf16x8 (&af)[4], bf16x8 (&wf)[4], s16x4 (&wh)[4][2]) {
    const uint32_t aa = a_addr[ks] + so, ba = b_addr[ks] + so;
    if (W_KN) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (ks == 0) { M3P_TR(wh[c][0], x_addr[c] + so, 0); M3P_TR(wh[c][1], x_addr[c] + so, 1024); }
        else { M3P_TR(wh[c][0], x_addr[c] + so, 8192); M3P_TR(wh[c][1], x_addr[c] + so, 9216); }
      }
    } else {
      M3P_DSR(wf[0], ba, 0); M3P_DSR(wf[1], ba, 2048); M3P_DSR(wf[2], ba, 4096); M3P_DSR(wf[3], ba, 6144);
    }
    M3P_DSR(af[0], aa, 0); M3P_DSR(af[1], aa, 2048); M3P_DSR(af[2], aa, 4096); M3P_DSR(af[3], aa, 6144);
  };
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto mfma_batch = [&](const bf16x8 (&af)[4], const bf16x8 (&wf_in)[4], const s16x4 (&wh)[4][2]) {
    bf16x8 wf[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      wf[j] = W_KN ? __builtin_bit_cast(bf16x8, __builtin_shufflevector(wh[j][0], wh[j][1], 0, 1, 2, 3, 4, 5, 6, 7)) : wf_in[j];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], af[i], acc[i][j], 0, 0, 0);
  };

  stage_next(0);
  if (total > 1) {
    stage_next(1);
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  bf16x8 af0[4], wf0[4], af1[4], wf1[4];
  s16x4 wh0[4][2], wh1[4][2];
  read_set(0, 0, af0, wf0, wh0);
  M3P_WAIT_LGKM(0);
  WgCursor cc = locate(g0l);
  int cur = 0;
  for (int step = 0; step < total; ++step) {
    const int nxt = (cur == 2) ? 0 : cur + 1;
    const int nx2 = (nxt == 2) ? 0 : nxt + 1;
    const bool more2 = (step + 2 < total);
    if (more2) stage_next(nx2);
    read_set(1, cur * STAGE, af1, wf1, wh1);
    __builtin_amdgcn_sched_barrier(0);
    mfma_batch(af0, wf0, wh0);
    M3P_WAIT_LGKM(0);
    if (more2) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    read_set(0, nxt * STAGE, af0, wf0, wh0);
    __builtin_amdgcn_sched_barrier(0);
    mfma_batch(af1, wf1, wh1);
    M3P_WAIT_LGKM(0);
    if ((cc.mt + 1 == cc.len) || (step + 1 == total)) {
      const int tm = cc.t / tiles_n, tn = cc.t - tm * tiles_n;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = tm * BM + wm * 64 + i * 16 + fr;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int n = tn * BN + wn * 64 + j * 16 + fg * 4;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (m < M && n + r < N) unsafeAtomicAdd(Cf + (size_t)m * ldc + n + r, alpha * acc[i][j][r]);
            acc[i][j][r] = 0.f;
          }
        }
      }
    }
    advance(cc);
    cur = nxt;
  }
}

#include "gemm_nt_w4.hpp"

// ---------------------------------------------------------------------------------
// NT kernel for a handful of rows (M <= 128: one decoding step of the causal decoder, heads on a batch of [CLS] rows):
// latency / HBM work - every weight row is read once, straight from global memory into the MFMA operand registers (a
// lane's 16-byte fragment is 8 consecutive contraction elements of one W row), no LDS staging, no persistent schedule.
// SPLITK: a workgroup owns 16 output columns and its four waves a quarter of the contraction each (small N: 48
// workgroups x 4 waves for N = 768 instead of 12), partial sums folded through LDS.  Otherwise a workgroup owns 64
// columns, one wave per 16 (the vocabulary projection: N = 250 002).  Epilogues as everywhere (epilogue_store).
// ---------------------------------------------------------------------------------
template <int EPI, int MT, bool SPLITK>
__global__ __launch_bounds__(256)
void gemm_nt_skinny_kernel(const bf16* __restrict__ A, int lda, const bf16* __restrict__ W, int ldw,
                           bf16* __restrict__ C, int ldc, int M, int N, int K, M3PEpilogue ep) {
  __shared__ f32x4 red[SPLITK ? 3 : 1][MT][64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int n0 = SPLITK ? blockIdx.x * 16 : (blockIdx.x * 4 + wid) * 16;
  const int klen = SPLITK ? K / 4 : K;
  const int kbeg = SPLITK ? wid * klen : 0;
  if (!SPLITK && n0 >= N) return;
  const bf16* wp = W + (size_t)min(n0 + fr, N - 1) * ldw + kbeg + fg * 8;
  const bf16* ap[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) ap[i] = A + (size_t)min(i * 16 + fr, M - 1) * lda + kbeg + fg * 8;
  f32x4 acc[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int k = 0; k < klen; k += 32) {
    const bf16x8 wf = *reinterpret_cast<const bf16x8*>(wp + k);
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const bf16x8 af = *reinterpret_cast<const bf16x8*>(ap[i] + k);
      acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, af, acc[i], 0, 0, 0);
    }
  }
  if (SPLITK) {
    if (wid > 0) {
#pragma unroll
      for (int i = 0; i < MT; ++i) red[wid - 1][i][lane] = acc[i];
    }
    __syncthreads();
    if (wid > 0) return;
#pragma unroll
    for (int i = 0; i < MT; ++i) acc[i] += red[0][i][lane] + red[1][i][lane] + red[2][i][lane];
  }
  f32x4 unused = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < MT; ++i) epilogue_store<EPI>(ep, C, ldc, M, N, i * 16 + fr, n0 + fg * 4, acc[i], unused);
}

template <int EPI, int MT>
int launch_nt_skinny(const bf16* A, int lda, const bf16* W, int ldw, bf16* C, int ldc, int M, int N, int K,
                     const M3PEpilogue& ep, hipStream_t st) {
  if (N <= 8192)
    hipLaunchKernelGGL((gemm_nt_skinny_kernel<EPI, MT, true>), dim3((N + 15) / 16), dim3(256), 0, st, A, lda, W, ldw, C, ldc, M, N, K, ep);
  else
    hipLaunchKernelGGL((gemm_nt_skinny_kernel<EPI, MT, false>), dim3((N + 63) / 64), dim3(256), 0, st, A, lda, W, ldw, C, ldc, M, N, K, ep);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

static int hw_cus() {
  static int n = 0;
  if (n == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n = prop.multiProcessorCount;
    if (n <= 0) n = 256;
    n -= n % 8;   // the persistent schedule deals tiles out per XCD
    if (n <= 0) n = 8;
  }
  return n;
}
// workgroups of a persistent grid: one per CU, or what m3p_set_persistent_grid left of them (data parallelism: RCCL's
// kernels need CUs of their own - a persistent GEMM workgroup fills its CU's LDS, nothing can co-reside with it)
static int g_persistent_grid = 0;
static int num_cus() {
  const int hw = hw_cus();
  return (g_persistent_grid > 0 && g_persistent_grid < hw) ? g_persistent_grid : hw;
}
// ... for a launch over ntiles output tiles: fewer tiles than CUs -> one workgroup per tile, rounded up to whole XCD rounds
static int persistent_grid(int ntiles) {
  const int grid = num_cus();
  return ntiles < grid ? (ntiles + 7) / 8 * 8 : grid;
}
// Raises a kernel's dynamic-LDS limit in front of its first launch; 0 or the HIP error.  The flag is per kernel symbol, so
// `lds` must be a function of the kernel's template arguments alone (every launcher's is).
template <auto Kern>
int set_max_lds(size_t lds) {
  static bool done = false;      // (set on success only: a failed call is tried again by the next launch, as before)
  if (!done) {
    hipError_t e = hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    done = true;
  }
  return M3P_OK;
}

// dynamic tile queues of the eight-wave kernel (m3p_set_tile_queue): a ring of 8-counter slots, one slot per launch
// The ring belongs to ONE stream - the first one a queued launch arrives on after m3p_set_tile_queue (slots are cleared by a
// memset on that stream, behind everything it has launched): a launch on any other stream takes the static schedule, so a
// slot is never handed out while a kernel of another stream may still be popping from it.  Slot hand-out is under a mutex
// (forward launches from the Python thread, backward from the autograd thread; ctypes drops the GIL around the calls).
static int* g_tq_pool = nullptr;
static int g_tq_slots = 0, g_tq_next = 0;
static hipStream_t g_tq_stream = nullptr;
static bool g_tq_bound = false;
static std::mutex g_tq_mu;
// -> counters of a fresh slot, or nullptr (no queue / foreign stream / memset failed: *err set)
static int* tq_acquire(hipStream_t st, hipError_t* err) {
  *err = hipSuccess;
  std::lock_guard<std::mutex> lk(g_tq_mu);
  if (!g_tq_pool) return nullptr;
  if (!g_tq_bound) { g_tq_stream = st; g_tq_bound = true; }
  if (st != g_tq_stream) return nullptr;
  if (g_tq_next == g_tq_slots) {       // ring used up: clear it behind everything this stream has launched so far
    *err = hipMemsetAsync(g_tq_pool, 0, (size_t)g_tq_slots * 8 * sizeof(int), st);
    if (*err != hipSuccess) return nullptr;
    g_tq_next = 0;
  }
  return g_tq_pool + 8 * g_tq_next++;
}

// the four-wave kernel takes contractions from this depth on (table below); the eight-wave kernel has no limit on the size of
// W (the vocabulary projection - W = 384 MB - measured 2.18 -> 1.85 ms on it)
constexpr int W4_MIN_K = 2048;
static bool tq_enabled() {
  std::lock_guard<std::mutex> lk(g_tq_mu);
  return g_tq_pool != nullptr;
}

// ---------------------------------------------------------------------------------------------------------------------
// WHICH KERNEL RUNS AN NT PRODUCT - the one place that decides (m3p_gemm_nt_plan reports it; launch_nt switches on it).
// Rows are tried top to bottom; "whole tiles" = M >= 1024, M % 256 == 0, N % 256 == 0, N >= 512, K % 64 == 0 (the entry point has
// already checked K % 64, lda / ldw % 8 and 16-byte operand bases).
//
//   shape / epilogue                                      kernel                     why (measured where)
//   ----------------------------------------------------  -------------------------  -------------------------------------------------
//   MULQ / BIAS_GELUQ / BIAS_LSE (whole tiles only,       eight-wave 256x256         their byte / statistics layouts ARE that kernel's
//     anything else -> M3P_EINVAL)                                                     (tile, wave, row block, lane) order
//   M <= 128, K % 128 == 0, not DGELU / MUL               skinny (no LDS)            one decoding step / [CLS] rows: every W row read once
//   whole tiles, K >= 2048, not DGELU / MUL,              four-wave 256x256          K-tile in one piece, buffer-form transfers: dx1 159 vs
//     no tile queue armed                                                              174 us, dh 125 vs 131, lin2 fwd 169 vs 177 (round 4)
//   whole tiles (any K)                                   eight-wave 256x256         second wave per SIMD hides epilogue + LDS-DMA issue:
//     + tile queue armed, > 1 tile per workgroup,           (queue instantiation)      q/k/v 137 vs 148 us at K = 768; vocabulary projection
//       K >= 512, not DGELU / MUL                                                      1.85 vs 2.18 ms
//   M >= 1024 otherwise (ragged M or N, N < 512)          ring 256x128, 3 stages     any shape; strip order for the vocabulary matrices
//   M < 1024                                              128x128, 2 stages          small-M fallback (cfg1, tests)
//
// Developer overrides (m3p_debug_set_variant, never set by the product): 2 forces the four-wave kernel wherever it applies,
// 6 the eight-wave kernel.
// ---------------------------------------------------------------------------------------------------------------------
static int nt_plan(int epi, int M, int N, int K, int* queue) {
  if (queue) *queue = 0;
  const bool whole = M >= 1024 && (M % 256) == 0 && (N % 256) == 0 && N >= 512 && (K % 64) == 0;
  if (epi == M3P_EPI_MULQ || epi == M3P_EPI_BIAS_GELUQ || epi == M3P_EPI_BIAS_LSE) return whole ? M3P_KERN_NT_W8 : M3P_EINVAL;
  const bool mul_epi = epi == M3P_EPI_DGELU || epi == M3P_EPI_MUL;
  if (M <= 128 && (K % 128) == 0 && !mul_epi) return M3P_KERN_NT_SKINNY;
  // (dGELU epilogue on the four-wave kernel: 240 VGPRs, measured slower in the step)
  const bool deep = N >= 512 && 2LL * N * K <= (64LL << 20) && epi != M3P_EPI_DGELU;
  const bool armed = tq_enabled();     // (the tile queue of data parallelism lives in the eight-wave kernel)
  const bool w4_first = g_variant == 1 && deep && K >= W4_MIN_K && epi != M3P_EPI_MUL && !armed;
  if (whole && g_variant != 2 && !w4_first) {
    // dynamic tile queue only where a workgroup takes several tiles (not for the multiply epilogues: with the queue's
    // bookkeeping on top of their aux pieces and column sums the instantiation spills ~100 bytes per lane)
    const int ntiles = (M / 256) * (N / 256);
    if (queue) *queue = (!mul_epi && armed && ntiles > persistent_grid(ntiles) && K >= 8 * BK) ? 1 : 0;
    return M3P_KERN_NT_W8;
  }
  if (M >= 1024 && (M % 256) == 0 && (N % 256) == 0 && (g_variant == 2 || (g_variant == 1 && deep)))
    return M3P_KERN_NT_W4;
  if (M >= 1024) return M3P_KERN_NT_RING;
  return M3P_KERN_NT_128;
}

template <int EPI>
int launch_nt(const bf16* A, int lda, const bf16* W, int ldw, bf16* C, int ldc, int M, int N, int K,
              const M3PEpilogue& ep, hipStream_t st) {
  int want_queue = 0;
  const int plan = nt_plan(EPI, M, N, K, &want_queue);
  if (plan == M3P_KERN_NT_SKINNY) {
    if constexpr (EPI != M3P_EPI_DGELU && EPI != M3P_EPI_MUL) {
      if (M <= 16) return launch_nt_skinny<EPI, 1>(A, lda, W, ldw, C, ldc, M, N, K, ep, st);
      if (M <= 32) return launch_nt_skinny<EPI, 2>(A, lda, W, ldw, C, ldc, M, N, K, ep, st);
      if (M <= 64) return launch_nt_skinny<EPI, 4>(A, lda, W, ldw, C, ldc, M, N, K, ep, st);
      return launch_nt_skinny<EPI, 8>(A, lda, W, ldw, C, ldc, M, N, K, ep, st);
    }
  }
  if (plan == M3P_KERN_NT_W8) {
    const int tiles_m = M / 256, tiles_n = N / 256;
    const size_t lds = 2 * 512 * ROWB + (EPI == M3P_EPI_DGELU ? GELU_TAB_N * sizeof(float) : 0) +
                       ((EPI == M3P_EPI_DGELU || EPI == M3P_EPI_MUL) ? 8 * 2048 : 8 * 4096);
    constexpr auto kern = gemm_nt_w8_kernel<EPI>;
    if (int rc = set_max_lds<kern>(lds)) return rc;
    const int grid = persistent_grid(tiles_m * tiles_n);
    // dynamic tile queue (ep.tile_ctr: eight zeroed counters, one per XCD) only where a workgroup takes several tiles
    // (not for the multiply epilogues: with the queue's bookkeeping on top of their aux pieces and column sums the instantiation
    //  spills ~100 bytes per lane - 0.31 against 0.28 ms on the dGELU product, more than the queue returns on 12 launches a step)
    constexpr bool kQueueOk = !(EPI == M3P_EPI_DGELU || EPI == M3P_EPI_MUL);
    int* ctr = nullptr;
    if (kQueueOk && want_queue) {
      hipError_t e;
      ctr = tq_acquire(st, &e);
      if (e != hipSuccess) return (int)e;
    }
    if constexpr (kQueueOk) if (ctr) {
      constexpr auto kern_d = gemm_nt_w8_kernel<EPI, true>;
      if (int rc = set_max_lds<kern_d>(lds)) return rc;
      hipLaunchKernelGGL(kern_d, dim3(grid), dim3(512), lds, st, A, lda, W, ldw, C, ldc, M, N, K, ep, tiles_m, tiles_n, ctr);
      M3P_CHECK_LAUNCH();
      return M3P_OK;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, st, A, lda, W, ldw, C, ldc, M, N, K, ep, tiles_m, tiles_n, ctr);
    M3P_CHECK_LAUNCH();
    return M3P_OK;
  }
  if (plan == M3P_KERN_NT_W4) {
    constexpr int BM = 256, BN = 256;
    const int tiles_m = (M + BM - 1) / BM, tiles_n = (N + BN - 1) / BN;
    const size_t lds = 2 * (BM + BN) * 128 + 4 * EP_HALF;
    // (a BIAS_DROP_RES launch with a row map runs the instantiation that looks the map up; every other launch compiles it out)
    const bool rows = (EPI == M3P_EPI_BIAS_DROP_RES && ep.rng_rows != nullptr);
    constexpr auto kern_rows = gemm_nt_w4_kernel<(EPI == M3P_EPI_BIAS_DROP_RES ? M3P_EPI_DROP_RES_ROWS : EPI)>, kern_plain = gemm_nt_w4_kernel<EPI>;
    if (int rc = rows ? set_max_lds<kern_rows>(lds) : set_max_lds<kern_plain>(lds)) return rc;
    auto kern = rows ? kern_rows : kern_plain;
    const int grid = persistent_grid(tiles_m * tiles_n);
    const long long wbytes = 2LL * N * K, abytes = 2LL * M * K;
    const int m_fast = (wbytes > (64LL << 20) && abytes < wbytes) ? 1 : 0;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, st, A, lda, W, ldw, C, ldc, M, N, K, ep, tiles_m, tiles_n, m_fast);
    M3P_CHECK_LAUNCH();
    return M3P_OK;
  }
  if (plan == M3P_KERN_NT_RING) {
    constexpr int BM = 256, BN = 128;
    const int tiles_m = (M + BM - 1) / BM, tiles_n = (N + BN - 1) / BN;
    const size_t lds = 3 * (BM + BN) * ROWB + (EPI == M3P_EPI_DGELU ? GELU_TAB_N * sizeof(float) : 0);
    constexpr auto kern = gemm_nt_ring_kernel<EPI>;
    if (int rc = set_max_lds<kern>(lds)) return rc;
    const int grid = persistent_grid(tiles_m * tiles_n);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, st, A, lda, W, ldw, C, ldc, M, N, K, ep, tiles_m, tiles_n);
    M3P_CHECK_LAUNCH();
    return M3P_OK;
  }
  constexpr int BM = 128, BN = 128;
  const int tiles_m = (M + BM - 1) / BM, tiles_n = (N + BN - 1) / BN;
  const size_t lds = 2 * (BM + BN) * ROWB;
  constexpr auto kern = gemm_nt_kernel<BM, BN, EPI>;
  if (int rc = set_max_lds<kern>(lds)) return rc;
  hipLaunchKernelGGL(kern, dim3(tiles_m * tiles_n), dim3(256), lds, st, A, lda, W, ldw, C, ldc, M, N, K, ep,
                     tiles_m, tiles_n);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

// M3P_EPI_MULQ: the byte-derivative epilogue exists on the eight-wave kernel only (its aux layout IS that kernel's tiling)
// M3P_EPI_BIAS_GELUQ: likewise (it writes that layout); M3P_EPI_BIAS_LSE: its statistics are per 64-column wave block
template <int EPI>
static int launch_nt_gq(const bf16* A, int lda, const bf16* W, int ldw, bf16* C, int ldc, int M, int N, int K,
                        const M3PEpilogue& ep, hipStream_t st) {
  if (M < 1024 || (M % 256) || (N % 256) || N < 512 || (K % 64) || (lda % 8) || (ldw % 8) || (ldc % 8) || ((uintptr_t)C & 15))
    return M3P_EINVAL;
  if (EPI == M3P_EPI_MULQ && (!ep.aux || ((uintptr_t)ep.aux & 15))) return M3P_EINVAL;
  constexpr bool kLse = (EPI == M3P_EPI_BIAS_LSE || EPI == M3P_EPI_BIAS_EXP);
  if ((EPI == M3P_EPI_BIAS_GELUQ || kLse) && (!ep.out2 || ((uintptr_t)ep.out2 & 15) || !ep.bias || ((uintptr_t)ep.bias & 15)))
    return M3P_EINVAL;
  if (kLse && (ep.ld_out2 <= 0 || ep.ld_out2 > N)) return M3P_EINVAL;
  if (EPI == M3P_EPI_BIAS_EXP && (!ep.row_ref || ((uintptr_t)ep.row_ref & 7))) return M3P_EINVAL;
  const int tiles_m = M / 256, tiles_n = N / 256;
  const size_t lds = 2 * 512 * ROWB + ((EPI == M3P_EPI_BIAS_GELUQ) ? GQ_TAB_BYTES + 8 * 2048 + 8 * 1024 : 8 * (EPI != M3P_EPI_MULQ ? 4096 : 2048)) +
                     (EPI == M3P_EPI_MULQ ? 2048 + 8 * 1024 : 0);      // (MULQ: behind the staging rows 2 KB - the 8-bit copy's running maxima / the
                                                                       //  prefetch experiment - and the 8-bit copy's own staging rows, 1 KB per wave)
  const int grid = persistent_grid(tiles_m * tiles_n);
  if constexpr (EPI == M3P_EPI_BIAS_GELUQ || EPI == M3P_EPI_MULQ) {
    if (ep.out8) {      // the instantiation that also leaves the 8-bit copy (its own registers: the plain one must not pay for it)
      if (((uintptr_t)ep.out8 & 15) || (ep.ld_out8 & 15) || ep.ld_out8 < N || !ep.scale8 || !ep.amax8) return M3P_EINVAL;
      // the copy of an activation is e4m3, of a gradient e5m2 - what the fp8 product's operand slots take (include/m3p_hip.h)
      if ((EPI == M3P_EPI_MULQ) != (ep.out8_bf8 != 0)) return M3P_EINVAL;
      constexpr auto kern8 = gemm_nt_w8_kernel<EPI, false, true>;
      if (int rc = set_max_lds<kern8>(lds)) return rc;
      hipLaunchKernelGGL(kern8, dim3(grid), dim3(512), lds, st, A, lda, W, ldw, C, ldc, M, N, K, ep, tiles_m, tiles_n, (int*)nullptr);
      M3P_CHECK_LAUNCH();
      return M3P_OK;
    }
  }
  constexpr auto kern = gemm_nt_w8_kernel<EPI>;
  if (int rc = set_max_lds<kern>(lds)) return rc;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, st, A, lda, W, ldw, C, ldc, M, N, K, ep, tiles_m, tiles_n, (int*)nullptr);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

// ---------------------------------------------------------------------------------
// weight-gradient kernel: dW[i,j] += alpha * sum_m dY[m,i] X[m,j]
// LDS tiles are [64 m][128 cols] bf16 (256-B rows, as in HBM); MFMA operands need 8
// consecutive m per lane for one column -> two ds_read_b64_tr_b16 per fragment.
// ---------------------------------------------------------------------------------
constexpr int WG_T = 128;           // output tile edge
constexpr int WG_ROWB = WG_T * 2;   // 256 B per LDS row
constexpr int WG_TILE_BYTES = BK * WG_ROWB;  // 16 KB

__device__ __forceinline__ bf16x4 lds_tr16(const char* p) {
  s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(p));
  return __builtin_bit_cast(bf16x4, v);
}

__global__ __launch_bounds__(256)
void gemm_wgrad_kernel(const bf16* __restrict__ dY, int lddy, const bf16* __restrict__ X, int ldx,
                       float* __restrict__ dW, int lddw, int M, int N, int K, float alpha,
                       int tiles_i, int tiles_j, int m_chunk) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ntile = tiles_i * tiles_j;
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int split = id / ntile, tile = id - split * ntile;
  const int ti = tile / tiles_j, tj = tile - ti * tiles_j;
  const int i0 = ti * WG_T, j0 = tj * WG_T;
  const int m_begin = split * m_chunk;
  const int m_end = min(M, m_begin + m_chunk);
  if (m_begin >= m_end) return;

  // staging: one wave instruction = 4 rows x 256 B; lane -> (row l>>4, LDS chunk l&15).
  // Bank swizzle for the transpose reads: a ds_read_b64_tr_b16 pass covers 32 lanes = 8 tile
  // rows {8g + j : g in 0..1, j in 0..3} x one 32-B segment each; all rows sit on the same
  // banks (256-B pitch), so the 32-B segment index is XORed with f(row) = (row & 3) |
  // ((row >> 3) & 1) << 2, which is distinct for those 8 rows -> conflict-free.  The LDS-DMA
  // writes lane-linear, so the permutation is applied to the SOURCE chunk (cdna guide rule 21).
  const int sr = lane >> 4, sc = lane & 15;
  const int n_chunks = (N + 7) / 8, k_chunks = (K + 7) / 8;
  int ycol[4], xcol[4];   // per 4-row group handled by this wave (rb = wid + 4*i  ->  (rb >> 1) & 1 == (i*4 + wid) >> 1 & 1)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int rb = wid + i * 4;
    const int f = sr | (((rb >> 1) & 1) << 2);
    const int gc = sc ^ (f << 1);
    // clamp the 8-column chunk so a ragged N / K never reads past the row pitch
    ycol[i] = min(i0 / 8 + gc, n_chunks - 1) * 8;
    xcol[i] = min(j0 / 8 + gc, k_chunks - 1) * 8;
  }

  auto stage = [&](int mt, int s) {
    char* sy = smem + s * 2 * WG_TILE_BYTES;
    char* sx = sy + WG_TILE_BYTES;
    const int mbase = m_begin + mt * BK;
    const bool fullt = (mbase + BK <= m_end);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rb = wid + i * 4;            // group of 4 rows
      const int m = mbase + rb * 4 + sr;
      if (fullt) {
        __builtin_amdgcn_global_load_lds(GLB_PTR(dY + (size_t)m * lddy + ycol[i]), LDS_PTR(sy + rb * 1024), 16, 0, 0);
        __builtin_amdgcn_global_load_lds(GLB_PTR(X + (size_t)m * ldx + xcol[i]), LDS_PTR(sx + rb * 1024), 16, 0, 0);
      } else {
        // ragged last tile: rows >= m_end contribute zeros
        uint4 vy = make_uint4(0, 0, 0, 0), vx = make_uint4(0, 0, 0, 0);
        if (m < m_end) {
          vy = *reinterpret_cast<const uint4*>(dY + (size_t)m * lddy + ycol[i]);
          vx = *reinterpret_cast<const uint4*>(X + (size_t)m * ldx + xcol[i]);
        }
        *reinterpret_cast<uint4*>(sy + rb * 1024 + lane * 16) = vy;
        *reinterpret_cast<uint4*>(sx + rb * 1024 + lane * 16) = vx;
      }
    }
  };

  const int wi = wid >> 1, wj = wid & 1;
  const int ft = lane & 15, fg = lane >> 4;
  // tr16 address of lane (t,g) for k-step ks, half jj, sub-tile c:
  //   row = ks*32 + g*8 + jj*4 + (t>>2);  col = wave_base + c*16 + (t&3)*4  (8-byte piece)
  //   chunk = col / 8 swizzled with f(row) << 1, f(row) = (t>>2) | (g&1)<<2 for every ks, jj
  const int frow = (fg * 8 + (ft >> 2)) * WG_ROWB;
  const int fsw = ((ft >> 2) | ((fg & 1) << 2)) << 1;
  int y_off[4], x_off[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int qy = wi * 8 + 2 * c + ((ft & 3) >> 1), qx = wj * 8 + 2 * c + ((ft & 3) >> 1);
    y_off[c] = frow + ((qy ^ fsw) << 4) + ((ft & 1) << 3);
    x_off[c] = WG_TILE_BYTES + frow + ((qx ^ fsw) << 4) + ((ft & 1) << 3);
  }

  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nmt = (m_end - m_begin + BK - 1) / BK;
  stage(0, 0);
  __syncthreads();
  for (int mt = 0; mt < nmt; ++mt) {
    const int cur = mt & 1;
    if (mt + 1 < nmt) stage(mt + 1, cur ^ 1);
    const char* sbase = smem + cur * 2 * WG_TILE_BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 yf[4], xf[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const char* py = sbase + y_off[c] + ks * 32 * WG_ROWB;
        const char* px = sbase + x_off[c] + ks * 32 * WG_ROWB;
        bf16x4 y0 = lds_tr16(py), y1 = lds_tr16(py + 4 * WG_ROWB);
        bf16x4 x0 = lds_tr16(px), x1 = lds_tr16(px + 4 * WG_ROWB);
        yf[c] = bf16x8{y0[0], y0[1], y0[2], y0[3], y1[0], y1[1], y1[2], y1[3]};
        xf[c] = bf16x8{x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
      }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yf[a], xf[b], acc[a][b], 0, 0, 0);
    }
    __syncthreads();
  }

  // D[i][j]: lane holds j = l&15, i = 4*(l>>4)+r
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int j = j0 + wj * 64 + b * 16 + ft;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + wi * 64 + a * 16 + fg * 4 + r;
        if (i < N && j < K) unsafeAtomicAdd(dW + (size_t)i * lddw + j, alpha * acc[a][b][r]);
      }
    }
}

#include "gemm_wgrad_w4.hpp"
// ---------------------------------------------------------------------------------
// Weight-gradient kernel, persistent stream-K ring version (production path when M % 64 == 0):
// dW[i,j] += alpha * sum_m dY[m,i] X[m,j] with 256(i) x 128(j) output tiles.  The whole
// contraction space (all output tiles x all 64-row K-tiles of M) is ONE stream, ordered
// (m-chunk, tile, K-tile) with the chunk length equal to one workgroup's share of the stream:
// workgroup w then owns exactly (chunk w / ntile, tile w % ntile), so the 32 workgroups of an
// XCD walk the SAME rows of M at the same time on 32 neighbouring tiles and share their
// dY / X row blocks in that XCD's L2 (measured: L2 hit rate 5 % -> see DESIGN.md with a
// 32-K-tile chunk, every operand byte came from the fabric).  The ragged last chunk is
// dealt out stream-K style, so every workgroup still gets an equal share (no split-factor
// quantisation) and at most a few fp32-atomic flushes.  Each workgroup runs its share through
// the same three-stage LDS ring / counted-vmcnt / double-buffered-fragment pipeline as the NT
// kernel; fragments come out of LDS with ds_read_b64_tr_b16 (inline asm, conflict-free
// through the source-side segment swizzle).
// ---------------------------------------------------------------------------------
constexpr int WR_I = 256, WR_J = 128;
constexpr int WR_YROW = WR_I * 2, WR_XROW = WR_J * 2;             // 512 / 256 B per LDS row
constexpr int WR_YB = BK * WR_YROW, WR_XB = BK * WR_XROW;         // 32 KB + 16 KB
constexpr int WR_STAGE = WR_YB + WR_XB;

__global__ __launch_bounds__(512)
void gemm_wgrad_ring_kernel(const bf16* __restrict__ dY, int lddy, const bf16* __restrict__ X, int ldx,
                            float* __restrict__ dW, int lddw, int M, int N, int K, float alpha,
                            int tiles_i, int tiles_j, int WR_CHUNK) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ntile = tiles_i * tiles_j;
  const int nmt = M / BK;
  const long long total_all = (long long)ntile * nmt;
  const int nwg = gridDim.x;
  const int slot = xcd_slot(nwg);
  // Two schedules.  Few tiles / long M (every layer weight): stream-K with chunk == share, see
  // above.  Many tiles / short M (the tied vocabulary matrix: 5862 tiles, 76 K-tiles): tiles
  // are dealt round-robin (WR_CHUNK == 0), each done over all of M by one workgroup, so that
  // an XCD's 32 workgroups hold 32 consecutive tiles = the six j-tiles of ~5 dY panels.
  const bool rr = (WR_CHUNK == 0);
  int g0, total;
  if (rr) {
    const int my_tiles = (ntile > slot) ? (ntile - slot + nwg - 1) / nwg : 0;
    if (my_tiles == 0) return;
    g0 = 0;
    total = my_tiles * nmt;
  } else {
    // shares are whole chunk strips: workgroup `slot` owns stream positions [slot*share, +share)
    const long long share = (total_all + nwg - 1) / nwg;
    const long long g0l = share * slot;
    if (g0l >= total_all) return;
    g0 = (int)g0l;
    total = (int)((g0l + share <= total_all ? g0l + share : total_all) - g0l);
  }

  auto locate = [&](int g) {
    WgCursor cu;
    if (rr) { cu.c = 0; cu.t = slot; cu.mt = 0; cu.len = nmt; return cu; }
    const int full = ntile * WR_CHUNK;
    cu.c = g / full;
    const int rem = g - cu.c * full;
    cu.len = min(WR_CHUNK, nmt - cu.c * WR_CHUNK);
    cu.t = rem / cu.len;
    cu.mt = rem - cu.t * cu.len;
    return cu;
  };
  auto advance = [&](WgCursor& cu) {
    if (++cu.mt == cu.len) {
      cu.mt = 0;
      if (rr) { cu.t += nwg; return; }
      if (++cu.t == ntile) { cu.t = 0; ++cu.c; cu.len = min(WR_CHUNK, nmt - cu.c * WR_CHUNK); }
    }
  };

  // ---- staging.  dY: one wave instruction = 2 rows x 512 B, lane -> (row l>>5, pos l&31);
  //      X: 4 rows x 256 B, lane -> (row l>>4, pos l&15).  Segment swizzle as in the 128^2 kernel.
  const int n_chunks = (N + 7) / 8, k_chunks = (K + 7) / 8;
  WgCursor lc = locate(g0);
  auto stage_next = [&](int s) {
    char* sy = smem + s * WR_STAGE;
    char* sx = sy + WR_YB;
    const int ti = lc.t / tiles_j, tj = lc.t - ti * tiles_j;
    const int mbase = (lc.c * WR_CHUNK + lc.mt) * BK;   // (c == 0 in round-robin mode)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rb = wid + i * 8;               // 2-row group 0..31
      const int row = rb * 2 + (lane >> 5);
      const int f = (row & 3) | (((row >> 3) & 1) << 2);
      const int gc = (lane & 31) ^ (f << 1);
      const int col = min(ti * (WR_I / 8) + gc, n_chunks - 1) * 8;
      __builtin_amdgcn_global_load_lds(GLB_PTR(dY + (size_t)(mbase + row) * lddy + col), LDS_PTR(sy + rb * 1024), 16, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int rb = wid + i * 8;               // 4-row group 0..15
      const int row = rb * 4 + (lane >> 4);
      const int f = (row & 3) | (((row >> 3) & 1) << 2);
      const int gc = (lane & 15) ^ (f << 1);
      const int col = min(tj * (WR_J / 8) + gc, k_chunks - 1) * 8;
      __builtin_amdgcn_global_load_lds(GLB_PTR(X + (size_t)(mbase + row) * ldx + col), LDS_PTR(sx + rb * 1024), 16, 0, 0);
    }
    advance(lc);
  };

  // ---- fragment addressing (tr16): lane (t = l&15, g = l>>4) reads row g*8 + (t>>2) (+32 ks, +4 jj),
  //      8-byte piece (t&3) of 16-column sub-tile c
  const int wi = wid >> 1, wj = wid & 1;
  const int ft = lane & 15, fg = lane >> 4;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  const int frow = fg * 8 + (ft >> 2);
  const int fsw = ((ft >> 2) | ((fg & 1) << 2)) << 1;
  uint32_t y_addr[4], x_addr[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int qy = wi * 8 + 2 * c + ((ft & 3) >> 1), qx = wj * 8 + 2 * c + ((ft & 3) >> 1);
    y_addr[c] = lds0 + frow * WR_YROW + ((qy ^ fsw) << 4) + ((ft & 1) << 3);
    x_addr[c] = lds0 + WR_YB + frow * WR_XROW + ((qx ^ fsw) << 4) + ((ft & 1) << 3);
  }
  // k-step 0 / 1 of a stage: row offsets 0 / 32 rows; second half of a fragment: +4 rows
  auto read_set0 = [&](uint32_t so, s16x4 (&y)[4][2], s16x4 (&x)[4][2]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      M3P_TR(y[c][0], y_addr[c] + so, 0); M3P_TR(y[c][1], y_addr[c] + so, 2048);
      M3P_TR(x[c][0], x_addr[c] + so, 0); M3P_TR(x[c][1], x_addr[c] + so, 1024);
    }
  };
  auto read_set1 = [&](uint32_t so, s16x4 (&y)[4][2], s16x4 (&x)[4][2]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      M3P_TR(y[c][0], y_addr[c] + so, 16384); M3P_TR(y[c][1], y_addr[c] + so, 18432);
      M3P_TR(x[c][0], x_addr[c] + so, 8192); M3P_TR(x[c][1], x_addr[c] + so, 9216);
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto frag = [](const s16x4 (&h)[2]) {
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(h[0], h[1], 0, 1, 2, 3, 4, 5, 6, 7));
  };
  auto mfma_batch = [&](const s16x4 (&y)[4][2], const s16x4 (&x)[4][2]) {
    bf16x8 yf[4], xf[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) { yf[c] = frag(y[c]); xf[c] = frag(x[c]); }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b)
        acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yf[a], xf[b], acc[a][b], 0, 0, 0);
  };

  stage_next(0);
  if (total > 1) {
    stage_next(1);
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  s16x4 y0[4][2], x0[4][2], y1[4][2], x1[4][2];
  read_set0(0, y0, x0);
  M3P_WAIT_LGKM(0);
  WgCursor cc = locate(g0);
  int cur = 0;
  for (int step = 0; step < total; ++step) {
    const int nxt = (cur == 2) ? 0 : cur + 1;
    const int nx2 = (nxt == 2) ? 0 : nxt + 1;
    const bool more2 = (step + 2 < total);
    if (more2) stage_next(nx2);
    read_set1(cur * WR_STAGE, y1, x1);
    __builtin_amdgcn_sched_barrier(0);
    mfma_batch(y0, x0);
    M3P_WAIT_LGKM(0);
    if (more2) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    read_set0(nxt * WR_STAGE, y0, x0);   // stale after the last K-tile: unused
    __builtin_amdgcn_sched_barrier(0);
    mfma_batch(y1, x1);
    M3P_WAIT_LGKM(0);

    const bool last_of_tile = (cc.mt + 1 == cc.len) || (step + 1 == total);
    if (last_of_tile) {
      // flush this (tile, chunk) segment: D[i][j], lane holds j = l&15, i = 4*(l>>4)+r
      const int ti = cc.t / tiles_j, tj = cc.t - ti * tiles_j;
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int j = tj * WR_J + wj * 64 + b * 16 + ft;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = ti * WR_I + wi * 64 + a * 16 + fg * 4 + r;
            if (i < N && j < K) unsafeAtomicAdd(dW + (size_t)i * lddw + j, alpha * acc[a][b][r]);
            acc[a][b][r] = 0.f;
          }
        }
    }
    advance(cc);
    cur = nxt;
  }
}

}  // namespace

namespace {
template <int EPI, bool A_BF8>
int launch_nt_fp8(const uint8_t* A, int lda, const uint8_t* W, int ldw, bf16* C, int ldc, int M, int N, int K,
                         const M3PEpilogue& ep, hipStream_t st) {
  const int tiles_m = M / 256, tiles_n = N / 256;
  const size_t lds = 2 * 512 * ROWB + (EPI == M3P_EPI_DGELU ? GELU_TAB_N * sizeof(float) : 0) +
                     ((EPI == M3P_EPI_DGELU || EPI == M3P_EPI_MUL) ? 8 * 2048 : 8 * 4096);
  constexpr auto kern = gemm_nt_w8f8_kernel<EPI, A_BF8>;
  if (int rc = set_max_lds<kern>(lds)) return rc;
  const int grid = persistent_grid(tiles_m * tiles_n);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, st, A, lda, W, ldw, C, ldc, M, N, K, ep, tiles_m, tiles_n);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

}  // namespace

extern "C" {

int m3p_gemm_nt_bf16(const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K,
                     int epilogue, const M3PEpilogue* ep_in, void* stream) {
  if (M <= 0 || N <= 0 || K <= 0 || (K % BK) != 0 || (lda % 8) != 0 || (ldw % 8) != 0 || (ldc % 4) != 0)
    return M3P_EINVAL;   // (K % 64 == 0 also covers the 32-deep stages of the 256x256 kernel)
  if (((uintptr_t)A & 15) || ((uintptr_t)W & 15) || ((uintptr_t)C & 7)) return M3P_EINVAL;
  M3PEpilogue ep = {};
  if (ep_in) ep = *ep_in;
  if ((epilogue == M3P_EPI_BIAS_DROP_RES || epilogue == M3P_EPI_RES || epilogue == M3P_EPI_DGELU || epilogue == M3P_EPI_MUL) &&
      (!ep.aux || (ep.ld_aux % 4) != 0))
    return M3P_EINVAL;
  if (epilogue == M3P_EPI_BIAS_GELU && (!ep.out2 || (ep.ld_out2 % 4) != 0)) return M3P_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const bf16* a = (const bf16*)A; const bf16* w = (const bf16*)W; bf16* c = (bf16*)C;
  switch (epilogue) {
    case M3P_EPI_NONE: return launch_nt<M3P_EPI_NONE>(a, lda, w, ldw, c, ldc, M, N, K, ep, st);
    case M3P_EPI_BIAS: return launch_nt<M3P_EPI_BIAS>(a, lda, w, ldw, c, ldc, M, N, K, ep, st);
    case M3P_EPI_BIAS_GELU: return launch_nt<M3P_EPI_BIAS_GELU>(a, lda, w, ldw, c, ldc, M, N, K, ep, st);
    case M3P_EPI_BIAS_DROP_RES: return launch_nt<M3P_EPI_BIAS_DROP_RES>(a, lda, w, ldw, c, ldc, M, N, K, ep, st);
    case M3P_EPI_RES: return launch_nt<M3P_EPI_RES>(a, lda, w, ldw, c, ldc, M, N, K, ep, st);
    case M3P_EPI_DGELU: return launch_nt<M3P_EPI_DGELU>(a, lda, w, ldw, c, ldc, M, N, K, ep, st);
    case M3P_EPI_MUL: return launch_nt<M3P_EPI_MUL>(a, lda, w, ldw, c, ldc, M, N, K, ep, st);
    case M3P_EPI_MULQ: return launch_nt_gq<M3P_EPI_MULQ>(a, lda, w, ldw, c, ldc, M, N, K, ep, st);
    case M3P_EPI_BIAS_GELUQ: return launch_nt_gq<M3P_EPI_BIAS_GELUQ>(a, lda, w, ldw, c, ldc, M, N, K, ep, st);
    case M3P_EPI_BIAS_LSE:      // (row_ref set: the shifted-exponential form, an instantiation of its own)
      if (ep.row_ref) return launch_nt_gq<M3P_EPI_BIAS_EXP>(a, lda, w, ldw, c, ldc, M, N, K, ep, st);
      return launch_nt_gq<M3P_EPI_BIAS_LSE>(a, lda, w, ldw, c, ldc, M, N, K, ep, st);
    default: return M3P_EINVAL;
  }
}

int m3p_gemm_nt_fp8(const void* A, int lda, int a_is_bf8, const void* W, int ldw, void* C, int ldc, int M, int N, int K,
                    int epilogue, const M3PEpilogue* ep_in, void* stream) {
  if (M <= 0 || N <= 0 || K <= 0 || (K % 128) != 0 || (lda % 16) != 0 || (ldw % 16) != 0 || (ldc % 8) != 0) return M3P_EINVAL;
  if ((M % 256) != 0 || (N % 256) != 0) return M3P_EINVAL;       // full 256x256 tiles only (the encoder layers' shapes)
  if (((uintptr_t)A & 15) || ((uintptr_t)W & 15) || ((uintptr_t)C & 15)) return M3P_EINVAL;
  M3PEpilogue ep = {};
  if (ep_in) ep = *ep_in;
  if ((epilogue == M3P_EPI_BIAS_DROP_RES || epilogue == M3P_EPI_RES || epilogue == M3P_EPI_DGELU || epilogue == M3P_EPI_MUL) &&
      (!ep.aux || (ep.ld_aux % 8) != 0))
    return M3P_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const uint8_t* a = (const uint8_t*)A; const uint8_t* w = (const uint8_t*)W; bf16* c = (bf16*)C;
#define M3P_F8_CASE(E)                                                                                        \
  case E: return a_is_bf8 ? launch_nt_fp8<E, true>(a, lda, w, ldw, c, ldc, M, N, K, ep, st)                    \
                          : launch_nt_fp8<E, false>(a, lda, w, ldw, c, ldc, M, N, K, ep, st)
  switch (epilogue) {
    M3P_F8_CASE(M3P_EPI_NONE);
    M3P_F8_CASE(M3P_EPI_BIAS);
    M3P_F8_CASE(M3P_EPI_BIAS_DROP_RES);
    M3P_F8_CASE(M3P_EPI_RES);
    M3P_F8_CASE(M3P_EPI_DGELU);
    M3P_F8_CASE(M3P_EPI_MUL);
    default: return M3P_ENOTIMPL;
  }
#undef M3P_F8_CASE
}

static int launch_streamk(const void* A, int lda, const void* W, int ldw, float* C, int ldc, int M, int N, int K, float alpha,
                          bool w_kn, int k_valid, void* stream) {
  if (M <= 0 || N <= 0 || K <= 0 || (K % BK) != 0 || (lda % 8) != 0 || (ldw % 8) != 0) return M3P_EINVAL;
  if (((uintptr_t)A & 15) || ((uintptr_t)W & 15)) return M3P_EINVAL;
  if (w_kn && (k_valid <= 0 || k_valid > K)) return M3P_EINVAL;
  const int tiles_m_all = (M + 255) / 256, tiles_n = (N + 127) / 128;
  const size_t lds = 3 * (256 + 128) * ROWB;
  if (int rc = w_kn ? set_max_lds<gemm_nt_streamk_kernel<true>>(lds) : set_max_lds<gemm_nt_streamk_kernel<false>>(lds)) return rc;
  auto kern = w_kn ? gemm_nt_streamk_kernel<true> : gemm_nt_streamk_kernel<false>;
  const int grid = num_cus();
  const int nk = K / BK;
  // More tiles than workgroups: one launch would hand every workgroup 1.x whole tiles, so the workgroups
  // sit at 256 different K positions and the second operand (384 MB for the vocabulary) streams from
  // HBM once per tile row (measured: 551 TF/s at M = 19456 against 896 at M = 4864).  Row blocks of at
  // most one tile per workgroup keep every launch in the regime the kernel was laid out for: all
  // workgroups walk the same K range together and W is shared through L2 / MALL.
  const int n_launch = (tiles_m_all * tiles_n + grid - 1) / grid;
  const int rows_per = ((tiles_m_all + n_launch - 1) / n_launch) * 256;
  for (int m0 = 0; m0 < M; m0 += rows_per) {
    const int m = (M - m0 < rows_per) ? M - m0 : rows_per;
    const int tiles_m = (m + 255) / 256;
    long long share = ((long long)tiles_m * tiles_n * nk + grid - 1) / grid;
    const int chunk = (int)(share < nk ? (share < 1 ? 1 : share) : nk);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, (hipStream_t)stream, (const bf16*)A + (size_t)m0 * lda, lda,
                       (const bf16*)W, ldw, C + (size_t)m0 * ldc, ldc, m, N, K, alpha, tiles_m, tiles_n, chunk, k_valid);
    M3P_CHECK_LAUNCH();
  }
  return M3P_OK;
}

int m3p_gemm_nt_streamk_f32(const void* A, int lda, const void* W, int ldw, float* C, int ldc, int M, int N, int K,
                            float alpha, void* stream) {
  return launch_streamk(A, lda, W, ldw, C, ldc, M, N, K, alpha, false, K, stream);
}

int m3p_gemm_nn_streamk_f32(const void* A, int lda, const void* W, int ldw, int k_valid, float* C, int ldc, int M, int N,
                            int K, float alpha, void* stream) {
  return launch_streamk(A, lda, W, ldw, C, ldc, M, N, K, alpha, true, k_valid, stream);
}

int m3p_set_persistent_grid(int workgroups) {
  if (workgroups < 0 || (workgroups % 8) != 0) return M3P_EINVAL;
  g_persistent_grid = workgroups;
  return M3P_OK;
}

int m3p_set_tile_queue(int32_t* counters, int n_slots) {
  if (counters && (n_slots <= 0 || ((uintptr_t)counters & 3))) return M3P_EINVAL;
  std::lock_guard<std::mutex> lk(g_tq_mu);
  g_tq_pool = counters;
  g_tq_slots = counters ? n_slots : 0;
  g_tq_next = 0;
  g_tq_bound = false;        // the next queued launch binds the ring to its stream
  return M3P_OK;
}

size_t m3p_gemm_wgrad_workspace_bytes(void) {
  const size_t grid = (size_t)hw_cus();
  return grid * (65536 + 272) * sizeof(float) + grid * sizeof(int);
}

// The four-wave weight-gradient kernel deals whole tiles round-robin as soon as there are more output tiles than workgroups:
// its other mode gives every workgroup ONE (tile, M-chunk) segment, which covers at most `grid` tiles.  (The switch used to
// sit at four tiles per workgroup, and between one and four the tiles past the grid - tile 8 of a 768 x 768 weight on a
// persistent grid of 8, tiles 256.. of a 272-tile weight on 256 CUs - were never computed: tests/test_gemm_schedules.py.)
static bool wgrad_w4_whole_tiles(long long ntile, int grid) { return ntile > (long long)grid; }

// m3p_gemm_wgrad_bias_arm: the calling thread's next whole-tile launch through m3p_gemm_wgrad_store_bf16 / m3p_gemm_wgrad_bf16
// is the BIAS instantiation with these operands (the callers of those entry points keep their call and its return code)
static thread_local const float* g_bias_w = nullptr;
static thread_local float* g_bias_out = nullptr;
static thread_local int g_bias_taken = 0;
int m3p_gemm_wgrad_bias_arm(const float* w, float* bsum) {
  const int taken = g_bias_taken;
  g_bias_taken = 0;
  g_bias_w = (w && bsum && !((uintptr_t)w & 3) && !((uintptr_t)bsum & 3)) ? w : nullptr;
  g_bias_out = g_bias_w ? bsum : nullptr;
  return taken;
}

// four-wave kernel + reduction; pb: optional second product over the same M (paired launch), nullptr = none
static bool wgrad_w4_ok(int M, int N, int K, int lddy, int ldx, const void* dY, const void* X) {
  return (M % 64) == 0 && M >= 4096 && (N % 256) == 0 && (K % 256) == 0 &&
         (lddy % 8) == 0 && (ldx % 8) == 0 && !((uintptr_t)dY & 15) && !((uintptr_t)X & 15);
}
extern "C++" {
template <bool YROWS = false>
static int launch_wgrad_w4(const void* dY, int lddy, const void* X, int ldx, float* dW, int lddw, int M, int N, int K,
                           float alpha, void* workspace, size_t workspace_bytes, void* stream, const WgradProblem* pb_in,
                           bool store = false) {
  const int ti = N / 256, tj = K / 256;
  WgradProblem pb = {};
  if (pb_in) pb = *pb_in;
  const int ntile = ti * tj + pb.tiles_i * pb.tiles_j;
  const size_t lds = 2 * 65536;
  if (int rc = set_max_lds<gemm_wgrad_w4_kernel<YROWS>>(lds)) return rc;
  const int grid = num_cus();
  const int nmt = M / 64;
  long long share = ((long long)ntile * nmt + grid - 1) / grid;
  int chunk = (int)(share < nmt ? (share < 1 ? 1 : share) : nmt);
  if (wgrad_w4_whole_tiles(ntile, grid)) chunk = 0;   // more tiles than workgroups: round-robin whole tiles
  if (pb_in && chunk == 0) return M3P_EINVAL;       // (pairs only in the one-segment-per-workgroup mode; the caller checks)
  if (store && chunk != 0) return M3P_ENOTIMPL;     // (a plain store needs every tile flushed exactly once: whole-tile round-robin mode)
  if constexpr (!YROWS) {
    if (g_bias_w && chunk == 0 && !pb_in && 2 * 65536 + (size_t)M * 2 <= 160 * 1024) {
      // armed (m3p_gemm_wgrad_bias_arm): the same whole-tile launch, column tile 0 also sums the first operand's weighted columns
      if (int rc = set_max_lds<gemm_wgrad_w4_kernel<false, WgradBias>>(160 * 1024)) return rc;
      hipLaunchKernelGGL((gemm_wgrad_w4_kernel<false, WgradBias>), dim3(grid), dim3(256), 2 * 65536 + (size_t)M * 2,
                         (hipStream_t)stream, (const bf16*)dY, lddy, (const bf16*)X, ldx, dW, lddw, M, N, K, alpha, ti, tj, 0,
                         (float*)nullptr, (int*)nullptr, store ? 1 : 0, WgradProblem{}, WgradBias{g_bias_w, g_bias_out});
      M3P_CHECK_LAUNCH();
      g_bias_w = nullptr;
      g_bias_out = nullptr;
      g_bias_taken = 1;
      return M3P_OK;
    }
  }
  // workspace for first-segment partials: one 256-KB slot per workgroup + a tile-id word each, owned by the
  // CALLER (m3p_gemm_wgrad_workspace_bytes): launches that may overlap on different streams need one each.
  // Without it the partial tiles go to dW with fp32 atomics (slower: DESIGN.md section 4).
  float* ws = nullptr;
  if (workspace && workspace_bytes >= m3p_gemm_wgrad_workspace_bytes() && (((uintptr_t)workspace & 15) == 0) && chunk != 0 &&
      (lddw % 4) == 0 && (((uintptr_t)dW & 15) == 0) && (!pb_in || ((pb.lddw % 4) == 0 && (((uintptr_t)pb.dW & 15) == 0))))
    ws = (float*)workspace;
  int* ws_tile = ws ? (int*)(ws + (size_t)grid * (65536 + 272)) : nullptr;
  hipLaunchKernelGGL(gemm_wgrad_w4_kernel<YROWS>, dim3(grid), dim3(256), lds, (hipStream_t)stream, (const bf16*)dY, lddy,
                     (const bf16*)X, ldx, dW, lddw, M, N, K, alpha, ti, tj, chunk, ws, ws_tile, store ? 1 : 0, pb);
  M3P_CHECK_LAUNCH();
  if (ws) {
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(16, ntile), dim3(256), 0, (hipStream_t)stream, (const float*)ws,
                       (const int*)ws_tile, grid, dW, lddw, tj, alpha, ti * tj, pb);
    M3P_CHECK_LAUNCH();
  }
  return M3P_OK;
}
}  // extern "C++"

// ---------------------------------------------------------------------------------------------------------------------
// WHICH KERNEL RUNS A WEIGHT GRADIENT dW[N,K] += dY[M,N]^T X[M,K] (m3p_gemm_wgrad_plan reports it):
//
//   shape                                                  kernel                                   why
//   -----------------------------------------------------  ---------------------------------------  --------------------------------
//   up to 12 whole-tile products over one M, together at   four-wave 256x256, ONE workgroup per      no partial tiles: 1339 TF over seven
//     most one tile per CU (m3p_gemm_wgrad_group_bf16,       tile over all of M, placed by XCD;       36-tile units against 1109 through the
//     not part of wgrad_plan: the caller groups)             dW += alpha * acc once, plain stores     launches below (tools/ab_wgrad_group.py)
//   M % 64 == 0, M >= 4096, N % 256 == 0, K % 256 == 0,    four-wave 256x256, one (tile, M-chunk)   1063 / 858 / 983 TF on FFN1 / FFN2 /
//     >= 9 output tiles, at most one tile per CU             segment per workgroup; partial tiles     QKV against 845 / 751 / 808 on the
//                                                            go to the caller's workspace and a       ring kernel; no atomics, summed in
//                                                            reduce kernel (16 x ntile blocks) sums   slot order (bit-reproducible)
//                                                            them into dW in slot order
//   same, more tiles than CUs (the vocabulary matrix)      four-wave, whole tiles round-robin       each tile flushed once: fp32 atomics,
//                                                                                                    or plain stores (m3p_gemm_wgrad_store_bf16);
//                                                                                                    m3p_gemm_wgrad_bias_bf16: + the weighted
//                                                                                                    column sums of dY from column tile 0
//   M % 64 == 0, M >= 4096 otherwise                       ring stream-K 256x128 (atomics)          ragged N / K
//   anything else                                          128x128 split-M (atomics)                small M (cfg1, tests)
// ---------------------------------------------------------------------------------------------------------------------
static int wgrad_plan(int M, int N, int K, bool aligned) {
  if (aligned && (M % 64) == 0 && M >= 4096 && (N % 256) == 0 && (K % 256) == 0 && (N / 256) * (K / 256) >= 9)
    return wgrad_w4_whole_tiles((long long)(N / 256) * (K / 256), num_cus()) ? M3P_KERN_WGRAD_W4_TILES : M3P_KERN_WGRAD_W4_CHUNKS;
  if ((M % BK) == 0 && M >= 4096) return M3P_KERN_WGRAD_RING;
  return M3P_KERN_WGRAD_128;
}

int m3p_gemm_nt_plan(int M, int N, int K, int epilogue) {
  if (M <= 0 || N <= 0 || K <= 0 || (K % BK) != 0 || epilogue < 0 || epilogue > M3P_EPI_BIAS_LSE) return M3P_EINVAL;
  int queue = 0;
  const int plan = nt_plan(epilogue, M, N, K, &queue);
  return (plan == M3P_KERN_NT_W8 && queue) ? M3P_KERN_NT_W8_QUEUE : plan;
}

int m3p_gemm_wgrad_plan(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0) return M3P_EINVAL;
  return wgrad_plan(M, N, K, true);
}

// Cf[M,N] += alpha * A[M,K] x W[K,N] on the four-wave kernel (YROWS form): the weight-gradient machinery with the roles
//   contraction = K, output rows = M (first operand A, contraction-contiguous), output columns = N (second operand W, rows = contraction)
int m3p_gemm_nn_w4_f32(const void* A, int lda, const void* W, int ldw, float* C, int ldc, int M, int N, int K, float alpha,
                       void* workspace, size_t workspace_bytes, void* stream) {
  if (M <= 0 || N <= 0 || K <= 0 || !A || !W || !C) return M3P_EINVAL;
  if ((K % 64) || K < 4096 || (M % 256) || (N % 256) || (lda % 8) || (ldw % 8) || lda < K || ldw < N || ldc < N ||
      ((uintptr_t)A & 15) || ((uintptr_t)W & 15))
    return M3P_ENOTIMPL;
  return launch_wgrad_w4<true>(A, lda, W, ldw, C, ldc, K, M, N, alpha, workspace, workspace_bytes, stream, nullptr);
}

int m3p_gemm_wgrad_pair_bf16(const void* dYa, int lddya, const void* Xa, int ldxa, float* dWa, int lddwa, int Na, int Ka,
                             const void* dYb, int lddyb, const void* Xb, int ldxb, float* dWb, int lddwb, int Nb, int Kb,
                             int M, float alpha, void* workspace, size_t workspace_bytes, void* stream) {
  if (M <= 0 || Na <= 0 || Ka <= 0 || Nb <= 0 || Kb <= 0) return M3P_EINVAL;
  const bool pair = wgrad_w4_ok(M, Na, Ka, lddya, ldxa, dYa, Xa) && wgrad_w4_ok(M, Nb, Kb, lddyb, ldxb, dYb, Xb) &&
                    workspace && workspace_bytes >= m3p_gemm_wgrad_workspace_bytes() && (((uintptr_t)workspace & 15) == 0) &&
                    // (the workspace form's own conditions - launch_wgrad_w4 - so that a pair never lands on the atomic flush)
                    (lddwa % 4) == 0 && (lddwb % 4) == 0 && (((uintptr_t)dWa | (uintptr_t)dWb) & 15) == 0 &&
                    lddwa >= Ka && lddwb >= Kb &&
                    (long long)((Na / 256) * (Ka / 256) + (Nb / 256) * (Kb / 256)) * 2 <= num_cus();
  if (!pair) {
    int rc = m3p_gemm_wgrad_bf16(dYa, lddya, Xa, ldxa, dWa, lddwa, M, Na, Ka, alpha, workspace, workspace_bytes, stream);
    if (rc != M3P_OK) return rc;
    return m3p_gemm_wgrad_bf16(dYb, lddyb, Xb, ldxb, dWb, lddwb, M, Nb, Kb, alpha, workspace, workspace_bytes, stream);
  }
  if (lddya < Na || ldxa < Ka || lddyb < Nb || ldxb < Kb) return M3P_EINVAL;
  WgradProblem pb = {(const bf16*)dYb, (const bf16*)Xb, dWb, lddyb, ldxb, lddwb, Nb / 256, Kb / 256};
  return launch_wgrad_w4<>(dYa, lddya, Xa, ldxa, dWa, lddwa, M, Na, Ka, alpha, workspace, workspace_bytes, stream, &pb);
}

// Placement of a grouped launch: workgroup w sits on XCD w % 8, position w / 8 of its `workgroups / 8` CUs.  The tiles of one
// product share their dY row panels and X column panels only through the XCD's L2, so every product first takes as many WHOLE
// XCDs as it fills, then the remainders go, largest first, each to the XCD with the least room that still takes it whole
// (split over the emptiest ones only when none does).  Seven 36-tile products on 256 CUs: 32 tiles of product k on XCD k,
// the seven remainders of 4 on XCD 7.  A product's tiles are dealt in row-major order, so neighbours in an XCD share a dY panel.
int m3p_gemm_wgrad_group_place(const int* tiles_i, const int* tiles_j, int n_items, int workgroups, uint32_t* place) {
  if (!tiles_i || !tiles_j || !place || n_items < 1 || n_items > M3P_WGRAD_GROUP_MAX || workgroups < 8 || workgroups > 256 ||
      (workgroups % 8) != 0)
    return M3P_EINVAL;
  const int per_xcd = workgroups / 8;
  int total = 0;
  for (int k = 0; k < n_items; ++k) {
    if (tiles_i[k] < 1 || tiles_j[k] < 1 || tiles_i[k] > 256 || tiles_j[k] > 256) return M3P_EINVAL;
    total += tiles_i[k] * tiles_j[k];
    if (total > workgroups) return M3P_ENOTIMPL;
  }
  int used[8] = {0, 0, 0, 0, 0, 0, 0, 0};       // tiles placed on each XCD
  int next[M3P_WGRAD_GROUP_MAX];                // next tile of each item to place
  for (int w = 0; w < workgroups; ++w) place[w] = 0xffffffffu;
  auto put = [&](int k, int xcd, int n) {
    for (int e = 0; e < n; ++e, ++next[k], ++used[xcd])
      place[used[xcd] * 8 + xcd] = (uint32_t)k << 16 | (uint32_t)(next[k] / tiles_j[k]) << 8 | (uint32_t)(next[k] % tiles_j[k]);
  };
  int xcd = 0;
  for (int k = 0; k < n_items; ++k) {
    next[k] = 0;
    for (int full = tiles_i[k] * tiles_j[k] / per_xcd; full > 0; --full) put(k, xcd++, per_xcd);
  }
  int order[M3P_WGRAD_GROUP_MAX];
  for (int k = 0; k < n_items; ++k) order[k] = k;
  auto left = [&](int k) { return tiles_i[k] * tiles_j[k] - next[k]; };
  std::stable_sort(order, order + n_items, [&](int a, int b) { return left(a) > left(b); });
  for (int o = 0; o < n_items; ++o) {
    const int k = order[o];
    while (left(k) > 0) {
      int best = -1, emptiest = 0;
      for (int x = 0; x < 8; ++x) {
        const int room = per_xcd - used[x];
        if (room >= left(k) && (best < 0 || room < per_xcd - used[best])) best = x;
        if (room > per_xcd - used[emptiest]) emptiest = x;
      }
      if (best >= 0) put(k, best, left(k));
      else put(k, emptiest, per_xcd - used[emptiest]);
    }
  }
  return M3P_OK;
}

int m3p_gemm_wgrad_group_bf16(const M3PWgradItem* items, int n_items, int M, float alpha, void* stream) {
  if (!items || n_items < 1 || n_items > M3P_WGRAD_GROUP_MAX || M <= 0) return M3P_EINVAL;
  const int grid = num_cus();
  if (grid > 256) return M3P_ENOTIMPL;
  WgradGroup grp;
  int ti[M3P_WGRAD_GROUP_MAX], tj[M3P_WGRAD_GROUP_MAX];
  for (int k = 0; k < n_items; ++k) {
    const M3PWgradItem& it = items[k];
    if (!it.dY || !it.X || !it.dW || it.N <= 0 || it.K <= 0) return M3P_EINVAL;
    if (!wgrad_w4_ok(M, it.N, it.K, it.lddy, it.ldx, it.dY, it.X) || it.lddy < it.N || it.ldx < it.K || it.lddw < it.K ||
        (it.lddw % 4) != 0 || ((uintptr_t)it.dW & 15) || it.N / 256 > 256 || it.K / 256 > 256)
      return M3P_ENOTIMPL;
    ti[k] = it.N / 256;
    tj[k] = it.K / 256;
    grp.item[k] = {(const bf16*)it.dY, (const bf16*)it.X, it.dW, it.lddy, it.ldx, it.lddw, tj[k]};
  }
  for (int k = n_items; k < M3P_WGRAD_GROUP_MAX; ++k) grp.item[k] = {nullptr, nullptr, nullptr, 0, 0, 0, 0};
  for (int w = grid; w < 256; ++w) grp.place[w] = 0xffffffffu;
  if (int rc = m3p_gemm_wgrad_group_place(ti, tj, n_items, grid, grp.place)) return rc;
  const size_t lds = 2 * 65536;
  if (int rc = set_max_lds<gemm_wgrad_w4_kernel<false, WgradGroup>>(lds)) return rc;
  hipLaunchKernelGGL((gemm_wgrad_w4_kernel<false, WgradGroup>), dim3(grid), dim3(256), lds, (hipStream_t)stream,
                     (const bf16*)nullptr, 0, (const bf16*)nullptr, 0, (float*)nullptr, 0, M, 0, 0, alpha, 0, 0, 1,
                     (float*)nullptr, (int*)nullptr, 0, WgradProblem{}, grp);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

int m3p_gemm_wgrad_store_bf16(const void* dY, int lddy, const void* X, int ldx, float* dW, int lddw, int M, int N, int K,
                              float alpha, void* workspace, size_t workspace_bytes, void* stream) {
  if (M <= 0 || N <= 0 || K <= 0 || (lddy % 8) != 0 || (ldx % 8) != 0 || !dW || lddw < K) return M3P_EINVAL;
  if (lddy < N || ldx < K || ((uintptr_t)dY & 15) || ((uintptr_t)X & 15)) return M3P_EINVAL;
  if (!wgrad_w4_ok(M, N, K, lddy, ldx, dY, X)) return M3P_ENOTIMPL;
  return launch_wgrad_w4<>(dY, lddy, X, ldx, dW, lddw, M, N, K, alpha, workspace, workspace_bytes, stream, nullptr, true);
}

// The whole-tile launch with the first operand's weighted column sums beside the product (gemm_wgrad_w4_kernel, BIAS).
// The weight vector, in bf16, shares the workgroup's LDS with the two stages: 2 bytes per row of M in the 32 KB behind them.
int m3p_gemm_wgrad_bias_bf16(const void* dY, int lddy, const void* X, int ldx, float* dW, int lddw, int M, int N, int K,
                             float alpha, const float* w, float* bsum, int store, void* stream) {
  if (M <= 0 || N <= 0 || K <= 0 || (lddy % 8) != 0 || (ldx % 8) != 0 || !dY || !X || !dW || !w || !bsum || lddw < K)
    return M3P_EINVAL;
  if (lddy < N || ldx < K) return M3P_EINVAL;
  if (!wgrad_w4_ok(M, N, K, lddy, ldx, dY, X) || ((uintptr_t)w & 3) || ((uintptr_t)bsum & 3)) return M3P_ENOTIMPL;
  const int ti = N / 256, tj = K / 256;
  const int grid = num_cus();
  const size_t lds = 2 * 65536 + (size_t)M * 2;
  if (!wgrad_w4_whole_tiles((long long)ti * tj, grid) || lds > 160 * 1024) return M3P_ENOTIMPL;
  if (int rc = set_max_lds<gemm_wgrad_w4_kernel<false, WgradBias>>(160 * 1024)) return rc;
  hipLaunchKernelGGL((gemm_wgrad_w4_kernel<false, WgradBias>), dim3(grid), dim3(256), lds, (hipStream_t)stream,
                     (const bf16*)dY, lddy, (const bf16*)X, ldx, dW, lddw, M, N, K, alpha, ti, tj, 0, (float*)nullptr,
                     (int*)nullptr, store ? 1 : 0, WgradProblem{}, WgradBias{w, bsum});
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

int m3p_gemm_wgrad_bf16(const void* dY, int lddy, const void* X, int ldx, float* dW, int lddw, int M, int N, int K,
                        float alpha, void* workspace, size_t workspace_bytes, void* stream) {
  if (M <= 0 || N <= 0 || K <= 0 || (lddy % 8) != 0 || (ldx % 8) != 0 || !dW || lddw < K) return M3P_EINVAL;
  if (lddy < ((N + 7) / 8) * 8 || ldx < ((K + 7) / 8) * 8) return M3P_EINVAL;
  if (((uintptr_t)dY & 15) || ((uintptr_t)X & 15)) return M3P_EINVAL;
  const int plan = wgrad_plan(M, N, K, wgrad_w4_ok(M, N, K, lddy, ldx, dY, X));
  if (plan == M3P_KERN_WGRAD_W4_CHUNKS || plan == M3P_KERN_WGRAD_W4_TILES) {      // (768 x 768 = 9 tiles included since the four-wave kernel lost its scalar overhead: 63 against 74 us on the ring kernel)
    return launch_wgrad_w4<>(dY, lddy, X, ldx, dW, lddw, M, N, K, alpha, workspace, workspace_bytes, stream, nullptr);
  }
  if (plan == M3P_KERN_WGRAD_RING) {
    const int ti = (N + WR_I - 1) / WR_I, tj = (K + WR_J - 1) / WR_J;
    const size_t lds = 3 * WR_STAGE;
    if (int rc = set_max_lds<gemm_wgrad_ring_kernel>(lds)) return rc;
    const int grid = num_cus();
    const int nmt = M / BK;
    long long share = ((long long)ti * tj * nmt + grid - 1) / grid;
    int chunk = (int)(share < nmt ? (share < 1 ? 1 : share) : nmt);
    if ((long long)ti * tj >= 4LL * grid) chunk = 0;   // many tiles: round-robin whole tiles
    hipLaunchKernelGGL(gemm_wgrad_ring_kernel, dim3(grid), dim3(512), lds, (hipStream_t)stream, (const bf16*)dY, lddy,
                       (const bf16*)X, ldx, dW, lddw, M, N, K, alpha, ti, tj, chunk);
    M3P_CHECK_LAUNCH();
    return M3P_OK;
  }
  const int tiles_i = (N + WG_T - 1) / WG_T, tiles_j = (K + WG_T - 1) / WG_T;
  const int ntile = tiles_i * tiles_j;
  // split the contraction so that ~2 blocks per CU are in flight; chunk is a multiple of 64
  int split = (512 + ntile - 1) / ntile;
  const int max_split = (M + BK - 1) / BK;
  if (split > max_split) split = max_split;
  if (split < 1) split = 1;
  int m_chunk = ((M + split - 1) / split + BK - 1) / BK * BK;
  split = (M + m_chunk - 1) / m_chunk;
  const size_t lds = 4 * WG_TILE_BYTES;
  if (int rc = set_max_lds<gemm_wgrad_kernel>(lds)) return rc;
  hipLaunchKernelGGL(gemm_wgrad_kernel, dim3(ntile * split), dim3(256), lds, (hipStream_t)stream,
                     (const bf16*)dY, lddy, (const bf16*)X, ldx, dW, lddw, M, N, K, alpha, tiles_i, tiles_j, m_chunk);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

}  // extern "C"
