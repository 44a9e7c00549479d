// Fused multi-head self-attention (forward + backward) for the M3P encoder on gfx950.
//
// Reference semantics (M3P/src/model/transformer.py:149-210, self-attention branch):
//   q = (x Wq + bq) / sqrt(dh)   <- the scale is already folded into the QKV GEMM epilogue
//   P = softmax_fp32(q k^T, keys >= len[b] masked to -inf);  P = dropout(P);  ctx = P v
// One workgroup per (batch, head).  The sequence is short (S = regions + tokens = 164 for
// M3P-base, <= 512), so a whole head's K and V live in LDS (row-major, 16-B chunk XOR
// swizzle applied on the LDS-DMA source address) and the S x S score matrix never
// leaves registers:
//   * S^T = K Q^T on v_mfma_f32_16x16x32_bf16 ("swapped" product): a lane then owns one
//     query column and 4 keys per 16-key tile, so the softmax row reduction is in-lane
//     plus two wave64 xor-shuffles (lanes l, l^16, l^32, l^48 share a query);
//   * the fp32 probabilities are normalised, dropped (counter-based hash RNG, re-generated
//     in backward), packed to bf16 and fed straight back as the MFMA B operand of
//     O^T = V^T P^T — the MFMA k-slot order is permuted identically for P (registers) and
//     V (ds_read_b64_tr_b16 transpose reads), so no cross-lane traffic is needed;
//   * output is token-major [M, d] (head-interleaved) so out_lin consumes it directly.
#include "common.hpp"


namespace {

// the two-phase backward of the M3P sequence (36 regions + 128 tokens: 11 tiles, 6 steps): four-wave workgroups, and the waves
// per SIMD their register allocation must leave room for
constexpr int ATTN_BWD_NW = 4;
constexpr int ATTN_BWD_WPS = 3;

// developer switch (m3p_debug_attn_variant, tests/test_attention.py): bit 0 = the two-phase backward for the M3P sequence,
// bit 1 = the plain one-pass backward instead of the persistent one
static int g_attn_variant = 0;

template <int DH> struct AttnCfg {
  static constexpr int ROWB = DH * 2;        // bytes per K/V row in LDS
  static constexpr int CH = DH / 8;          // 16-B chunks per row
  static constexpr int RPI = 1024 / ROWB;    // rows per LDS-DMA wave instruction
  static constexpr int KK = DH / 32;         // MFMA k-steps across the head dim
  static constexpr int NT = DH / 16;         // 16-wide tiles across the head dim
  // chunk swizzle (only needed, and only bijective within a row, for 128-B rows)
  static __device__ __forceinline__ int swz(int chunk, int row) { return DH == 64 ? (chunk ^ (row & 7)) : chunk; }
};

__device__ __forceinline__ bf16x4 lds_tr16(const char* p) {
  s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(p));
  return __builtin_bit_cast(bf16x4, v);
}
// sum over the 16 lanes of a DPP row (lanes 16 g .. 16 g + 15), result in every lane of the row: quad butterflies, then two
// rotations of the row.  Four VALU adds with DPP operands; __shfl_xor goes through ds_bpermute (an LDS-pipeline round trip each).
__device__ __forceinline__ float row16_sum(float v) {
#define M3P_DPP_ADD(ctrl) v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, 0xf, 0xf, true))
  M3P_DPP_ADD(0xB1);      // quad_perm [1,0,3,2]
  M3P_DPP_ADD(0x4E);      // quad_perm [2,3,0,1]
  M3P_DPP_ADD(0x124);     // row_ror:4
  M3P_DPP_ADD(0x128);     // row_ror:8
#undef M3P_DPP_ADD
  return v;
}
// bit r (0..3) of `bits` as an all-ones / all-zeros word.  (asm: written as sbfe the compiler turns `value & mask` into a bit
// test, a compare and a select - three instructions for two.)
__device__ __forceinline__ uint32_t bit_to_mask(uint32_t bits, int r) {
  uint32_t o;
  switch (r) {
    case 0: asm("v_bfe_i32 %0, %1, 0, 1" : "=v"(o) : "v"(bits)); break;
    case 1: asm("v_bfe_i32 %0, %1, 1, 1" : "=v"(o) : "v"(bits)); break;
    case 2: asm("v_bfe_i32 %0, %1, 2, 1" : "=v"(o) : "v"(bits)); break;
    default: asm("v_bfe_i32 %0, %1, 3, 1" : "=v"(o) : "v"(bits)); break;
  }
  return o;
}
// sum over groups of CH (4 or 8) consecutive lanes, result in every lane of the group
template <int CH>
__device__ __forceinline__ float chunks_sum(float v) {
#define M3P_DPP_ADD(ctrl) v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, 0xf, 0xf, true))
  M3P_DPP_ADD(0xB1);      // quad_perm [1,0,3,2]
  M3P_DPP_ADD(0x4E);      // quad_perm [2,3,0,1]
  if (CH == 8) M3P_DPP_ADD(0x141);   // row_half_mirror: lane j of each 8 <- lane 7 - j (the other quad's sum)
#undef M3P_DPP_ADD
  return v;
}
__device__ __forceinline__ bf16x8 cat8(bf16x4 a, bf16x4 b) {
  return bf16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// A row's 16 columns of a d-tile sit in FOUR lanes (fg = lane >> 4 = 0..3 hold columns 4 fg .. 4 fg + 3: 8 bytes each) after
// the MFMA chains of the backward kernels: NT 8-byte stores per lane and matrix row.  One v_permlane16_swap per register of
// a d-tile PAIR (odd 16-lane rows of the first trade places with the even rows of the second: tests/test_hw_probes.py)
// leaves every lane with 16 contiguous bytes - columns 8 (fg >> 1) .. + 7 of tile n0 + (fg & 1) - and halves the store
// instructions at equal bytes and addresses.  The store tails of these kernels are bound by the CU's vector-memory ISSUE
// (eleven waves x 12 instructions per head: 3.2 k ticks in the persistent kernel's timeline), not by bandwidth (cdna guide,
// T21): 185.7 -> 168.2 us on the persistent backward.  `row` = the lane's matrix row (d-tile 0, column 0); every lane of the
// wave must come through here (the swap exchanges registers between lanes), `ok` masks the store.
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
template <int NT>
__device__ __forceinline__ void store_row_widened(bf16* row, int fg, bool ok, const bf16x4 (&r)[NT]) {
  static_assert(NT % 2 == 0, "d-tiles are swapped in pairs");
  bf16* p = row + 8 * (fg >> 1) + 16 * (fg & 1);
#pragma unroll
  for (int n0 = 0; n0 < NT; n0 += 2) {
    u32x2_t x = __builtin_bit_cast(u32x2_t, r[n0]), y = __builtin_bit_cast(u32x2_t, r[n0 + 1]);
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %2\n\tv_permlane16_swap_b32 %1, %3"
                 : "+v"(x[0]), "+v"(x[1]), "+v"(y[0]), "+v"(y[1]));
    if (ok) *reinterpret_cast<u32x4_t*>(p + 16 * n0) = u32x4_t{x[0], x[1], y[0], y[1]};
  }
}

// Stage `nrows` rows (clamped to the last valid row `S-1`) of a [S, DH] head slice whose rows
// are `ld` elements apart into LDS as [nrows][DH] with the chunk swizzle.
template <int DH>
__device__ __forceinline__ void stage_rows(const bf16* __restrict__ g, size_t ld, int S, int nrows, char* lds,
                                           int wid, int lane, int nwaves = 4) {
  using Cf = AttnCfg<DH>;
  const int rin = lane / Cf::CH, c = lane % Cf::CH;
  const int ninstr = (nrows + Cf::RPI - 1) / Cf::RPI;
  for (int i = wid; i < ninstr; i += nwaves) {
    const int row = i * Cf::RPI + rin;
    const int gr = min(row, S - 1);
    const int gc = Cf::swz(c, row);
    __builtin_amdgcn_global_load_lds(GLB_PTR(g + (size_t)gr * ld + gc * 8), LDS_PTR(lds + i * 1024), 16, 0, 0);
  }
}

// The same transfers issued where the compiler cannot see them (persistent kernels: a tile is requested while the previous
// one is still being computed on).  With the builtin form in flight the compiler assumes the transfer may alias ANY LDS read
// it emits and puts s_waitcnt vmcnt(0) in front of each - the request then completes before the computation it was meant to
// run under starts.  The caller owns the ordering: an (asm volatile) s_waitcnt vmcnt before the tile's first read.  Counted
// vmcnt waits the compiler emits for its own loads stay correct: untracked younger operations only make them stricter.
template <int DH>
__device__ __forceinline__ void stage_rows_hidden(const bf16* __restrict__ g, size_t ld, int S, int nrows, char* lds,
                                                  int wid, int lane, int nwaves) {
  using Cf = AttnCfg<DH>;
  const int rin = lane / Cf::CH, c = lane % Cf::CH;
  const int ninstr = (nrows + Cf::RPI - 1) / Cf::RPI;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)lds;
  for (int i = wid; i < ninstr; i += nwaves) {
    const int row = i * Cf::RPI + rin;
    const int gr = min(row, S - 1);
    const int gc = Cf::swz(c, row);
    const bf16* src = g + (size_t)gr * ld + gc * 8;
    const uint32_t dst = __builtin_amdgcn_readfirstlane(lds0 + (uint32_t)i * 1024u);
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" :: "v"(src), "s"(dst) : "memory", "m0");
  }
}

// ---------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------
// NTC: number of 16-key tiles known at compile time (11 = the M3P sequence, 36 regions + 128 tokens = 164 keys) so the
// per-tile guards fold away (they compiled to ~90 uniform branches and the SGPR pressure behind ~220 lane spills); 0 = runtime.
// NW: waves per workgroup.  4 with three ~48-KB workgroups per CU at S = 164 (168 registers per lane); 8 for long
// sequences whose K + V tiles leave room for one workgroup per CU only (S = 356: 96 KB) - two waves per SIMD
// instead of one to hide each other's latencies.
template <int DH, int KT, bool DROP, int NTC, int NW = 4, bool EVENS = false>     // EVENS: the row length S is even (launcher's promise)
__global__ __launch_bounds__(NW * 64, NW == 8 ? 2 : 3)
void attn_fwd_kernel(const bf16* __restrict__ qkv, const int* __restrict__ keylen, bf16* __restrict__ ctx,
                     float* __restrict__ lse, unsigned long long* __restrict__ keepmask, int S, int H, int dmodel,
                     uint32_t seed, uint32_t thresh24, float inv_keep) {
  using Cf = AttnCfg<DH>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const int nt = NTC ? NTC : (S + 15) >> 4;    // 16-key tiles == 16-query blocks
  const int nk = (nt + 1) >> 1;                // 32-key MFMA steps of P V
  const size_t ld = 3 * (size_t)dmodel;
  const bf16* Qg = qkv + (size_t)b * S * ld + h * DH;
  const bf16* Kg = Qg + dmodel;
  const bf16* Vg = Qg + 2 * dmodel;
  char* sK = smem;
  char* sV = smem + nt * 16 * Cf::ROWB;
  stage_rows<DH>(Kg, ld, S, nt * 16, sK, wid, lane, NW);
  stage_rows<DH>(Vg, ld, S, nk * 32, sV, wid, lane, NW);
  const int fq = lane & 15, fg = lane >> 4;
  // query blocks go round-robin over the waves; the starting wave rotates with the workgroup id so
  // that the waves with one block fewer (nt % 4 != 0) do not always land on the same SIMDs of a CU
  const int wrot = (wid + (blockIdx.x >> 3)) & (NW - 1);
  bf16x8 qnext[Cf::KK];
  {
    const int qc0 = min(wrot * 16 + fq, S - 1);
#pragma unroll
    for (int kk = 0; kk < Cf::KK; ++kk)
      qnext[kk] = *reinterpret_cast<const bf16x8*>(Qg + (size_t)qc0 * ld + 32 * kk + 8 * fg);
  }
  const int klen = keylen[b];
  __syncthreads();

  // K fragment: row 16t + fq, chunk (4kk + fg) swizzled with row & 7 == fq & 7
  int k_off[Cf::KK];
#pragma unroll
  for (int kk = 0; kk < Cf::KK; ++kk) k_off[kk] = fq * Cf::ROWB + Cf::swz(4 * kk + fg, fq) * 16;
  // V tr16 read: row R = 32kk + 16jj + 4fg + (fq >> 2), 8-byte piece (fq & 3) of d-tile n
  const int vrow = 4 * fg + (fq >> 2);
  int v_off[Cf::NT];
#pragma unroll
  for (int n = 0; n < Cf::NT; ++n)
    v_off[n] = vrow * Cf::ROWB + Cf::swz(2 * n + ((fq & 3) >> 1), vrow) * 16 + 8 * (fq & 1);

  for (int qb = wrot; qb < nt; qb += NW) {
    const int q = qb * 16 + fq;
    const int qc = min(q, S - 1);
    bf16x8 qf[Cf::KK];
#pragma unroll
    for (int kk = 0; kk < Cf::KK; ++kk) qf[kk] = qnext[kk];
    {  // prefetch the next block's Q fragments: the global-load latency hides behind this block's work
      const int qcn = min(q + 16 * NW, S - 1);
#pragma unroll
      for (int kk = 0; kk < Cf::KK; ++kk)
        qnext[kk] = *reinterpret_cast<const bf16x8*>(Qg + (size_t)qcn * ld + 32 * kk + 8 * fg);
    }

    f32x4 s[2 * KT];
#pragma unroll
    for (int t = 0; t < 2 * KT; ++t) s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    // k-step outermost: consecutive MFMAs write different tiles (no dependent-issue bubbles)
#pragma unroll
    for (int kk = 0; kk < Cf::KK; ++kk) {
#pragma unroll
      for (int t = 0; t < 2 * KT; ++t)
        if (t < nt) {
          const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sK + t * 16 * Cf::ROWB + k_off[kk]);
          s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[kk], s[t], 0, 0, 0);
        }
    }
    // ---- softmax over keys (key = 16t + 4fg + r) for query column fq; tiles t >= nt are padding
    constexpr float kLog2e = 1.4426950408889634f;
    float mx = -INFINITY;
    // keys >= klen are masked to -inf.  Only the tile that straddles klen (and padded tiles behind it) needs
    // per-element compares: the test per tile is wave-uniform.  (Written per element, the 4 nt compares are
    // loop-invariant lane masks: the compiler hoisted them into ~90 SGPRs and spilled those to VGPR lanes.)
    int klen_it = klen;
    asm volatile("" : "+s"(klen_it));
#pragma unroll
    for (int t = 0; t < 2 * KT; ++t)
      if (t < nt) {
        if (16 * t + 16 > klen_it) {
#pragma unroll
          for (int r = 0; r < 4; ++r) s[t][r] = (16 * t + 4 * fg + r < klen_it) ? s[t][r] : -INFINITY;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[t][r]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mx2 = mx * kLog2e;
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < 2 * KT; ++t)
      if (t < nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[t][r], kLog2e, -mx2));   // = exp(s - mx)
          s[t][r] = p;
          sum += p;
        }
      }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.0f / sum;
    const uint32_t rbase = (uint32_t)((b * H + h) * S + qc) * (uint32_t)S;
    // one hash per PAIR of keys (common.hpp): key k of query row q is element rbase + k; with an even row length S every
    // row starts on an even element and the lane's four consecutive keys 16 t + 4 fg + r are two whole pairs
    const uint32_t thr16 = thresh24 >> 8;
    // (a compile-time fact in the instantiation the M3P sequence runs on: left to a run-time test the compiler merges the two
    //  forms into one that computes the odd form's third hash for everybody - 101 against 91 us)
    const bool even_rows = EVENS || (S & 1) == 0;
    // keep-mask words for backward: word [qb][t][r], bit l = keep(query 16qb + (l & 15),
    // key 16t + 4(l >> 4) + r) - the compare's lane mask as it comes out of the VALU
    unsigned long long* mrow = keepmask ? keepmask + ((size_t)(b * H + h) * nt + qb) * nt * 4 : nullptr;
    // The ballot of compare (t, r) is dropped into lane (4t + r) & 63 of a register pair (v_writelane), so a
    // query block's words leave as one coalesced 8-byte-per-lane store (single-lane 16-byte stores cost 19 us).
    constexpr int MW = (8 * KT + 63) / 64;
    uint32_t mlo[MW], mhi[MW];
#pragma unroll
    for (int g = 0; g < MW; ++g) mlo[g] = mhi[g] = 0u;
    bf16x8 pf[KT];
#pragma unroll
    for (int kk = 0; kk < KT; ++kk) {
      float p[8];
      const float invk = DROP ? inv * inv_keep : inv;
      bool kq[8] = {true, true, true, true, true, true, true, true};
      if (DROP) {
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          const int t = 2 * kk + hf;
          if (t < nt) {
            const uint32_t base = rbase + (uint32_t)(16 * t + 4 * fg);
            bool k4[4];
            if (even_rows) {       // (wave-uniform; the empty asm keeps the compiler from if-converting the two forms into one
                                   //  that computes the odd form's third hash for everybody)
              asm volatile("" ::: "memory");
              const uint32_t h0 = m3p_hash32(base >> 1, seed), h1 = m3p_hash32((base >> 1) + 1u, seed);
              k4[0] = (h0 & 0xFFFFu) >= thr16; k4[1] = (h0 >> 16) >= thr16;
              k4[2] = (h1 & 0xFFFFu) >= thr16; k4[3] = (h1 >> 16) >= thr16;
            } else {
              asm volatile("" ::: "memory");
              m3p_keep_run<4>(base, seed, thresh24, k4);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) kq[4 * hf + r] = k4[r];
          }
        }
      }
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        const int t = 2 * kk + hf;
        unsigned long long kw[4] = {0ull, 0ull, 0ull, 0ull};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = 4 * hf + r;
          float v = 0.f;
          if (t < nt) {
            v = s[t][r] * invk;
            if (DROP) {
              const bool keep = kq[j];
              kw[r] = __builtin_amdgcn_ballot_w64(keep);
              v = keep ? v : 0.f;
            }
          }
          p[j] = v;
        }
        if (DROP && t < nt) {
          // the four ballots of a key tile dropped into lanes 4 t .. 4 t + 3 of the word registers by ONE statement: a
          // v_writelane that reads an SGPR a v_cmp has just written gets the stale value without wait states (measured; the
          // assembler pads nothing inside inline asm) - one s_nop 3 now serves eight writes (round 6; it was one per element)
          asm("s_nop 3\n\tv_writelane_b32 %0, %2, %10\n\tv_writelane_b32 %1, %3, %10\n\tv_writelane_b32 %0, %4, %11\n\tv_writelane_b32 %1, %5, %11\n\t"
              "v_writelane_b32 %0, %6, %12\n\tv_writelane_b32 %1, %7, %12\n\tv_writelane_b32 %0, %8, %13\n\tv_writelane_b32 %1, %9, %13"
              : "+v"(mlo[(4 * t) >> 6]), "+v"(mhi[(4 * t) >> 6])
              : "s"((uint32_t)kw[0]), "s"((uint32_t)(kw[0] >> 32)), "s"((uint32_t)kw[1]), "s"((uint32_t)(kw[1] >> 32)),
                "s"((uint32_t)kw[2]), "s"((uint32_t)(kw[2] >> 32)), "s"((uint32_t)kw[3]), "s"((uint32_t)(kw[3] >> 32)),
                "i"((4 * t) & 63), "i"((4 * t + 1) & 63), "i"((4 * t + 2) & 63), "i"((4 * t + 3) & 63));
        }
      }
      pf[kk] = bf16x8{(bf16)p[0], (bf16)p[1], (bf16)p[2], (bf16)p[3], (bf16)p[4], (bf16)p[5], (bf16)p[6], (bf16)p[7]};
    }
    if (DROP && mrow) {
#pragma unroll
      for (int g = 0; g < MW; ++g)
        if (64 * g + lane < 4 * nt) mrow[64 * g + lane] = ((unsigned long long)mhi[g] << 32) | mlo[g];
    }
    // ---- O^T[d][q] = sum_key V[key][d] P[q][key]
    f32x4 o[Cf::NT];
#pragma unroll
    for (int n = 0; n < Cf::NT; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < KT; ++kk) {
      if (kk < nk) {
#pragma unroll
        for (int n = 0; n < Cf::NT; ++n) {
          const char* pv = sV + kk * 32 * Cf::ROWB + v_off[n];
          const bf16x8 vf = cat8(lds_tr16(pv), lds_tr16(pv + 16 * Cf::ROWB));
          o[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[kk], o[n], 0, 0, 0);
        }
      }
    }
    {
      bf16x4 ob[Cf::NT];
#pragma unroll
      for (int n = 0; n < Cf::NT; ++n) ob[n] = bf16x4{(bf16)o[n][0], (bf16)o[n][1], (bf16)o[n][2], (bf16)o[n][3]};
      store_row_widened<Cf::NT>(ctx + (size_t)(b * S + min(q, S - 1)) * dmodel + h * DH, fg, q < S, ob);      // (16-byte stores)
      if (q < S && fg == 0) lse[(size_t)(b * H + h) * S + q] = mx + __logf(sum);
    }
  }
}

// ---------------------------------------------------------------------------------------
// backward
//   D[q]  = sum_d dO[q][d] O[q][d]
//   P     = exp(S - lse);  Pd = dropout(P)
//   dV    = Pd^T dO ;  dPd = dO V^T ;  dS = P * (drop'(dPd) - D)
//   dQ    = dS K (then * 1/sqrt(dh): q was stored pre-scaled) ;  dK = dS^T Q
// Phase A (a wave owns 16-key blocks, Q and dO in LDS): S = Q K^T in the un-swapped
//   orientation (lane = key column, 4 queries per tile) so P and dS feed the q-contraction
//   MFMAs of dV^T / dK^T directly from registers.
// Phase B (a wave owns 16-query blocks, K and V in LDS): the swapped orientation again
//   (lane = query column) so dS^T feeds dQ^T = K^T dS^T from registers.
// The scores are recomputed in both phases: MFMA time is cheap here, LDS transposes are not.
// ---------------------------------------------------------------------------------------
// DROP: attention dropout active (compile-time: as a runtime flag the compiler turned it into
// per-element selects over both variants).  MASK (implies DROP): keep bits from the forward pass.
// NKC: number of 32-row steps known at compile time (6 = the M3P sequence, 36 regions + 128 tokens,
// padded to 192) so both streaming loops unroll and every LDS address becomes base + immediate
// (the rolled loop spent 28 of its ~110 VALU instructions per step on address updates); 0 = runtime.
// NTC: number of 16-row tiles known at compile time as well (11 for S = 164): keep-bit word addresses become
// immediates off one pointer instead of per-tile scalar arithmetic held in (spilled) SGPRs.
// KB: 16-row blocks a wave owns per pass (1 or 2).  With 2, the streamed operand's fragments (Q / dO rows and their
// transposes in phase A, K / V in phase B) are fetched once for two owned blocks: half the LDS reads per MFMA, and two
// independent MFMA -> softmax -> MFMA chains per wave to hide each other's waits (counters, r03: the waves of this kernel
// sit in s_waitcnt 56 % of their cycles; LDS array ~45 % busy).  Costs registers: KB = 2 runs two workgroups per CU.
// ONEPASS (round 5; the M3P sequence only: NKC = 6, NTC = 11, twelve waves = ONE workgroup per CU): the scores are computed
// ONCE.  Phase A leaves dS^T - bf16, [key][query], 60.5 KB - in LDS beside Q / dO / K (all four operand tiles of the head
// are fetched once: 516 MB per launch instead of 813), and phase B is four MFMAs per 32-key step, dQ^T = K^T dS^T, both
// operands through transposing LDS reads - no second QK^T / dO V^T, no second softmax, no V tile, no Q / dO fragments.
template <int DH, int KT, bool DROP, bool MASK, int NKC, int NTC, int NW = 4, int KB = 1, int KBQ = KB, bool ONEPASS = false>
__global__ __launch_bounds__(NW * 64, NTC == 11 ? ATTN_BWD_WPS : ((NW == 8 || KB == 2) ? 2 : 3))   // NW = 4: three 49-KB workgroups per CU; 8: one ~100-KB workgroup (long S); 12 (ONEPASS): one 143-KB workgroup, three waves per SIMD
void attn_bwd_kernel(const bf16* __restrict__ qkv, const int* __restrict__ keylen, const bf16* __restrict__ ctx,
                     const bf16* __restrict__ dctx, const float* __restrict__ lse,
                     const unsigned long long* __restrict__ keepmask, bf16* __restrict__ dqkv,
                     float* __restrict__ dbias_qkv, int S, int H, int dmodel, float qscale, uint32_t seed,
                     uint32_t thresh24, float inv_keep) {
  using Cf = AttnCfg<DH>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  // block ownership rotates with the workgroup: with 11 blocks over four waves one wave owns two instead of three, and the
  // same wave id of every workgroup on a CU sits on the same SIMD - without the rotation one SIMD of four idles a third of
  // both phases while the other three carry the launch (the forward kernel does the same)
  const int wrot = (NW & (NW - 1)) ? wid : ((wid + (blockIdx.x >> 3)) & (NW - 1));
  const int nt = NTC ? NTC : ((S + 15) >> 4);
  const int nk = NKC ? NKC : ((S + 31) >> 5);
  const size_t ld = 3 * (size_t)dmodel;
  const int b_rd = b;
  const bf16* Qg = qkv + (size_t)b_rd * S * ld + h * DH;
  const bf16* Kg = Qg + dmodel;
  const bf16* Vg = Qg + 2 * dmodel;
  const bf16* Og = ctx + (size_t)b_rd * S * dmodel + h * DH;
  const bf16* dOg = dctx + (size_t)b_rd * S * dmodel + h * DH;
  bf16* dQg = dqkv + (size_t)b * S * ld + h * DH;
  bf16* dKg = dQg + dmodel;
  bf16* dVg = dQg + 2 * dmodel;
  const float* lse_bh = lse + (size_t)(b * H + h) * S;
  const int klen = keylen[b];
  // MASK: the forward pass left the dropout keep bits of this head (m3p_attn_fwd keepmask); both
  // phases then test a bit instead of re-hashing every (query, key) pair twice (~14 VALU ops each)
  const unsigned long long* mbh = MASK ? keepmask + (size_t)(b * H + h) * nt * nt * 4 : nullptr;

  // LDS: two [nk*32][DH] bf16 tiles + lse[nk*32] + D[nk*32] (fp32)
  const int tile_bytes = nk * 32 * Cf::ROWB;
  char* s0 = smem;                    // phase A: Q   | phase B: K
  char* s1 = smem + tile_bytes;       // phase A: dO  | phase B: V
  float* sL = reinterpret_cast<float*>(smem + 2 * tile_bytes);
  float* sD = sL + nk * 32;
  const int fq = lane & 15, fg = lane >> 4;
  float* sB = sD + nk * 32;           // [NW waves][3][DH] bias-gradient accumulators (q | k | v), one slot per wave
  float* sBw = sB + wid * 3 * DH;
  // ONEPASS: the K tile (staged with Q / dO, read in phase B) and dS^T [NTC * 16 keys][NTC * 16 queries] bf16 behind them.  Row
  // pitch 352 B = 11 x 32: the 16 rows x 32 B a transposing read (or phase A's store) touches then fall on distinct 32-B bank
  // groups for any eight consecutive rows.
  constexpr int DSP = NTC * 32;
  char* sK = reinterpret_cast<char*>(sB + NW * 3 * DH);
  char* sDS = sK + tile_bytes;
  static_assert(!ONEPASS || (NKC == 6 && NTC == 11 && KB == 1 && DH == 64), "ONEPASS is the M3P-sequence instantiation");
  // bias gradients = column sums of the bf16 dQ/dK/dV rows this block writes.  Each lane keeps running sums of ITS rows in
  // registers (part x d-tile x 4 columns); the reduction over the 16 lanes (fq) that hold different rows of the same columns
  // happens once per phase - four DPP adds per value - into the wave's LDS slot, and the slots are summed at the end of the
  // kernel.  (Per owned block instead - 16 registers fewer - the DPP chains and the LDS read-modify-write cost 2.6 k ticks a
  // block, r03 timeline; with ds_bpermute shuffles it was 93 of 386 us once.)  The k-bias gradient is identically zero
  // (softmax is invariant to a per-query shift of the scores, so sum_key dS[q][key] = 0): it is written as exact 0 instead of
  // the rounding noise a column sum of bf16 dK rows would give.
  f32x4 bsum[Cf::NT];       // phase A: v-bias sums, flushed to LDS, then reused for q in phase B
#pragma unroll
  for (int n = 0; n < Cf::NT; ++n) bsum[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto bias_acc = [&](int, int n, const bf16x4& v4) {
    bsum[n] += f32x4{(float)v4[0], (float)v4[1], (float)v4[2], (float)v4[3]};
  };
  auto bias_flush = [&](int part) {
#pragma unroll
    for (int n = 0; n < Cf::NT; ++n) {
      f32x4 x = bsum[n];
#pragma unroll
      for (int r = 0; r < 4; ++r) x[r] = row16_sum(x[r]);
      if (fq == 0) *reinterpret_cast<f32x4*>(sBw + part * DH + 16 * n + 4 * fg) = x;
      bsum[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };

  int r_off[Cf::KK];   // row-major fragment (row 16t + fq, chunk 4kk + fg)
#pragma unroll
  for (int kk = 0; kk < Cf::KK; ++kk) r_off[kk] = fq * Cf::ROWB + Cf::swz(4 * kk + fg, fq) * 16;
  const int trow = 4 * fg + (fq >> 2);
  int t_off[Cf::NT];   // tr16 read (row R = 32kk + 16jj + trow, d-tile n)
#pragma unroll
  for (int n = 0; n < Cf::NT; ++n)
    t_off[n] = trow * Cf::ROWB + Cf::swz(2 * n + ((fq & 3) >> 1), trow) * 16 + 8 * (fq & 1);

  // 16-row tile t lies wholly behind the sequence (S = 164: the 12th tile, rows 176..191, of the six 32-row steps):
  // with the tile count known at compile time the code for it simply is not generated; as a run-time test it was
  // only worth it without the keep-bit words (measured slower with them)
#define PAD_TILE(t) (NTC ? (t) >= NTC : (!MASK && (t) >= nt))
  constexpr float kLog2e = 1.4426950408889634f;
  constexpr float kMasked = -1.0e30f;    // score of a masked key: exp2 of it is exactly 0
  // Q and dO tiles are requested first (LDS-DMA, asynchronous), then this wave's first K / V fragments (they do not depend on
  // LDS).  D[q] = rowsum(dO * O) is taken from the dO rows THIS wave staged (a wave may read its own LDS-DMA rows after its own
  // vmcnt(0), no barrier needed) times the matching O chunks fetched from global beside them: dO is read from HBM once
  // instead of twice (r03: 818 MB per launch against 516 MB algorithmic) and all waves share the work.
  constexpr bool kDfromLds = NKC != 0;
  constexpr int kStageInstr = NKC * 32 / Cf::RPI;                       // LDS-DMA instructions per tile
  constexpr int kNIW = kDfromLds ? (kStageInstr + NW - 1) / NW : 1;     // ... of which this wave issues at most
  bf16x8 orow[kNIW];
  if (kDfromLds) {
    const int rin = lane / Cf::CH, c = lane % Cf::CH;
#pragma unroll
    for (int j = 0; j < kNIW; ++j) {
      const int row = (wid + j * NW) * Cf::RPI + rin;                   // (same row / chunk as this lane's piece of stage_rows)
      orow[j] = *reinterpret_cast<const bf16x8*>(Og + (size_t)min(row, S - 1) * dmodel + Cf::swz(c, row) * 8);
    }
  }
  stage_rows<DH>(Qg, ld, S, nk * 32, s0, wid, lane, NW);
  stage_rows<DH>(dOg, (size_t)dmodel, S, nk * 32, s1, wid, lane, NW);
  if (ONEPASS) stage_rows<DH>(Kg, ld, S, nk * 32, sK, wid, lane, NW);      // (behind dO: the D prologue waits for this wave's dO rows with vmcnt(0) anyway)
  bf16x8 kf[KB][Cf::KK], vf[KB][Cf::KK];
  auto load_kv = [&](int u, int kb) {
    const int keyc = min(kb * 16 + fq, S - 1);
#pragma unroll
    for (int kk = 0; kk < Cf::KK; ++kk) {
      kf[u][kk] = *reinterpret_cast<const bf16x8*>(Kg + (size_t)keyc * ld + 32 * kk + 8 * fg);
      vf[u][kk] = *reinterpret_cast<const bf16x8*>(Vg + (size_t)keyc * ld + 32 * kk + 8 * fg);
    }
  };
  // (not with dropout re-hashed instead of read from the forward's keep bits: that variant has no registers to spare)
  constexpr bool kNextFrag = NKC != 0 && NTC != 0 && !(DROP && !MASK);      // (nor the less specialised instantiations: they spill with 16 more)
  bf16x8 kfn[KB][Cf::KK], vfn[KB][Cf::KK];     // the next owned block's, in flight while this one is computed
  auto load_kv_next = [&](int u, int kb) {
    const int keyc = min(kb * 16 + fq, S - 1);
#pragma unroll
    for (int kk = 0; kk < Cf::KK; ++kk) {
      kfn[u][kk] = *reinterpret_cast<const bf16x8*>(Kg + (size_t)keyc * ld + 32 * kk + 8 * fg);
      vfn[u][kk] = *reinterpret_cast<const bf16x8*>(Vg + (size_t)keyc * ld + 32 * kk + 8 * fg);
    }
  };
  if (wrot * KB < nt) {
#pragma unroll
    for (int u = 0; u < KB; ++u) load_kv(u, wrot * KB + u);
  }
  // ---- prologue: D[q] = rowsum(dO * O), lse -> LDS (padded rows: D = 0, lse = +inf so P = 0)
  const float log2_inv_keep = DROP ? __builtin_amdgcn_logf(inv_keep) : 0.f;     // (v_log_f32 is log2)
  const float keep_prob = DROP ? __builtin_amdgcn_rcpf(inv_keep) : 1.f;
  for (int q = tid; q < nk * 32; q += NW * 64) {
    float dsum = 0.f, l = INFINITY;
    if (q < S) {
      if (!kDfromLds) {
        const bf16* op = Og + (size_t)q * dmodel;
        const bf16* dp = dOg + (size_t)q * dmodel;
#pragma unroll
        for (int c = 0; c < DH / 8; ++c) {
          const bf16x8 ov = *reinterpret_cast<const bf16x8*>(op + 8 * c);
          const bf16x8 dv = *reinterpret_cast<const bf16x8*>(dp + 8 * c);
#pragma unroll
          for (int e = 0; e < 8; ++e) dsum += (float)ov[e] * (float)dv[e];
        }
      }
      // probabilities are rebuilt as exp2(S log2e - lse log2e): fma + v_exp.  With dropout the rebuilt value is p / keep
      // (log2(1 / keep) folded into the stored lse) and D is stored as D * keep: Pd = (p / keep) [kept], dS = Pd dPd - (p / keep) (D keep)
      l = lse_bh[q] * kLog2e - log2_inv_keep;
    }
    if (!kDfromLds) sD[q] = dsum * keep_prob;
    sL[q] = l;
  }
  if (kDfromLds) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this wave's LDS-DMA rows (and its O chunks) have landed
    const int rin = lane / Cf::CH, c = lane % Cf::CH;
#pragma unroll
    for (int j = 0; j < kNIW; ++j) {
      const int i = wid + j * NW;
      if (i < kStageInstr) {
        const bf16x8 dv = *reinterpret_cast<const bf16x8*>(s1 + i * 1024 + lane * 16);
        float part = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) part += (float)orow[j][e] * (float)dv[e];
        part = chunks_sum<Cf::CH>(part);
        const int row = i * Cf::RPI + rin;
        if (c == 0) sD[row] = row < S ? part * keep_prob : 0.f;
      }
    }
  }
  // ================= phase A: dV, dK (wave owns key blocks) =================
  __syncthreads();

  // keep-bit words of a step are requested two steps ahead (unrolled steps only: the buffers alternate at compile time): the
  // words are read once per launch, so every one of them is an L2 miss the step would otherwise wait for in full
  constexpr bool kPreA = MASK && NKC != 0;
  unsigned long long mwA[2][KB][2];
  auto mask_words_A = [&](int kb0_, int kq_, int par) {
#pragma unroll
    for (int u = 0; u < KB; ++u)
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
        mwA[par][u][hf] = mbh[((size_t)min(2 * kq_ + hf, nt - 1) * nt + min(kb0_ + u, nt - 1)) * 4 + (fq & 3)];
  };
  if (kPreA) {
    mask_words_A(wrot * KB, 0, 0);
    mask_words_A(wrot * KB, 1, 1);
  }
  for (int kb0 = wrot * KB; kb0 < nt; kb0 += NW * KB) {
    // (an owned block behind the last key tile - odd tile counts with KB = 2 - runs as an all-masked block: p = 0, nothing stored)
    int key[KB], keyc[KB];
    float kbias[KB];
#pragma unroll
    for (int u = 0; u < KB; ++u) {
      key[u] = (kb0 + u) * 16 + fq;            // this lane's key column
      keyc[u] = min(key[u], S - 1);
      kbias[u] = (key[u] < klen) ? 0.f : kMasked;
      if (kNextFrag) {
        if (kb0 != wrot * KB) {
#pragma unroll
          for (int kk = 0; kk < Cf::KK; ++kk) { kf[u][kk] = kfn[u][kk]; vf[u][kk] = vfn[u][kk]; }
        }
        if (kb0 + NW * KB < nt) load_kv_next(u, kb0 + NW * KB + u);
      } else if (kb0 != wrot * KB) {
        load_kv(u, kb0 + u);
      }
    }
    // dV^T[d][key] = sum_q dO[q][d] Pd[q][key] ; dK^T[d][key] = sum_q Q[q][d] dS[q][key]
    // streamed over 32-query steps: P / dS of a step are produced (lane = key column, query
    // 16t + 4fg + r) and consumed as MFMA B operands at once — nothing S x S is held
    f32x4 dv[KB][Cf::NT], dk[KB][Cf::NT];
#pragma unroll
    for (int u = 0; u < KB; ++u)
#pragma unroll
      for (int n = 0; n < Cf::NT; ++n) dv[u][n] = dk[u][n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll(NKC ? NKC : 1)
    for (int kq = 0; kq < nk; ++kq) {
      // the MFMA chains of a step (scores and dPd of both 16-query tiles, of every owned block) are issued interleaved,
      // k-step outermost, so that no MFMA waits on the one just issued
      f32x4 scA[KB][2], dpA[KB][2], dnegA[2];
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        const int t = 2 * kq + hf;
        // a masked key column starts its score accumulator at -1e30 (no per-element select);
        // without dropout dPd - D comes straight out of the MFMA (accumulator starts at -D[q])
        dnegA[hf] = f32x4{-sD[16 * t + 4 * fg + 0], -sD[16 * t + 4 * fg + 1], -sD[16 * t + 4 * fg + 2],
                          -sD[16 * t + 4 * fg + 3]};
#pragma unroll
        for (int u = 0; u < KB; ++u) {
          scA[u][hf] = f32x4{kbias[u], kbias[u], kbias[u], kbias[u]};
          dpA[u][hf] = DROP ? f32x4{0.f, 0.f, 0.f, 0.f} : dnegA[hf];
        }
      }
#pragma unroll
      for (int kk = 0; kk < Cf::KK; ++kk) {
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          const int t = 2 * kq + hf;
          if (PAD_TILE(t)) continue;   // query tile that is pure padding (S = 164: rows 176..191)
          const bf16x8 qf = *reinterpret_cast<const bf16x8*>(s0 + t * 16 * Cf::ROWB + r_off[kk]);
          const bf16x8 df = *reinterpret_cast<const bf16x8*>(s1 + t * 16 * Cf::ROWB + r_off[kk]);
#pragma unroll
          for (int u = 0; u < KB; ++u) {
            scA[u][hf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf, kf[u][kk], scA[u][hf], 0, 0, 0);   // S[q][key]
            dpA[u][hf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(df, vf[u][kk], dpA[u][hf], 0, 0, 0);   // dPd[q][key]
          }
        }
      }
      bf16x8 pfrag[KB], sfrag[KB];
#pragma unroll
      for (int u = 0; u < KB; ++u) {
        f32x4 pd2[2], ds2[2];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          const int t = 2 * kq + hf;
          if (PAD_TILE(t)) {      // (skipping the padded tile measured slower with MASK): contributes zeros
            pd2[hf] = ds2[hf] = f32x4{0.f, 0.f, 0.f, 0.f};
            continue;
          }
          const f32x4 dneg = dnegA[hf], sc = scA[u][hf], dp = dpA[u][hf];
          uint32_t kbits = 0;
          if (MASK) {
            // forward layout: word [qb = t][tile = kb][r = key & 3], bit (q & 15) + 16 ((key & 15) >> 2)
            const unsigned long long w = kPreA ? mwA[kq & 1][u][hf]
                                               : mbh[((size_t)min(t, nt - 1) * nt + min(kb0 + u, nt - 1)) * 4 + (fq & 3)];
            kbits = (uint32_t)(w >> (4 * fg + 16 * (fq >> 2)));
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int q = 16 * t + 4 * fg + r;
            const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[r], kLog2e, -sL[q]));   // padded q: lse = +inf -> 0
            if (DROP) {      // p = P / keep here, dneg = -D keep
              float pd;
              if (MASK) {
                pd = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, p) & bit_to_mask(kbits, r));
              } else {
                static_assert(MASK || !DROP, "dropout in backward reads the forward pass's keep words");
                pd = p;
              }
              pd2[hf][r] = pd;
              ds2[hf][r] = __builtin_fmaf(pd, dp[r], p * dneg[r]);
            } else {
              pd2[hf][r] = p;
              ds2[hf][r] = p * dp[r];
            }
          }
        }
        pfrag[u] = bf16x8{(bf16)pd2[0][0], (bf16)pd2[0][1], (bf16)pd2[0][2], (bf16)pd2[0][3],
                          (bf16)pd2[1][0], (bf16)pd2[1][1], (bf16)pd2[1][2], (bf16)pd2[1][3]};
        sfrag[u] = bf16x8{(bf16)ds2[0][0], (bf16)ds2[0][1], (bf16)ds2[0][2], (bf16)ds2[0][3],
                          (bf16)ds2[1][0], (bf16)ds2[1][1], (bf16)ds2[1][2], (bf16)ds2[1][3]};
      }
      if constexpr (ONEPASS) {
        // dS^T[key = 16 kb0 + fq][query = 16 t + 4 fg + r] - this lane's four values of a tile are four consecutive queries of
        // its key row: one 8-byte LDS store per tile
        if (kb0 < NTC) {
#pragma unroll
          for (int hf = 0; hf < 2; ++hf) {
            if (PAD_TILE(2 * kq + hf)) continue;
            const bf16x4 d4 = hf ? bf16x4{sfrag[0][4], sfrag[0][5], sfrag[0][6], sfrag[0][7]}
                                 : bf16x4{sfrag[0][0], sfrag[0][1], sfrag[0][2], sfrag[0][3]};
            *reinterpret_cast<bf16x4*>(sDS + (kb0 * 16 + fq) * DSP + (32 * kq + 16 * hf + 4 * fg) * 2) = d4;
          }
        }
      }
      if (kPreA) {      // (behind the last step of a block: the first steps of the next owned block, clamped on the last one)
        if (kq + 2 < nk) mask_words_A(kb0, kq + 2, kq & 1);
        else mask_words_A(kb0 + NW * KB, kq + 2 - nk, kq & 1);
      }
#pragma unroll
      for (int n = 0; n < Cf::NT; ++n) {
        const char* pq = s0 + kq * 32 * Cf::ROWB + t_off[n];
        const char* pdo = s1 + kq * 32 * Cf::ROWB + t_off[n];
        const bf16x8 qT = cat8(lds_tr16(pq), lds_tr16(pq + 16 * Cf::ROWB));
        const bf16x8 dT = cat8(lds_tr16(pdo), lds_tr16(pdo + 16 * Cf::ROWB));
#pragma unroll
        for (int u = 0; u < KB; ++u) {
          dv[u][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dT, pfrag[u], dv[u][n], 0, 0, 0);
          dk[u][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qT, sfrag[u], dk[u][n], 0, 0, 0);
        }
      }
      if (NKC) __builtin_amdgcn_sched_barrier(0);   // unrolled steps stay in order: no register blow-up from hoisted loads
    }
#pragma unroll
    for (int u = 0; u < KB; ++u) {
      bf16x4 kb4[Cf::NT], vb4[Cf::NT];
#pragma unroll
      for (int n = 0; n < Cf::NT; ++n) {
        kb4[n] = bf16x4{(bf16)dk[u][n][0], (bf16)dk[u][n][1], (bf16)dk[u][n][2], (bf16)dk[u][n][3]};
        vb4[n] = bf16x4{(bf16)dv[u][n][0], (bf16)dv[u][n][1], (bf16)dv[u][n][2], (bf16)dv[u][n][3]};
      }
      const bool ok = key[u] < S;
      if (dbias_qkv) {   // (rows >= S contribute zeros; the shuffles need all 64 lanes)
#pragma unroll
        for (int n = 0; n < Cf::NT; ++n) bias_acc(2, n, ok ? vb4[n] : bf16x4{0, 0, 0, 0});
      }
      store_row_widened<Cf::NT>(dKg + (size_t)keyc[u] * ld, fg, ok, kb4);      // (16-byte stores: see store_row_widened)
      store_row_widened<Cf::NT>(dVg + (size_t)keyc[u] * ld, fg, ok, vb4);
    }
  }
  if (dbias_qkv) bias_flush(2);
  __syncthreads();   // everyone done with Q / dO tiles

  if constexpr (ONEPASS) {
    // ================= phase B, one-pass form: dQ^T[d][q] = sum_key K^T[d][key] dS^T[key][q] =================
    // A operand: K^T through transposing reads of the K tile (rows = keys), B operand: dS^T through transposing reads of the
    // tile phase A left (rows = keys, this wave's 16 query columns) - lane fq holds query column fq, keys 4 fg + r of both
    // 16-key tiles of the step, exactly the contraction order of the K^T fragment.
    for (int qb = wid; qb < nt; qb += NW) {
      f32x4 dq[Cf::NT];
#pragma unroll
      for (int n = 0; n < Cf::NT; ++n) dq[n] = f32x4{0.f, 0.f, 0.f, 0.f};
      const char* pds = sDS + trow * DSP + qb * 32 + (fq & 3) * 8;
#pragma unroll
      for (int kq = 0; kq < NKC; ++kq) {
        const bf16x4 lo = lds_tr16(pds + (32 * kq) * DSP);
        const bf16x4 hi = PAD_TILE(2 * kq + 1) ? bf16x4{0, 0, 0, 0} : lds_tr16(pds + (32 * kq + 16) * DSP);
        const bf16x8 sfr = cat8(lo, hi);
#pragma unroll
        for (int n = 0; n < Cf::NT; ++n) {
          const char* pk = sK + kq * 32 * Cf::ROWB + t_off[n];
          const bf16x8 kT = cat8(lds_tr16(pk), lds_tr16(pk + 16 * Cf::ROWB));
          dq[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kT, sfr, dq[n], 0, 0, 0);
        }
      }
      const int q = qb * 16 + fq;
      bf16x4 qb4[Cf::NT];
#pragma unroll
      for (int n = 0; n < Cf::NT; ++n)
        qb4[n] = bf16x4{(bf16)(dq[n][0] * qscale), (bf16)(dq[n][1] * qscale), (bf16)(dq[n][2] * qscale), (bf16)(dq[n][3] * qscale)};
      if (dbias_qkv) {
#pragma unroll
        for (int n = 0; n < Cf::NT; ++n) bias_acc(0, n, q < S ? qb4[n] : bf16x4{0, 0, 0, 0});
      }
      store_row_widened<Cf::NT>(dQg + (size_t)min(q, S - 1) * ld, fg, q < S, qb4);
    }
  } else {
  // ================= phase B: dQ (wave owns query blocks) =================
  stage_rows<DH>(Kg, ld, S, nk * 32, s0, wid, lane, NW);
  stage_rows<DH>(Vg, ld, S, nk * 32, s1, wid, lane, NW);
  bf16x8 qf[KBQ][Cf::KK], df[KBQ][Cf::KK];
  auto load_qd = [&](int u, int qb) {
    const int qc = min(qb * 16 + fq, S - 1);
#pragma unroll
    for (int kk = 0; kk < Cf::KK; ++kk) {
      qf[u][kk] = *reinterpret_cast<const bf16x8*>(Qg + (size_t)qc * ld + 32 * kk + 8 * fg);
      df[u][kk] = *reinterpret_cast<const bf16x8*>(dOg + (size_t)qc * dmodel + 32 * kk + 8 * fg);
    }
  };
  bf16x8 qfn[KBQ][Cf::KK], dfn[KBQ][Cf::KK];
  auto load_qd_next = [&](int u, int qb) {
    const int qc = min(qb * 16 + fq, S - 1);
#pragma unroll
    for (int kk = 0; kk < Cf::KK; ++kk) {
      qfn[u][kk] = *reinterpret_cast<const bf16x8*>(Qg + (size_t)qc * ld + 32 * kk + 8 * fg);
      dfn[u][kk] = *reinterpret_cast<const bf16x8*>(dOg + (size_t)qc * dmodel + 32 * kk + 8 * fg);
    }
  };
  if (wrot * KBQ < nt) {
#pragma unroll
    for (int u = 0; u < KBQ; ++u) load_qd(u, wrot * KBQ + u);
  }
  __syncthreads();

  for (int qb0 = wrot * KBQ; qb0 < nt; qb0 += NW * KBQ) {
    int q[KBQ], qc[KBQ];
    float lq[KBQ], dq_[KBQ];      // lse (log2 units) and D of this lane's queries (a block behind the last tile: lse = +inf -> p = 0)
    uint32_t rbase[KBQ];
#pragma unroll
    for (int u = 0; u < KBQ; ++u) {
      q[u] = (qb0 + u) * 16 + fq;
      qc[u] = min(q[u], S - 1);
      if (kNextFrag) {
        if (qb0 != wrot * KBQ) {
#pragma unroll
          for (int kk = 0; kk < Cf::KK; ++kk) { qf[u][kk] = qfn[u][kk]; df[u][kk] = dfn[u][kk]; }
        }
        if (qb0 + NW * KBQ < nt) load_qd_next(u, qb0 + NW * KBQ + u);
      } else if (qb0 != wrot * KBQ) {
        load_qd(u, qb0 + u);
      }
      const bool in = q[u] < nk * 32;
      lq[u] = in ? sL[min(q[u], nk * 32 - 1)] : INFINITY;
      dq_[u] = in ? sD[min(q[u], nk * 32 - 1)] : 0.f;
      rbase[u] = (uint32_t)((b * H + h) * S + qc[u]) * (uint32_t)S;
    }
    int klen_it = klen;
    asm volatile("" : "+s"(klen_it));   // opaque per query block: keeps the key-mask tests inside the loop
    // keep-bit words (wave-uniform: scalar loads, one s_load_dwordx16 per step) are requested one step ahead.  (They share
    // lgkmcnt with the LDS reads and return out of order, so the next LDS wait still waits for them; fetching them with a vector
    // load, a dword per lane, and v_readlane at the use measured slower: 219 us against 211.)
    constexpr bool kPreB = MASK && NKC != 0;
    unsigned long long mwB[2][KBQ][2][4];
    auto mask_words_B = [&](int kq_, int par) {
#pragma unroll
      for (int u = 0; u < KBQ; ++u)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          const unsigned long long* mw_ = mbh + ((size_t)min(qb0 + u, nt - 1) * nt + min(2 * kq_ + hf, nt - 1)) * 4;
#pragma unroll
          for (int r = 0; r < 4; ++r) mwB[par][u][hf][r] = mw_[r];
        }
    };
    if (kPreB) mask_words_B(0, 0);
    // dQ^T[d][q] = sum_key K[key][d] dS[q][key], streamed over 32-key steps
    f32x4 dq[KBQ][Cf::NT];
#pragma unroll
    for (int u = 0; u < KBQ; ++u)
#pragma unroll
      for (int n = 0; n < Cf::NT; ++n) dq[u][n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll(NKC ? NKC : 1)
    for (int kq = 0; kq < nk; ++kq) {
      if (kPreB && kq + 1 < nk) mask_words_B(kq + 1, (kq + 1) & 1);
      f32x4 scB[KBQ][2], dpB[KBQ][2];
#pragma unroll
      for (int u = 0; u < KBQ; ++u)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          scB[u][hf] = f32x4{0.f, 0.f, 0.f, 0.f};
          dpB[u][hf] = DROP ? f32x4{0.f, 0.f, 0.f, 0.f} : f32x4{-dq_[u], -dq_[u], -dq_[u], -dq_[u]};
        }
#pragma unroll
      for (int kk = 0; kk < Cf::KK; ++kk) {
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          const int t = 2 * kq + hf;
          if (PAD_TILE(t)) continue;   // key tile beyond the sequence
          const bf16x8 kfr = *reinterpret_cast<const bf16x8*>(s0 + t * 16 * Cf::ROWB + r_off[kk]);
          const bf16x8 vfr = *reinterpret_cast<const bf16x8*>(s1 + t * 16 * Cf::ROWB + r_off[kk]);
#pragma unroll
          for (int u = 0; u < KBQ; ++u) {
            scB[u][hf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfr, qf[u][kk], scB[u][hf], 0, 0, 0);   // S^T[key][q]
            dpB[u][hf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vfr, df[u][kk], dpB[u][hf], 0, 0, 0);   // dPd^T[key][q]
          }
        }
      }
      bf16x8 sfrag[KBQ];
#pragma unroll
      for (int u = 0; u < KBQ; ++u) {
        f32x4 ds2[2];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          const int t = 2 * kq + hf;
          if (PAD_TILE(t)) {
            ds2[hf] = f32x4{0.f, 0.f, 0.f, 0.f};
            continue;
          }
          f32x4 sc = scB[u][hf];
          const f32x4 dp = dpB[u][hf];
          const unsigned long long* mw = MASK ? mbh + ((size_t)min(qb0 + u, nt - 1) * nt + min(t, nt - 1)) * 4 : nullptr;   // wave-uniform
          // keys >= klen: only the tile straddling klen (or behind it) needs per-element tests (wave-uniform branch;
          // per-element compares are loop-invariant lane masks the compiler hoists into spilled SGPRs)
          if (16 * t + 16 > klen_it) {
            asm volatile("");   // (keeps this a branch: if-converted it is 2 VALU ops on every element)
#pragma unroll
            for (int r = 0; r < 4; ++r) sc[r] = (16 * t + 4 * fg + r < klen_it) ? sc[r] : kMasked;
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int key = 16 * t + 4 * fg + r;
            const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[r], kLog2e, -lq[u]));
            if (DROP) {
              float kfac;      // 1 if kept, else 0 (p = P / keep here, dq_ = D keep)
              if (MASK) {
                // this lane's own bit of the forward ballot: the 64-bit word IS the select mask
                asm("v_cndmask_b32_e64 %0, 0, 1.0, %1" : "=v"(kfac) : "s"(kPreB ? mwB[kq & 1][u][hf][r] : mw[r]));
              } else {
                static_assert(MASK || !DROP, "dropout in backward reads the forward pass's keep words");
                kfac = 1.f;
              }
              ds2[hf][r] = p * __builtin_fmaf(dp[r], kfac, -dq_[u]);
            } else {
              ds2[hf][r] = p * dp[r];
            }
          }
        }
        sfrag[u] = bf16x8{(bf16)ds2[0][0], (bf16)ds2[0][1], (bf16)ds2[0][2], (bf16)ds2[0][3],
                          (bf16)ds2[1][0], (bf16)ds2[1][1], (bf16)ds2[1][2], (bf16)ds2[1][3]};
      }
#pragma unroll
      for (int n = 0; n < Cf::NT; ++n) {
        const char* pk = s0 + kq * 32 * Cf::ROWB + t_off[n];
        const bf16x8 kT = cat8(lds_tr16(pk), lds_tr16(pk + 16 * Cf::ROWB));
#pragma unroll
        for (int u = 0; u < KBQ; ++u) dq[u][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kT, sfrag[u], dq[u][n], 0, 0, 0);
      }
      if (NKC) __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int u = 0; u < KBQ; ++u) {
      bf16x4 qb4[Cf::NT];
#pragma unroll
      for (int n = 0; n < Cf::NT; ++n)
        qb4[n] = bf16x4{(bf16)(dq[u][n][0] * qscale), (bf16)(dq[u][n][1] * qscale), (bf16)(dq[u][n][2] * qscale), (bf16)(dq[u][n][3] * qscale)};
      const bool ok = q[u] < S;
      if (dbias_qkv) {
#pragma unroll
        for (int n = 0; n < Cf::NT; ++n) bias_acc(0, n, ok ? qb4[n] : bf16x4{0, 0, 0, 0});
      }
      store_row_widened<Cf::NT>(dQg + (size_t)qc[u] * ld, fg, ok, qb4);
    }
  }
  }      // (two-phase form)

  // ---- bias gradients: column sums of the bf16 dQ / dV rows this block wrote (k: zero, see above)
  if (dbias_qkv) {
    bias_flush(0);
    __syncthreads();
    for (int i = tid; i < 3 * DH; i += NW * 64) {
      const int part = i / DH, c = i - part * DH;
      if (part != 1) {
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) tot += sB[w * 3 * DH + i];
        atomicAdd(dbias_qkv + part * dmodel + h * DH + c, tot);
      }
    }
  }
}

#undef PAD_TILE

// ---------------------------------------------------------------------------------------
// backward, PERSISTENT one-pass form for the M3P sequence (round 5): 64-wide heads, 36 regions + 128 tokens = 11 tiles /
// 6 steps, keep bits from the forward pass (or no dropout).  One twelve-wave workgroup per CU walks its share of the
// (batch, head) pairs; per head
//   [D = rowsum(dO O), lse -> LDS] B1 [K tile requested; phase A: each wave one 16-key block - S, dPd once, P / dS, dV, dK,
//   dS^T -> LDS] B2 [dK / dV stored; the NEXT head's Q / dO tiles, O chunks, K / V fragments, lse, keep words requested;
//   phase B: each wave one 16-query block, dQ^T = K^T dS^T, four MFMAs per 32-key step].
// What the timeline of the plain one-pass kernel (profiles/r05_attn_bwd_onepass_timeline.txt) showed: of 31.5 k ticks a head
// spends in its workgroup, 12.4 k are the two phases - the rest is the prologue's memory latency (11.1 k), barriers that wait
// for global STORES (__syncthreads' vmcnt(0): 5.4 k) and the exit (2.6 k), none of which three independent four-wave
// workgroups per CU hid any worse.  Here the next head's loads fly under phase B and the K tile's under phase A, the barriers
// wait for LDS only, and the stores are never waited for inside the loop.
// ---------------------------------------------------------------------------------------
template <bool DROP, bool MASK>
__global__ __launch_bounds__(768, 3)
void attn_bwd_p_kernel(const bf16* __restrict__ qkv, const int* __restrict__ keylen, const bf16* __restrict__ ctx,
                       const bf16* __restrict__ dctx, const float* __restrict__ lse,
                       const unsigned long long* __restrict__ keepmask, bf16* __restrict__ dqkv,
                       float* __restrict__ dbias_qkv, int S, int H, int dmodel, int nheads, float qscale, float inv_keep) {
  constexpr int DH = 64, NW = 12, NKC = 6, NTC = 11, NR = NKC * 32;
  using Cf = AttnCfg<DH>;
  constexpr int DSP = NTC * 32;                      // row pitch of dS^T: 352 B (see attn_bwd_kernel, ONEPASS)
  constexpr int TILE = NR * Cf::ROWB;                // 24 576 B
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  char* s0 = smem;                                   // Q
  char* s1 = s0 + TILE;                              // dO
  char* sK = s1 + TILE;                              // K (phase B)
  char* sDS = sK + TILE;                             // dS^T [176 keys][176 queries] bf16
  float* sL = reinterpret_cast<float*>(sDS + NTC * 16 * DSP);
  float* sD = sL + NR;
  float* sB = sD + NR;                               // [2 heads in flight][NW][3][DH] bias-gradient partial sums
  // the head's dropout keep words of this wave's key tile: [NW][11 query tiles x 4] - ONE 8-byte load per lane and head (lane
  // 4 t + r fetches word (t, r)) parked here, instead of two loads per step (vector-memory ISSUE is what the CU runs short of)
  unsigned long long* sMW = reinterpret_cast<unsigned long long*>(sB + 2 * NW * 3 * DH) + wid * 48;
  const size_t ld = 3 * (size_t)dmodel;
  const int fq = lane & 15, fg = lane >> 4;
  const int rin = lane / Cf::CH, c8 = lane % Cf::CH;
  int r_off[Cf::KK];
#pragma unroll
  for (int kk = 0; kk < Cf::KK; ++kk) r_off[kk] = fq * Cf::ROWB + Cf::swz(4 * kk + fg, fq) * 16;
  const int trow = 4 * fg + (fq >> 2);
  int t_off[Cf::NT];
#pragma unroll
  for (int n = 0; n < Cf::NT; ++n)
    t_off[n] = trow * Cf::ROWB + Cf::swz(2 * n + ((fq & 3) >> 1), trow) * 16 + 8 * (fq & 1);
  constexpr float kLog2e = 1.4426950408889634f;
  constexpr float kMasked = -1.0e30f;
  const float log2_inv_keep = DROP ? __builtin_amdgcn_logf(inv_keep) : 0.f;
  const float keep_prob = DROP ? __builtin_amdgcn_rcpf(inv_keep) : 1.f;
  constexpr int kStageInstr = NR / Cf::RPI;                       // 24 LDS-DMA instructions per tile
  constexpr int kNIW = (kStageInstr + NW - 1) / NW;               // 2 of them per wave
#define PAD_TILE(t) ((t) >= NTC)

  // ---- what a head needs from global memory before its phase A; requested a head ahead
  bf16x8 orow[kNIW], kf[Cf::KK], vf[Cf::KK];
  float lse_r = 0.f;
  unsigned long long mw_req = 0;
  auto request_head = [&](int hd) {
    const int b = hd / H, h = hd - b * H;
    const bf16* Qg = qkv + (size_t)b * S * ld + h * DH;
    const bf16* Og = ctx + (size_t)b * S * dmodel + h * DH;
    const bf16* dOg = dctx + (size_t)b * S * dmodel + h * DH;
#pragma unroll
    for (int j = 0; j < kNIW; ++j) {
      const int row = (wid + j * NW) * Cf::RPI + rin;
      orow[j] = *reinterpret_cast<const bf16x8*>(Og + (size_t)min(row, S - 1) * dmodel + Cf::swz(c8, row) * 8);
    }
    stage_rows_hidden<DH>(Qg, ld, S, NR, s0, wid, lane, NW);
    stage_rows_hidden<DH>(dOg, (size_t)dmodel, S, NR, s1, wid, lane, NW);
    const int keyc = min(min(wid, NTC - 1) * 16 + fq, S - 1);
#pragma unroll
    for (int kk = 0; kk < Cf::KK; ++kk) {
      kf[kk] = *reinterpret_cast<const bf16x8*>(Qg + dmodel + (size_t)keyc * ld + 32 * kk + 8 * fg);
      vf[kk] = *reinterpret_cast<const bf16x8*>(Qg + 2 * dmodel + (size_t)keyc * ld + 32 * kk + 8 * fg);
    }
    if (tid < NR && tid < S) lse_r = lse[(size_t)hd * S + tid];      // (raw: arithmetic on it here would wait for the load here)
    if (MASK && lane < 4 * NTC)
      mw_req = keepmask[(size_t)hd * NTC * NTC * 4 + ((size_t)(lane >> 2) * NTC + min(wid, NTC - 1)) * 4 + (lane & 3)];
  };

  f32x4 bsum[Cf::NT];
#pragma unroll
  for (int n = 0; n < Cf::NT; ++n) bsum[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto bias_acc = [&](int n, const bf16x4& v4) { bsum[n] += f32x4{(float)v4[0], (float)v4[1], (float)v4[2], (float)v4[3]}; };
  // Column sums of the 16 values a lane holds over its DPP row (the 16 lanes of one fg), as a HALVING butterfly (round 6: the two
  // flushes per head were 23 % of this kernel's VALU instructions - 64 v_mov_dpp + 32 v_pk_add each - for 128 floats,
  // profiles/r06_attn_bwd_ablation.txt): in each of the first two stages a lane keeps only the half of the values its row
  // position selects - lanes 8..15 the tiles n = 2, 3 (partner: lane + 8), then lanes of odd 4-lane banks the odd tile (partner:
  // half-mirror) - one bank-masked v_add_f32_dpp per kept value and side; the last two stages are plain quad butterflies on the
  // four values left.  16 + 8 + 4 + 4 adds instead of 64 + 32; lanes 0 / 4 / 8 / 12 of a row end with tiles 0 / 1 / 2 / 3.
  auto bias_flush = [&](float* slot, int part) {
    float t[2][4], u[4];
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        asm volatile("v_add_f32_dpp %0, %1, %1 row_ror:8 row_mask:0xf bank_mask:0x3" : "=v"(t[n][r]) : "v"(bsum[n][r]));
        asm volatile("v_add_f32_dpp %0, %1, %1 row_ror:8 row_mask:0xf bank_mask:0xc" : "+v"(t[n][r]) : "v"(bsum[n + 2][r]));
      }
    asm volatile("s_nop 1");      // (a VALU result read through DPP: two wait states - the compiler does not see into the asm)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      asm volatile("v_add_f32_dpp %0, %1, %1 row_half_mirror row_mask:0xf bank_mask:0x5" : "=v"(u[r]) : "v"(t[0][r]));
      asm volatile("v_add_f32_dpp %0, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xa" : "+v"(u[r]) : "v"(t[1][r]));
    }
    asm volatile("s_nop 1");
    f32x4 x;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = u[r];
      v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, true));   // quad_perm [1,0,3,2]
      v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, true));   // quad_perm [2,3,0,1]
      x[r] = v;
    }
    if ((fq & 3) == 0) *reinterpret_cast<f32x4*>(slot + part * DH + 16 * (fq >> 2) + 4 * fg) = x;
#pragma unroll
    for (int n = 0; n < Cf::NT; ++n) bsum[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  };
  auto bias_reduce = [&](const float* slots, int h) {
    for (int i = tid; i < 3 * DH; i += NW * 64) {
      const int part = i / DH, c = i - part * DH;
      if (part != 1) {      // (k-bias: identically zero, see attn_bwd_kernel)
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) tot += slots[w * 3 * DH + i];
        atomicAdd(dbias_qkv + part * dmodel + h * DH + c, tot);
      }
    }
  };

  // a head's results: row `key` (= this lane's key of block `wid` in phase A, its query of block `wid` in phase B) of dK, dV, dQ
  bf16x4 kb4[Cf::NT], vb4[Cf::NT], qb4[Cf::NT];
  const int key = wid * 16 + fq;
  bf16* dQg_prev = nullptr;
  auto store_head = [&](bf16* dQh) {      // (16-byte stores: store_row_widened)
    if (wid < NTC) {
      bf16* row = dQh + (size_t)min(key, S - 1) * ld;
      store_row_widened<Cf::NT>(row, fg, key < S, qb4);
      store_row_widened<Cf::NT>(row + dmodel, fg, key < S, kb4);
      store_row_widened<Cf::NT>(row + 2 * dmodel, fg, key < S, vb4);
    }
  };
  int hd = blockIdx.x;
  if (hd >= nheads) return;
  // staggered start: the workgroups of a launch all fetch, then all compute.  Four phases a fraction of a head apart spread the
  // fetch bursts (183.1 -> 180.5 us at 2 x 1024 clocks per phase, nothing beyond: tools/ab_attn.py, profiles/r05_attn_bwd_ab.txt);
  // the late starters' tail is 1 / 12 of what it was in the GEMMs (twelve heads per workgroup).
  constexpr int kStagger = 2;
  for (int i = 0; i < (int)((blockIdx.x >> 3) & 3) * kStagger; ++i) __builtin_amdgcn_s_sleep(16);
  request_head(hd);
  int par = 0, prev_h = -1;
  for (;;) {
    const int b = hd / H, h = hd - b * H;
    bf16* dQg = dqkv + (size_t)b * S * ld + h * DH;
    const bf16* Kg = qkv + (size_t)b * S * ld + h * DH + dmodel;
    const int klen = keylen[b];
    float* sBh = sB + par * (NW * 3 * DH);
    // ---- D[q] = rowsum(dO O) keep, lse -> LDS.  This wave's dO rows (its own LDS-DMA) and O chunks have landed after its vmcnt.
    // (__builtin_amdgcn_s_waitcnt, not inline asm: the compiler's own wait insertion must KNOW this wait happened - behind an
    //  opaque asm it assumed the requests of the previous trip still pending and protected every register they target with a
    //  vmcnt(0) in the middle of the next request.  Only LOADS are outstanding here: a head's dK / dV / dQ rows are stored
    //  behind the NEXT head's first barrier, with a whole phase A to complete in before anything waits for vmcnt again.)
    __builtin_amdgcn_s_waitcnt(0x0F70);                               // vmcnt(0)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                  // (the tiles' transfers are invisible to the compiler: this one cannot be dropped)
#pragma unroll
    for (int j = 0; j < kNIW; ++j) {
      const int i = wid + j * NW;
      if (i < kStageInstr) {
        const bf16x8 dvv = *reinterpret_cast<const bf16x8*>(s1 + i * 1024 + lane * 16);
        float part = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) part += (float)orow[j][e] * (float)dvv[e];
        part = chunks_sum<Cf::CH>(part);
        const int row = i * Cf::RPI + rin;
        if (c8 == 0) sD[row] = row < S ? part * keep_prob : 0.f;
      }
    }
    if (tid < NR) sL[tid] = tid < S ? lse_r * kLog2e - log2_inv_keep : INFINITY;
    if (MASK && lane < 4 * NTC) sMW[lane] = mw_req;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                                  // B1: Q, dO, D, lse in place; phase B of the previous head over
    asm volatile("" ::: "memory");
    if (prev_h >= 0 && dbias_qkv) bias_reduce(sB + (par ^ 1) * (NW * 3 * DH), prev_h);
    if (prev_h >= 0) store_head(dQg_prev);
    dQg_prev = dQg;
    stage_rows_hidden<DH>(Kg, ld, S, NR, sK, wid, lane, NW);       // lands under phase A
    // ================= phase A: dV, dK, dS^T (this wave: key block `wid`) =================
    if (wid < NTC) {
      const float kbias = (key < klen) ? 0.f : kMasked;
      f32x4 dv[Cf::NT], dk[Cf::NT];
#pragma unroll
      for (int n = 0; n < Cf::NT; ++n) dv[n] = dk[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kq = 0; kq < NKC; ++kq) {
        f32x4 scA[2], dpA[2], dnegA[2];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          const int t = 2 * kq + hf;
          dnegA[hf] = f32x4{-sD[16 * t + 4 * fg + 0], -sD[16 * t + 4 * fg + 1], -sD[16 * t + 4 * fg + 2], -sD[16 * t + 4 * fg + 3]};
          scA[hf] = f32x4{kbias, kbias, kbias, kbias};
          dpA[hf] = DROP ? f32x4{0.f, 0.f, 0.f, 0.f} : dnegA[hf];
        }
#pragma unroll
        for (int kk = 0; kk < Cf::KK; ++kk) {
#pragma unroll
          for (int hf = 0; hf < 2; ++hf) {
            const int t = 2 * kq + hf;
            if (PAD_TILE(t)) continue;
            const bf16x8 qf = *reinterpret_cast<const bf16x8*>(s0 + t * 16 * Cf::ROWB + r_off[kk]);
            const bf16x8 df = *reinterpret_cast<const bf16x8*>(s1 + t * 16 * Cf::ROWB + r_off[kk]);
            scA[hf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf, kf[kk], scA[hf], 0, 0, 0);   // S[q][key]
            dpA[hf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(df, vf[kk], dpA[hf], 0, 0, 0);   // dPd[q][key]
          }
        }
        f32x4 pd2[2], ds2[2];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          const int t = 2 * kq + hf;
          if (PAD_TILE(t)) {
            pd2[hf] = ds2[hf] = f32x4{0.f, 0.f, 0.f, 0.f};
            continue;
          }
          uint32_t kbits = 0;
          if (MASK) kbits = (uint32_t)(sMW[4 * t + (fq & 3)] >> (4 * fg + 16 * (fq >> 2)));
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int q = 16 * t + 4 * fg + r;
            const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(scA[hf][r], kLog2e, -sL[q]));   // padded q: lse = +inf -> 0
            if (DROP) {      // p = P / keep here, dneg = -D keep
              const float pd = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, p) & bit_to_mask(kbits, r));
              pd2[hf][r] = pd;
              ds2[hf][r] = __builtin_fmaf(pd, dpA[hf][r], p * dnegA[hf][r]);
            } else {
              pd2[hf][r] = p;
              ds2[hf][r] = p * dpA[hf][r];
            }
          }
        }
        const bf16x8 pfrag = bf16x8{(bf16)pd2[0][0], (bf16)pd2[0][1], (bf16)pd2[0][2], (bf16)pd2[0][3],
                                    (bf16)pd2[1][0], (bf16)pd2[1][1], (bf16)pd2[1][2], (bf16)pd2[1][3]};
        const bf16x8 sfrag = bf16x8{(bf16)ds2[0][0], (bf16)ds2[0][1], (bf16)ds2[0][2], (bf16)ds2[0][3],
                                    (bf16)ds2[1][0], (bf16)ds2[1][1], (bf16)ds2[1][2], (bf16)ds2[1][3]};
        // dS^T[key][query]: this lane's four values of a tile are four consecutive queries of its key row
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          if (PAD_TILE(2 * kq + hf)) continue;
          *reinterpret_cast<bf16x4*>(sDS + key * DSP + (32 * kq + 16 * hf + 4 * fg) * 2) =
              hf ? bf16x4{sfrag[4], sfrag[5], sfrag[6], sfrag[7]} : bf16x4{sfrag[0], sfrag[1], sfrag[2], sfrag[3]};
        }
#pragma unroll
        for (int n = 0; n < Cf::NT; ++n) {
          const char* pq = s0 + kq * 32 * Cf::ROWB + t_off[n];
          const char* pdo = s1 + kq * 32 * Cf::ROWB + t_off[n];
          const bf16x8 qT = cat8(lds_tr16(pq), lds_tr16(pq + 16 * Cf::ROWB));
          const bf16x8 dT = cat8(lds_tr16(pdo), lds_tr16(pdo + 16 * Cf::ROWB));
          dv[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dT, pfrag, dv[n], 0, 0, 0);
          dk[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qT, sfrag, dk[n], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int n = 0; n < Cf::NT; ++n) {
        kb4[n] = bf16x4{(bf16)dk[n][0], (bf16)dk[n][1], (bf16)dk[n][2], (bf16)dk[n][3]};
        vb4[n] = bf16x4{(bf16)dv[n][0], (bf16)dv[n][1], (bf16)dv[n][2], (bf16)dv[n][3]};
        if (dbias_qkv) bias_acc(n, key < S ? vb4[n] : bf16x4{0, 0, 0, 0});
      }
    }
    if (dbias_qkv) bias_flush(sBh + wid * 3 * DH, 2);
    // B2: dS^T complete, the K tile landed (each wave waits for its own pieces; no store is outstanding - dK / dV go out below)
    __builtin_amdgcn_s_waitcnt(0);                       // vmcnt(0) expcnt(0) lgkmcnt(0)
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    const int next = hd + gridDim.x;
    if (next < nheads) request_head(next);             // Q / dO tiles are free: everyone is past phase A
    // ================= phase B: dQ^T[d][q] = sum_key K^T[d][key] dS^T[key][q] (this wave: query block `wid`) =================
    if (wid < NTC) {
      f32x4 dq[Cf::NT];
#pragma unroll
      for (int n = 0; n < Cf::NT; ++n) dq[n] = f32x4{0.f, 0.f, 0.f, 0.f};
      const char* pds = sDS + trow * DSP + wid * 32 + (fq & 3) * 8;
#pragma unroll
      for (int kq = 0; kq < NKC; ++kq) {
        const bf16x4 lo = lds_tr16(pds + (32 * kq) * DSP);
        const bf16x4 hi = PAD_TILE(2 * kq + 1) ? bf16x4{0, 0, 0, 0} : lds_tr16(pds + (32 * kq + 16) * DSP);
        const bf16x8 sfr = cat8(lo, hi);
#pragma unroll
        for (int n = 0; n < Cf::NT; ++n) {
          const char* pk = sK + kq * 32 * Cf::ROWB + t_off[n];
          const bf16x8 kT = cat8(lds_tr16(pk), lds_tr16(pk + 16 * Cf::ROWB));
          dq[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kT, sfr, dq[n], 0, 0, 0);
        }
      }
#pragma unroll
      for (int n = 0; n < Cf::NT; ++n) {
        qb4[n] = bf16x4{(bf16)(dq[n][0] * qscale), (bf16)(dq[n][1] * qscale), (bf16)(dq[n][2] * qscale), (bf16)(dq[n][3] * qscale)};
        if (dbias_qkv) bias_acc(n, key < S ? qb4[n] : bf16x4{0, 0, 0, 0});
      }
    }
    if (dbias_qkv) bias_flush(sBh + wid * 3 * DH, 0);
    prev_h = h;
    par ^= 1;
    if (next >= nheads) break;
    hd = next;
  }
  store_head(dQg_prev);
  if (dbias_qkv) {
    __syncthreads();
    bias_reduce(sB + (par ^ 1) * (NW * 3 * DH), prev_h);
  }
#undef PAD_TILE
}

template <int DH>
int launch_fwd(const bf16* qkv, const int* keylen, bf16* ctx, float* lse, unsigned long long* keepmask, int B, int S, int H,
               int dmodel, uint32_t seed, uint32_t thresh24, float inv_keep, hipStream_t st) {
  const int nt = (S + 15) / 16, nk = (S + 31) / 32;
  const size_t lds = (size_t)(nt * 16 + nk * 32) * DH * 2;
  const bool wide = 2 * lds > 160 * 1024;   // a second workgroup would not fit: run eight waves in the one that does
#define M3P_ATTN_FWD(KT)                                                                                        \
  do {                                                                                                          \
    constexpr int NW0 = (KT == 16) ? 8 : 4;   /* S > 384 is always `wide`: no four-wave instantiation (it spills) */ \
    auto kern = thresh24 ? attn_fwd_kernel<DH, KT, true, 0, NW0> : attn_fwd_kernel<DH, KT, false, 0, NW0>;       \
    if (nt == 11 && KT == 6) kern = thresh24 ? ((S & 1) ? attn_fwd_kernel<DH, 6, true, 11> : attn_fwd_kernel<DH, 6, true, 11, 4, true>) \
                                             : attn_fwd_kernel<DH, 6, false, 11>; \
    if (wide) kern = thresh24 ? attn_fwd_kernel<DH, KT, true, 0, 8> : attn_fwd_kernel<DH, KT, false, 0, 8>;       \
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    if (e != hipSuccess) return (int)e;                                                                         \
    hipLaunchKernelGGL(kern, dim3(B* H), dim3((wide || NW0 == 8) ? 512 : 256), lds, st, qkv, keylen, ctx, lse, keepmask, S, H, dmodel, seed, \
                       thresh24, inv_keep);                                                                     \
  } while (0)
  if (nk <= 6) M3P_ATTN_FWD(6);
  else if (nk <= 12) M3P_ATTN_FWD(12);
  else if (nk <= 16) M3P_ATTN_FWD(16);
  else return M3P_EINVAL;
#undef M3P_ATTN_FWD
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

template <int DH>
int launch_bwd(const bf16* qkv, const int* keylen, const bf16* ctx, const bf16* dctx, const float* lse,
               const unsigned long long* keepmask, bf16* dqkv, float* dbias, int B, int S, int H, int dmodel, float qscale,
               uint32_t seed, uint32_t thresh24, float inv_keep, hipStream_t st) {
  const int nk = (S + 31) / 32;
  const bool wide = (size_t)2 * ((size_t)2 * nk * 32 * DH * 2) > 160 * 1024;   // one workgroup per CU anyway: eight waves
  // the M3P sequence (36 regions + 128 tokens: 11 tiles, 6 steps): one block per wave pass, ATTN_BWD_NW waves
  const bool m3p_seq = nk == 6 && (S + 15) / 16 == 11;
  // the one-pass form: 64-wide heads of the M3P sequence, keep bits from the forward pass or no dropout
  const bool onepass = m3p_seq && DH == 64 && (!thresh24 || keepmask) && !(g_attn_variant & 1);
  const int nwaves = wide ? 8 : (onepass ? 12 : (m3p_seq ? ATTN_BWD_NW : 4));
  const size_t lds = (size_t)2 * nk * 32 * DH * 2 + (size_t)2 * nk * 32 * sizeof(float) + 3 * nwaves * DH * sizeof(float) +
                     (onepass ? (size_t)nk * 32 * DH * 2 + (size_t)11 * 16 * 11 * 32 : 0);
#define M3P_ATTN_BWD(KT, DROP, MASK)                                                                            \
  do {                                                                                                          \
    auto kern = attn_bwd_kernel<DH, KT, DROP, MASK, 0, 0>;                                                      \
    if (wide) kern = attn_bwd_kernel<DH, KT, DROP, MASK, 0, 0, 8>;                                              \
    if (nk == 6) kern = attn_bwd_kernel<DH, KT, DROP, MASK, 6, 0>;                                              \
    if (m3p_seq) kern = attn_bwd_kernel<DH, KT, DROP, MASK, 6, 11, ATTN_BWD_NW, 1, 1>;                                \
    if constexpr (DH == 64 && (MASK || !DROP)) { if (onepass) kern = attn_bwd_kernel<DH, KT, DROP, MASK, 6, 11, 12, 1, 1, true>; } \
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    if (e != hipSuccess) return (int)e;                                                                         \
    hipLaunchKernelGGL(kern, dim3(B* H), dim3(nwaves * 64), lds, st, qkv, keylen, ctx, dctx, lse, keepmask, dqkv, dbias, S, H, \
                       dmodel, qscale, seed, thresh24, inv_keep);                                               \
  } while (0)
  if (nk > 16) return M3P_EINVAL;
  if constexpr (DH == 64) {
    if (onepass && !(g_attn_variant & 2)) {
      // CU count of the CURRENT device (one attribute query per call: a process may drive several devices), and the 157 KB of
      // dynamic LDS this kernel needs: a device that refuses them takes the two-phase kernel below instead
      int dev = 0, n_cu = 0;
      if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n_cu <= 0)
        n_cu = 256;
      const size_t ldsp = (size_t)3 * 192 * 128 + (size_t)11 * 16 * 11 * 32 + 2 * 192 * sizeof(float) + 2 * 12 * 3 * 64 * sizeof(float) + 12 * 48 * 8;
      auto kp = thresh24 ? attn_bwd_p_kernel<true, true> : attn_bwd_p_kernel<false, false>;
      if (hipFuncSetAttribute((const void*)kp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsp) == hipSuccess) {
        const int nheads = B * H;
        hipLaunchKernelGGL(kp, dim3(nheads < n_cu ? nheads : n_cu), dim3(768), ldsp, st, qkv, keylen, ctx, dctx, lse, keepmask, dqkv, dbias,
                           S, H, dmodel, nheads, qscale, inv_keep);
        M3P_CHECK_LAUNCH();
        return M3P_OK;
      }
      (void)hipGetLastError();
    }
  }
  // (round 6: with dropout on, backward takes the forward pass's keep words - the re-hashing instantiations existed for tests
  //  only, spilled 124-135 scratch instructions each and are gone; the entry point has refused the call already)
  if (!thresh24) M3P_ATTN_BWD(16, false, false);
  else M3P_ATTN_BWD(16, true, true);
#undef M3P_ATTN_BWD
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

}  // namespace

extern "C" {

void m3p_debug_attn_variant(int v) { g_attn_variant = v; }

int m3p_attn_fwd(const void* qkv, const int32_t* keylen, void* ctx, float* lse, uint64_t* keepmask, int B, int S, int H, int dh,
                 uint32_t seed, uint32_t thresh24, float inv_keep, void* stream) {
  if (B <= 0 || S <= 0 || H <= 0 || S > 512) return M3P_EINVAL;
  if (((uintptr_t)qkv & 15) || ((uintptr_t)ctx & 7)) return M3P_EINVAL;
  const int dmodel = H * dh;
  hipStream_t st = (hipStream_t)stream;
  if (dh == 64) return launch_fwd<64>((const bf16*)qkv, keylen, (bf16*)ctx, lse, (unsigned long long*)keepmask, B, S, H, dmodel, seed, thresh24, inv_keep, st);
  if (dh == 32) return launch_fwd<32>((const bf16*)qkv, keylen, (bf16*)ctx, lse, (unsigned long long*)keepmask, B, S, H, dmodel, seed, thresh24, inv_keep, st);
  return M3P_EINVAL;
}

int m3p_attn_bwd(const void* qkv, const int32_t* keylen, const void* ctx, const void* dctx, const float* lse,
                 const uint64_t* keepmask, void* dqkv, float* dbias_qkv, int B, int S, int H, int dh, float qscale,
                 uint32_t seed, uint32_t thresh24, float inv_keep, void* stream) {
  if (B <= 0 || S <= 0 || H <= 0 || S > 512) return M3P_EINVAL;
  if (thresh24 && !keepmask) return M3P_EINVAL;       // dropout on: the keep words of m3p_attn_fwd are required
  if (((uintptr_t)qkv & 15) || ((uintptr_t)ctx & 15) || ((uintptr_t)dctx & 15) || ((uintptr_t)dqkv & 7)) return M3P_EINVAL;
  const int dmodel = H * dh;
  hipStream_t st = (hipStream_t)stream;
  if (dh == 64)
    return launch_bwd<64>((const bf16*)qkv, keylen, (const bf16*)ctx, (const bf16*)dctx, lse, (const unsigned long long*)keepmask, (bf16*)dqkv, dbias_qkv, B, S, H,
                          dmodel, qscale, seed, thresh24, inv_keep, st);
  if (dh == 32)
    return launch_bwd<32>((const bf16*)qkv, keylen, (const bf16*)ctx, (const bf16*)dctx, lse, (const unsigned long long*)keepmask, (bf16*)dqkv, dbias_qkv, B, S, H,
                          dmodel, qscale, seed, thresh24, inv_keep, st);
  return M3P_EINVAL;
}

}  // extern "C"
