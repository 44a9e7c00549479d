// Tiled attention over a source encoding (forward + backward) for the teacher-forced decoder passes of the seq2seq steps
// (crossfwd(stream_='text', causal=True, src_enc=...): the encoder-attention sub-layer, transformer.py:149-210 with kv = the
// source encoding) on gfx950.
//
// The rectangular, key-length-masked sibling of attn_causal.hip: Tq query rows of every (sequence, head) attend the first
// nk = min(klen[b], Lk) rows of a separate key | value tensor, no causal mask.  It computes what m3p_attn_rows_fwd / _bwd
// (causal = 0, pos0 = 0) of decode.hip compute, with their layouts and their dropout stream index
// ((b*H + h)*Tq + t)*Lk + key, on v_mfma_f32_16x16x32_bf16, with no atomics and nothing Tq x Lk stored.
//
// Blocks of 64 as in the causal file (tile helpers: attn_tile.hpp): a workgroup (four waves) owns 64 queries - or, for
// dk / dv, 64 keys - of one (sequence, head), a wave 16 of them, and walks the 64-row tiles of the other side.  The loop
// bounds come from klen[b] and are workgroup-uniform (scalar): key tiles wholly at or past nk are never visited, in the last
// one the 16-key sub-tiles past nk are skipped and the ragged one is masked per element.  Key / value rows at or past nk
// enter LDS and registers as ZEROS (the bound of the fetch is nk, not Lk): the source encoding may hold anything there, NaN
// included, and a masked probability of 0 would not stop 0 x NaN.  Waves whose 16 rows all lie behind Tq only move tiles.
//   forward     S^T = K Q^T (lane = query column), online softmax in fp32, P -> bf16 straight back as the B operand of
//               O^T = V^T P^T
//   backward 1  query blocks: D[t] = sum_j p_tj dPd_tj in fp32, parked as one float in the first four bytes of the row's dq
//               slot of (b, t, h)
//   backward 2  key blocks over ALL Lk keys: S = Q K^T and dPd = dO V^T (lane = key column), p = exp(S - lse),
//               dV^T += dO^T Pd, dK^T += Q^T dS over every query tile; the owner rounds its fp32 accumulators once and stores
//               the row - exact zeros for keys >= nk, so the caller zeroes nothing and casts nothing
//   backward 3  query blocks again: dS^T from the parked D, dQ^T += K^T dS^T, every dq row written over its parked D
// klen[b] == 0: ctx = 0, lse = 0, dq = 0, dkv = 0, like the rows kernels.
#include "attn_tile.hpp"

namespace {

constexpr int XA_MAX_TQ = 512;           // the position table of the model has 514 rows
constexpr int XA_MAX_KEYS = 1024;        // the rows kernels' own cap (QA_MAX_KEYS): they stay a complete fallback

// keys of sequence b that exist: workgroup-uniform, so the loops over key tiles branch on a scalar
__device__ __forceinline__ int xa_nkeys(const int32_t* __restrict__ klen, int b, int Lk) {
  const int nk = klen ? min(max(klen[b], 0), Lk) : Lk;
  return __builtin_amdgcn_readfirstlane(nk);
}

// A product as one ROUNDED fp32 value: the file is built with -ffp-contract=fast, which would fuse dp * keep - D into one
// fma in the dQ and key-owner passes while the D pass rounds the product, and leave the product's rounding error behind.
// With one key (p = 1, D = dp * keep) dS must be exactly 0, as the rows kernels give it; the empty statement hides the
// product from the fusion.
__device__ __forceinline__ float xa_rounded(float v) {
  __asm__ volatile("" : "+v"(v));
  return v;
}

// ---------------------------------------------------------------------------------------
// forward: workgroup = (sequence, head, 64-query block), wave = 16 queries, lane = query column fq, keys 4 fg + r of a tile
// ---------------------------------------------------------------------------------------
// (four waves per SIMD asked for: left alone the DH = 64 instantiation takes 160 registers - three - and with the cap 128,
//  still without scratch, like the causal forward)
template <int DH>
__global__ __launch_bounds__(256, 4) void attn_cross_fwd_kernel(const bf16* __restrict__ q, int ld_q, const bf16* __restrict__ kv,
                                                            long long kv_bstride, int ld_kv, const int32_t* __restrict__ klen,
                                                            bf16* __restrict__ ctx, float* __restrict__ lse, int Tq, int H, int BH,
                                                            int Lk, uint32_t seed, uint32_t thresh24, float inv_keep) {
  using Cf = CaCfg<DH>;
  __shared__ __attribute__((aligned(16))) char sK[Cf::TILEB];
  __shared__ __attribute__((aligned(16))) char sV[Cf::TILEB];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fq = lane & 15, fg = lane >> 4;
  const int qb = (int)(blockIdx.x / BH);
  const int bh = (int)(blockIdx.x % BH), b = bh / H, h = bh - b * H;
  const int d = H * DH;
  const int nk = xa_nkeys(klen, b, Lk), nkt = (nk + 63) >> 6;
  const bf16* Qg = q + (size_t)b * Tq * ld_q + h * DH;
  const bf16* Kg = kv + (size_t)b * kv_bstride + h * DH;
  const bf16* Vg = Kg + d;
  const int qrow = qb * 64 + wid * 16 + fq;
  const bool wave_on = qb * 64 + wid * 16 < Tq;        // (wave-uniform) at least one of this wave's rows exists
  bf16x8 qf[Cf::KK];
#pragma unroll
  for (int kk = 0; kk < Cf::KK; ++kk)
    qf[kk] = qrow < Tq ? *reinterpret_cast<const bf16x8*>(Qg + (size_t)qrow * ld_q + 32 * kk + 8 * fg) : ca_zero8();
  // K fragment: row 16t + fq, chunk 4kk + fg;  V transposing read: row 32kk2 + 16jj + 4fg + (fq >> 2), 8-byte piece fq & 3 of d-tile n
  int k_off[Cf::KK], v_off[Cf::NT];
#pragma unroll
  for (int kk = 0; kk < Cf::KK; ++kk) k_off[kk] = fq * Cf::ROWB + Cf::swz(4 * kk + fg, fq) * 16;
  const int vrow = 4 * fg + (fq >> 2);
#pragma unroll
  for (int n = 0; n < Cf::NT; ++n) v_off[n] = vrow * Cf::ROWB + Cf::swz(2 * n + ((fq & 3) >> 1), vrow) * 16 + 8 * (fq & 1);

  float m = CA_MASKED, l = 0.f;      // running maximum and normaliser of this lane's query (equal in its four fg lanes)
  f32x4 o[Cf::NT];
#pragma unroll
  for (int n = 0; n < Cf::NT; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  const uint32_t rbase = (uint32_t)(bh * Tq + qrow) * (uint32_t)Lk;
  bf16x8 kr[Cf::CPT], vr[Cf::CPT];
  tile_fetch<DH>(Kg, ld_kv, 0, nk, tid, kr);
  tile_fetch<DH>(Vg, ld_kv, 0, nk, tid, vr);
  for (int kt = 0; kt < nkt; ++kt) {
    __syncthreads();                 // the previous tile has been consumed
    tile_put<DH>(sK, tid, kr);
    tile_put<DH>(sV, tid, vr);
    __syncthreads();
    if (kt + 1 < nkt) {
      tile_fetch<DH>(Kg, ld_kv, (kt + 1) * 64, nk, tid, kr);
      tile_fetch<DH>(Vg, ld_kv, (kt + 1) * 64, nk, tid, vr);
    }
    if (!wave_on) continue;
    const int rem = nk - 64 * kt;                      // keys of this tile that exist (>= 1)
    const int nsub = rem >= 64 ? 4 : (rem + 15) >> 4;  // 16-key sub-tiles holding one
    f32x4 s[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < Cf::KK; ++kk) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (t < nsub) {
          const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sK + t * 16 * Cf::ROWB + k_off[kk]);
          s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[kk], s[t], 0, 0, 0);      // S^T[key 4fg + r][query fq]
        }
    }
    float mx = m;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (t >= nsub) {
        s[t] = f32x4{CA_MASKED, CA_MASKED, CA_MASKED, CA_MASKED};
      } else if (t == nsub - 1 && rem < 64) {
#pragma unroll
        for (int r = 0; r < 4; ++r) s[t][r] = (16 * t + 4 * fg + r < rem) ? s[t][r] : CA_MASKED;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[t][r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float alpha = __expf(m - mx);
    m = mx;
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[t][r] = __expf(s[t][r] - mx);
        sum += s[t][r];
      }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    // (the normaliser is the sum of ALL probabilities; dropout zeroes the ones that do not enter the context, the
    //  rescale by inv_keep waits for the end)
    l = l * alpha + sum;
#pragma unroll
    for (int n = 0; n < Cf::NT; ++n) o[n] *= alpha;
    bf16x8 pf[2];
#pragma unroll
    for (int kk2 = 0; kk2 < 2; ++kk2) {
      float p8[8];
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        const int t = 2 * kk2 + hf;
        float kf4[4] = {1.f, 1.f, 1.f, 1.f};
        if (thresh24 != 0 && t < nsub) keep4(rbase + (uint32_t)(64 * kt + 16 * t + 4 * fg), seed, thresh24, 1.f, kf4);
#pragma unroll
        for (int r = 0; r < 4; ++r) p8[4 * hf + r] = s[t][r] * kf4[r];
      }
      pf[kk2] = ca_pack8(p8);
    }
    // O^T[d][q] += sum_key V[key][d] P[q][key]
#pragma unroll
    for (int kk2 = 0; kk2 < 2; ++kk2)
      if (2 * kk2 < nsub) {
#pragma unroll
        for (int n = 0; n < Cf::NT; ++n) {
          const char* pv = sV + kk2 * 32 * Cf::ROWB + v_off[n];
          const bf16x8 vf = ca_cat8(ca_tr16(pv), ca_tr16(pv + 16 * Cf::ROWB));
          o[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[kk2], o[n], 0, 0, 0);
        }
      }
  }
  if (qrow < Tq) {
    // (nk == 0 - a sequence without keys: the loop never ran, l = 0 - gives ctx = 0 and lse = 0 like the rows kernels)
    const float inv = nk > 0 ? inv_keep / l : 0.f;
    bf16* orow = ctx + ((size_t)b * Tq + qrow) * d + h * DH + 4 * fg;
#pragma unroll
    for (int n = 0; n < Cf::NT; ++n)
      *reinterpret_cast<bf16x4*>(orow + 16 * n) =
          bf16x4{(bf16)(o[n][0] * inv), (bf16)(o[n][1] * inv), (bf16)(o[n][2] * inv), (bf16)(o[n][3] * inv)};
    if (fg == 0) lse[(size_t)bh * Tq + qrow] = nk > 0 ? m + __logf(l) : 0.f;
  }
}

// ---------------------------------------------------------------------------------------
// backward, query blocks (same orientation as the forward).  DQ = false: D[t] = sum_j p_tj dPd_tj, parked in the dq slot;
// DQ = true: dS^T from the parked D, dQ^T[d][q] = sum_key K[key][d] dS[q][key], times qscale (q was stored pre-scaled).
// ---------------------------------------------------------------------------------------
// (three / two waves per SIMD asked for: one more than that spills at DH = 64, left alone both passes take two)
template <int DH, bool DQ>
__global__ __launch_bounds__(256, DQ ? 2 : 3) void attn_cross_bwd_q_kernel(const bf16* __restrict__ q, int ld_q, const bf16* __restrict__ kv,
                                                              long long kv_bstride, int ld_kv, const int32_t* __restrict__ klen,
                                                              const bf16* __restrict__ dctx, const float* __restrict__ lse,
                                                              bf16* __restrict__ dq, int ld_dq, int Tq, int H, int BH, int Lk,
                                                              float qscale, uint32_t seed, uint32_t thresh24, float inv_keep) {
  using Cf = CaCfg<DH>;
  __shared__ __attribute__((aligned(16))) char sK[Cf::TILEB];
  __shared__ __attribute__((aligned(16))) char sV[Cf::TILEB];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fq = lane & 15, fg = lane >> 4;
  const int qb = (int)(blockIdx.x / BH);
  const int bh = (int)(blockIdx.x % BH), b = bh / H, h = bh - b * H;
  const int d = H * DH;
  const int nk = xa_nkeys(klen, b, Lk), nkt = (nk + 63) >> 6;
  const bf16* Qg = q + (size_t)b * Tq * ld_q + h * DH;
  const bf16* Kg = kv + (size_t)b * kv_bstride + h * DH;
  const bf16* Vg = Kg + d;
  const int qrow = qb * 64 + wid * 16 + fq;
  const bool qok = qrow < Tq;
  const bool wave_on = qb * 64 + wid * 16 < Tq;
  bf16x8 qf[Cf::KK], gf[Cf::KK];
#pragma unroll
  for (int kk = 0; kk < Cf::KK; ++kk) {
    qf[kk] = qok ? *reinterpret_cast<const bf16x8*>(Qg + (size_t)qrow * ld_q + 32 * kk + 8 * fg) : ca_zero8();
    gf[kk] = qok ? *reinterpret_cast<const bf16x8*>(dctx + ((size_t)b * Tq + qrow) * d + h * DH + 32 * kk + 8 * fg) : ca_zero8();
  }
  bf16* dqrow = dq + ((size_t)b * Tq + (qok ? qrow : 0)) * ld_dq + h * DH;
  const float lq = qok ? lse[(size_t)bh * Tq + qrow] : INFINITY;       // a row behind the sequence: p = exp(s - inf) = 0
  // (without keys the loop never runs and no barrier separates this read from the row's store: D is not read then)
  float Dq = (DQ && qok && nk > 0) ? *reinterpret_cast<const float*>(dqrow) : 0.f;
  int k_off[Cf::KK], v_off[Cf::NT];
#pragma unroll
  for (int kk = 0; kk < Cf::KK; ++kk) k_off[kk] = fq * Cf::ROWB + Cf::swz(4 * kk + fg, fq) * 16;
  const int vrow = 4 * fg + (fq >> 2);
#pragma unroll
  for (int n = 0; n < Cf::NT; ++n) v_off[n] = vrow * Cf::ROWB + Cf::swz(2 * n + ((fq & 3) >> 1), vrow) * 16 + 8 * (fq & 1);
  f32x4 dqa[Cf::NT];
#pragma unroll
  for (int n = 0; n < Cf::NT; ++n) dqa[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  const uint32_t rbase = (uint32_t)(bh * Tq + qrow) * (uint32_t)Lk;
  bf16x8 kr[Cf::CPT], vr[Cf::CPT];
  tile_fetch<DH>(Kg, ld_kv, 0, nk, tid, kr);
  tile_fetch<DH>(Vg, ld_kv, 0, nk, tid, vr);
  for (int kt = 0; kt < nkt; ++kt) {
    __syncthreads();
    tile_put<DH>(sK, tid, kr);
    tile_put<DH>(sV, tid, vr);
    __syncthreads();
    if (kt + 1 < nkt) {
      tile_fetch<DH>(Kg, ld_kv, (kt + 1) * 64, nk, tid, kr);
      tile_fetch<DH>(Vg, ld_kv, (kt + 1) * 64, nk, tid, vr);
    }
    if (!wave_on) continue;
    const int rem = nk - 64 * kt;
    const int nsub = rem >= 64 ? 4 : (rem + 15) >> 4;
    f32x4 sc[4], dp[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) sc[t] = dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < Cf::KK; ++kk) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (t < nsub) {
          const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sK + t * 16 * Cf::ROWB + k_off[kk]);
          const bf16x8 vf = *reinterpret_cast<const bf16x8*>(sV + t * 16 * Cf::ROWB + k_off[kk]);
          sc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[kk], sc[t], 0, 0, 0);      // S^T[key][query]
          dp[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, gf[kk], dp[t], 0, 0, 0);      // dPd^T[key][query]
        }
    }
    float ds[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (t < nsub) {
        float kf4[4] = {1.f, 1.f, 1.f, 1.f};
        if (thresh24 != 0) keep4(rbase + (uint32_t)(64 * kt + 16 * t + 4 * fg), seed, thresh24, inv_keep, kf4);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float p = __expf(sc[t][r] - lq);
          if (t == nsub - 1 && rem < 64) p = (16 * t + 4 * fg + r < rem) ? p : 0.f;
          const float dpd = xa_rounded(dp[t][r] * kf4[r]);       // gradient wrt p through the dropout
          if (DQ) ds[t][r] = p * (dpd - Dq);
          else Dq = __builtin_fmaf(p, dpd, Dq);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) ds[t][r] = 0.f;
      }
    }
    if (DQ) {
#pragma unroll
      for (int kk2 = 0; kk2 < 2; ++kk2)
        if (2 * kk2 < nsub) {
          const float s8[8] = {ds[2 * kk2][0], ds[2 * kk2][1], ds[2 * kk2][2], ds[2 * kk2][3],
                               ds[2 * kk2 + 1][0], ds[2 * kk2 + 1][1], ds[2 * kk2 + 1][2], ds[2 * kk2 + 1][3]};
          const bf16x8 sf = ca_pack8(s8);
#pragma unroll
          for (int n = 0; n < Cf::NT; ++n) {
            const char* pk = sK + kk2 * 32 * Cf::ROWB + v_off[n];
            const bf16x8 kT = ca_cat8(ca_tr16(pk), ca_tr16(pk + 16 * Cf::ROWB));
            dqa[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kT, sf, dqa[n], 0, 0, 0);
          }
        }
    }
  }
  if (DQ) {
    if (qok) {
#pragma unroll
      for (int n = 0; n < Cf::NT; ++n)
        *reinterpret_cast<bf16x4*>(dqrow + 16 * n + 4 * fg) = bf16x4{(bf16)(dqa[n][0] * qscale), (bf16)(dqa[n][1] * qscale),
                                                                     (bf16)(dqa[n][2] * qscale), (bf16)(dqa[n][3] * qscale)};
    }
  } else {
    Dq += __shfl_xor(Dq, 16, 64);
    Dq += __shfl_xor(Dq, 32, 64);
    if (qok && fg == 0) *reinterpret_cast<float*>(dqrow) = Dq;
  }
}

// ---------------------------------------------------------------------------------------
// backward, key blocks: workgroup = (sequence, head, 64-key block) over all Lk keys, wave = 16 keys, lane = key column fq,
// queries 4 fg + r of a 16-query sub-tile.  dV^T[d][key] = sum_q dO[q][d] Pd[q][key], dK^T[d][key] = sum_q Q[q][d] dS[q][key]
// over every query tile; P and dS of a tile go from the accumulators straight into the B operands.  A block wholly at or
// past nk skips the loop; every key < Lk is stored, the ones >= nk as zeros.
// ---------------------------------------------------------------------------------------
// (two waves per SIMD asked for, as for the causal kernel: left alone the DH = 64 instantiation takes one wave per SIMD)
template <int DH>
__global__ __launch_bounds__(256, 2) void attn_cross_bwd_kv_kernel(const bf16* __restrict__ q, int ld_q, const bf16* __restrict__ kv,
                                                                  long long kv_bstride, int ld_kv,
                                                                  const int32_t* __restrict__ klen, const bf16* __restrict__ dctx,
                                                                  const float* __restrict__ lse, const bf16* __restrict__ dq,
                                                                  int ld_dq, bf16* __restrict__ dkv, int ld_dkv, int Tq, int H,
                                                                  int BH, int Lk, uint32_t seed, uint32_t thresh24, float inv_keep) {
  using Cf = CaCfg<DH>;
  __shared__ __attribute__((aligned(16))) char sQ[Cf::TILEB];
  __shared__ __attribute__((aligned(16))) char sG[Cf::TILEB];      // dO
  __shared__ __attribute__((aligned(16))) float sL[64];            // lse of the tile's queries (+inf behind the sequence)
  __shared__ __attribute__((aligned(16))) float sD[64];            // their D
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fq = lane & 15, fg = lane >> 4;
  const int kb = (int)(blockIdx.x / BH);
  const int bh = (int)(blockIdx.x % BH), b = bh / H, h = bh - b * H;
  const int d = H * DH;
  const int nk = xa_nkeys(klen, b, Lk);
  const int nqb = (Tq + 63) >> 6;
  const bf16* Qg = q + (size_t)b * Tq * ld_q + h * DH;
  const bf16* Gg = dctx + (size_t)b * Tq * d + h * DH;
  const bf16* Kg = kv + (size_t)b * kv_bstride + h * DH;
  const int key = kb * 64 + wid * 16 + fq;
  const bool kok = key < nk;
  const bool wave_on = kb * 64 + wid * 16 < nk;        // (wave-uniform) at least one of this wave's keys exists
  bf16x8 kf[Cf::KK], vf[Cf::KK];
#pragma unroll
  for (int kk = 0; kk < Cf::KK; ++kk) {
    kf[kk] = kok ? *reinterpret_cast<const bf16x8*>(Kg + (size_t)key * ld_kv + 32 * kk + 8 * fg) : ca_zero8();
    vf[kk] = kok ? *reinterpret_cast<const bf16x8*>(Kg + d + (size_t)key * ld_kv + 32 * kk + 8 * fg) : ca_zero8();
  }
  int r_off[Cf::KK], t_off[Cf::NT];
#pragma unroll
  for (int kk = 0; kk < Cf::KK; ++kk) r_off[kk] = fq * Cf::ROWB + Cf::swz(4 * kk + fg, fq) * 16;
  const int trow = 4 * fg + (fq >> 2);
#pragma unroll
  for (int n = 0; n < Cf::NT; ++n) t_off[n] = trow * Cf::ROWB + Cf::swz(2 * n + ((fq & 3) >> 1), trow) * 16 + 8 * (fq & 1);
  f32x4 dv[Cf::NT], dk[Cf::NT];
#pragma unroll
  for (int n = 0; n < Cf::NT; ++n) dv[n] = dk[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nqt = kb * 64 < nk ? nqb : 0;              // (workgroup-uniform) a block without keys walks nothing
  bf16x8 qr[Cf::CPT], gr[Cf::CPT];
  tile_fetch<DH>(Qg, ld_q, 0, nqt > 0 ? Tq : 0, tid, qr);
  tile_fetch<DH>(Gg, d, 0, nqt > 0 ? Tq : 0, tid, gr);
  for (int qt = 0; qt < nqt; ++qt) {
    __syncthreads();
    tile_put<DH>(sQ, tid, qr);
    tile_put<DH>(sG, tid, gr);
    if (tid < 64) {
      const int qq = qt * 64 + tid;
      const bool ok = qq < Tq;
      sL[tid] = ok ? lse[(size_t)bh * Tq + qq] : INFINITY;
      sD[tid] = ok ? *reinterpret_cast<const float*>(dq + ((size_t)b * Tq + qq) * ld_dq + h * DH) : 0.f;
    }
    __syncthreads();
    if (qt + 1 < nqt) {
      tile_fetch<DH>(Qg, ld_q, (qt + 1) * 64, Tq, tid, qr);
      tile_fetch<DH>(Gg, d, (qt + 1) * 64, Tq, tid, gr);
    }
    if (!wave_on) continue;
    const int remq = Tq - 64 * qt;                       // queries of this tile that exist (>= 1)
    const int nsub = remq >= 64 ? 4 : (remq + 15) >> 4;  // 16-query sub-tiles holding one
    f32x4 sc[4], dp[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) sc[t] = dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < Cf::KK; ++kk) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (t < nsub) {
          const bf16x8 qf = *reinterpret_cast<const bf16x8*>(sQ + t * 16 * Cf::ROWB + r_off[kk]);
          const bf16x8 gf = *reinterpret_cast<const bf16x8*>(sG + t * 16 * Cf::ROWB + r_off[kk]);
          sc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf, kf[kk], sc[t], 0, 0, 0);      // S[query 4fg + r][key fq]
          dp[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gf, vf[kk], dp[t], 0, 0, 0);      // dPd[query][key]
        }
    }
    float pd[4][4], ds[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (t < nsub) {
        const f32x4 l4 = *reinterpret_cast<const f32x4*>(sL + 16 * t + 4 * fg);
        const f32x4 d4 = *reinterpret_cast<const f32x4*>(sD + 16 * t + 4 * fg);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qq = qt * 64 + 16 * t + 4 * fg + r;
          const float p = kok ? __expf(sc[t][r] - l4[r]) : 0.f;       // (a key >= nk: its column is not part of the softmax)
          float keepf = 1.f;
          if (thresh24 != 0)
            keepf = m3p_keep((uint32_t)(bh * Tq + qq) * (uint32_t)Lk + (uint32_t)key, seed, thresh24) ? inv_keep : 0.f;
          const float dpd = xa_rounded(dp[t][r] * keepf);
          pd[t][r] = p * keepf;
          ds[t][r] = p * (dpd - d4[r]);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) pd[t][r] = ds[t][r] = 0.f;
      }
    }
#pragma unroll
    for (int kk2 = 0; kk2 < 2; ++kk2)
      if (2 * kk2 < nsub) {
        const float p8[8] = {pd[2 * kk2][0], pd[2 * kk2][1], pd[2 * kk2][2], pd[2 * kk2][3],
                             pd[2 * kk2 + 1][0], pd[2 * kk2 + 1][1], pd[2 * kk2 + 1][2], pd[2 * kk2 + 1][3]};
        const float s8[8] = {ds[2 * kk2][0], ds[2 * kk2][1], ds[2 * kk2][2], ds[2 * kk2][3],
                             ds[2 * kk2 + 1][0], ds[2 * kk2 + 1][1], ds[2 * kk2 + 1][2], ds[2 * kk2 + 1][3]};
        const bf16x8 pf = ca_pack8(p8), sf = ca_pack8(s8);
#pragma unroll
        for (int n = 0; n < Cf::NT; ++n) {
          const char* pg = sG + kk2 * 32 * Cf::ROWB + t_off[n];
          const char* pq = sQ + kk2 * 32 * Cf::ROWB + t_off[n];
          const bf16x8 gT = ca_cat8(ca_tr16(pg), ca_tr16(pg + 16 * Cf::ROWB));
          const bf16x8 qT = ca_cat8(ca_tr16(pq), ca_tr16(pq + 16 * Cf::ROWB));
          dv[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gT, pf, dv[n], 0, 0, 0);
          dk[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qT, sf, dk[n], 0, 0, 0);
        }
      }
  }
  if (key < Lk) {
    bf16* krow = dkv + ((size_t)b * Lk + key) * ld_dkv + h * DH + 4 * fg;
#pragma unroll
    for (int n = 0; n < Cf::NT; ++n) {
      const bf16x4 k4 = bf16x4{(bf16)dk[n][0], (bf16)dk[n][1], (bf16)dk[n][2], (bf16)dk[n][3]};
      const bf16x4 v4 = bf16x4{(bf16)dv[n][0], (bf16)dv[n][1], (bf16)dv[n][2], (bf16)dv[n][3]};
      const bf16x4 z4 = bf16x4{0, 0, 0, 0};
      *reinterpret_cast<bf16x4*>(krow + 16 * n) = kok ? k4 : z4;
      *reinterpret_cast<bf16x4*>(krow + d + 16 * n) = kok ? v4 : z4;
    }
  }
}

// shapes outside the tiled kernels' range are "not implemented", so that a caller can take the rows kernels instead
int xa_admit(int B, int Tq, int H, int dh, int Lk) {
  if (B <= 0 || Tq <= 0 || H <= 0 || Lk <= 0) return M3P_EINVAL;
  if ((dh != 32 && dh != 64) || Tq > XA_MAX_TQ || Lk > XA_MAX_KEYS) return M3P_ENOTIMPL;
  if ((unsigned long long)B * H * Tq * Lk >= (1ull << 32)) return M3P_ENOTIMPL;       // 32-bit dropout stream index
  return M3P_OK;
}

}  // namespace

extern "C" {

int m3p_attn_cross_fwd(const void* q, int ld_q, const void* kv, long long kv_bstride, int ld_kv, const int32_t* klen, void* ctx,
                       float* lse, int B, int Tq, int H, int dh, int Lk, uint32_t seed, uint32_t thresh24, float inv_keep,
                       void* stream) {
  if (!q || !kv || !ctx || !lse) return M3P_EINVAL;
  const int rc = xa_admit(B, Tq, H, dh, Lk);
  if (rc != M3P_OK) return rc;
  if (ld_q < H * dh || ld_kv < 2 * H * dh) return M3P_EINVAL;
  if ((ld_q % 8) != 0 || (ld_kv % 8) != 0 || (kv_bstride % 8) != 0 || ((uintptr_t)q & 15) || ((uintptr_t)kv & 15) ||
      ((uintptr_t)ctx & 15))
    return M3P_ENOTIMPL;
  const int nqb = (Tq + 63) / 64, BH = B * H;
  const dim3 grid((unsigned)(nqb * BH)), block(256);
  if (dh == 64)
    hipLaunchKernelGGL(attn_cross_fwd_kernel<64>, grid, block, 0, (hipStream_t)stream, (const bf16*)q, ld_q, (const bf16*)kv,
                       kv_bstride, ld_kv, klen, (bf16*)ctx, lse, Tq, H, BH, Lk, seed, thresh24, inv_keep);
  else
    hipLaunchKernelGGL(attn_cross_fwd_kernel<32>, grid, block, 0, (hipStream_t)stream, (const bf16*)q, ld_q, (const bf16*)kv,
                       kv_bstride, ld_kv, klen, (bf16*)ctx, lse, Tq, H, BH, Lk, seed, thresh24, inv_keep);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

int m3p_attn_cross_bwd(const void* q, int ld_q, const void* kv, long long kv_bstride, int ld_kv, const int32_t* klen,
                       const void* dctx, const float* lse, void* dq, int ld_dq, void* dkv, int ld_dkv, int B, int Tq, int H,
                       int dh, int Lk, float qscale, uint32_t seed, uint32_t thresh24, float inv_keep, void* stream) {
  if (!q || !kv || !dctx || !lse || !dq || !dkv) return M3P_EINVAL;
  const int rc = xa_admit(B, Tq, H, dh, Lk);
  if (rc != M3P_OK) return rc;
  if (ld_q < H * dh || ld_kv < 2 * H * dh || ld_dq < H * dh || ld_dkv < 2 * H * dh) return M3P_EINVAL;
  if ((ld_q % 8) != 0 || (ld_kv % 8) != 0 || (kv_bstride % 8) != 0 || (ld_dq % 8) != 0 || (ld_dkv % 8) != 0 ||
      ((uintptr_t)q & 15) || ((uintptr_t)kv & 15) || ((uintptr_t)dctx & 15) || ((uintptr_t)dq & 15) || ((uintptr_t)dkv & 15))
    return M3P_ENOTIMPL;
  const int nqb = (Tq + 63) / 64, nkb = (Lk + 63) / 64, BH = B * H;
  const dim3 gridq((unsigned)(nqb * BH)), gridk((unsigned)(nkb * BH)), block(256);
  hipStream_t st = (hipStream_t)stream;
#define XA_BWD(DH_)                                                                                                              \
  do {                                                                                                                           \
    hipLaunchKernelGGL((attn_cross_bwd_q_kernel<DH_, false>), gridq, block, 0, st, (const bf16*)q, ld_q, (const bf16*)kv,        \
                       kv_bstride, ld_kv, klen, (const bf16*)dctx, lse, (bf16*)dq, ld_dq, Tq, H, BH, Lk, qscale, seed, thresh24,  \
                       inv_keep);                                                                                                \
    hipLaunchKernelGGL(attn_cross_bwd_kv_kernel<DH_>, gridk, block, 0, st, (const bf16*)q, ld_q, (const bf16*)kv, kv_bstride,    \
                       ld_kv, klen, (const bf16*)dctx, lse, (const bf16*)dq, ld_dq, (bf16*)dkv, ld_dkv, Tq, H, BH, Lk, seed,      \
                       thresh24, inv_keep);                                                                                      \
    hipLaunchKernelGGL((attn_cross_bwd_q_kernel<DH_, true>), gridq, block, 0, st, (const bf16*)q, ld_q, (const bf16*)kv,         \
                       kv_bstride, ld_kv, klen, (const bf16*)dctx, lse, (bf16*)dq, ld_dq, Tq, H, BH, Lk, qscale, seed, thresh24,  \
                       inv_keep);                                                                                                \
  } while (0)
  if (dh == 64) XA_BWD(64);
  else XA_BWD(32);
#undef XA_BWD
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

}  // extern "C"
