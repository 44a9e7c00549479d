// Tiled causal self-attention (forward + backward) of the teacher-forced decoder passes on gfx950: the decoder-only pass of
// the causal language-model objective (crossfwd(stream_='text', causal=True) without a source encoding: xtrainer.py:694-732)
// and the self-attention sub-layer of the seq2seq steps' pass over a source encoding (whose other attention is
// attn_cross.hip), training and cache-less scoring alike.
//
// The rows kernels of decode.hip serve short target sequences: a wave per (sequence, head, query), no MFMAs, and a backward
// that adds dk / dv with two 64-float atomics per (query, key) pair.  A CLM stream batch is bptt (256) long in every lane, so
// this file does the same attention - m3p_attn_rows_fwd / _bwd(causal=1, klen=NULL, pos0=0, Lk=T), the same dropout stream
// index ((b*H + h)*T + t)*T + key - on v_mfma_f32_16x16x32_bf16 with no atomics and nothing T x T stored.
//
// Blocks of 64: a workgroup (four waves) owns 64 queries - or, for dk / dv, 64 keys - of one (sequence, head), a wave 16 of
// them, and walks the 64-row tiles of the other side that causality leaves: keys at and below the diagonal for a query
// block, queries at and behind it for a key block.  Tiles wholly above the diagonal are never visited, and inside the
// diagonal tile a wave skips the 16-row sub-tiles above its own rows and masks its own sub-tile per element (one compare:
// a lane owns a column).  A tile goes global -> registers (rows >= T as zeros) -> LDS, row-major with the 16-byte chunk
// swizzle of attention.hip (the helpers live in attn_tile.hpp, shared with attn_cross.hip); the next tile's loads are in
// flight while the current one is computed on.
//   forward     S^T = K Q^T (lane = query column), online softmax over the key tiles in fp32, P -> bf16 straight back as the
//               B operand of O^T = V^T P^T (V through transposing LDS reads, same k-slot permutation as attention.hip)
//   backward 1  query blocks: D[t] = sum_j p_tj dPd_tj in fp32 (there is no ctx argument to take rowsum(dO * O) from), parked
//               as one float in the first four bytes of the row's dq slot of (b, t, h) - dqkv is the only buffer the ABI has
//   backward 2  key blocks: S = Q K^T and dPd = dO V^T un-swapped (lane = key column), p = exp(S - lse), then
//               dV^T += dO^T Pd, dK^T += Q^T dS over the queries at and below the diagonal; the owner stores the rows once
//   backward 3  query blocks again: dS^T recomputed from the parked D, dQ^T += K^T dS^T, then every dq row is written over
//               its parked D (a lane reads the D of its own row only, before the loop)
// Causal work grows with the query block (shrinks with the key block): block ids are handed out heaviest first.
#include "attn_tile.hpp"

namespace {

constexpr int CA_MAX_T = 512;            // the position table of the model has 514 rows

// ---------------------------------------------------------------------------------------
// forward: workgroup = (sequence, head, 64-query block), wave = 16 queries, lane = query column fq, keys 4 fg + r of a tile
// ---------------------------------------------------------------------------------------
template <int DH>
__global__ __launch_bounds__(256) void attn_causal_fwd_kernel(const bf16* __restrict__ qkv, int ld, bf16* __restrict__ ctx,
                                                             float* __restrict__ lse, int T, int H, int BH, int nqb,
                                                             uint32_t seed, uint32_t thresh24, float inv_keep) {
  using Cf = CaCfg<DH>;
  __shared__ __attribute__((aligned(16))) char sK[Cf::TILEB];
  __shared__ __attribute__((aligned(16))) char sV[Cf::TILEB];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fq = lane & 15, fg = lane >> 4;
  const int qb = nqb - 1 - (int)(blockIdx.x / BH);          // heaviest (last) query blocks first
  const int bh = (int)(blockIdx.x % BH), b = bh / H, h = bh - b * H;
  const int d = H * DH;
  const bf16* Qg = qkv + (size_t)b * T * ld + h * DH;
  const bf16* Kg = Qg + d;
  const bf16* Vg = Qg + 2 * d;
  const int q = qb * 64 + wid * 16 + fq;
  bf16x8 qf[Cf::KK];
#pragma unroll
  for (int kk = 0; kk < Cf::KK; ++kk)
    qf[kk] = q < T ? *reinterpret_cast<const bf16x8*>(Qg + (size_t)q * ld + 32 * kk + 8 * fg) : ca_zero8();
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
  const uint32_t rbase = (uint32_t)(bh * T + q) * (uint32_t)T;
  bf16x8 kr[Cf::CPT], vr[Cf::CPT];
  tile_fetch<DH>(Kg, ld, 0, T, tid, kr);
  tile_fetch<DH>(Vg, ld, 0, T, tid, vr);
  for (int kt = 0; kt <= qb; ++kt) {
    __syncthreads();                 // the previous tile has been consumed
    tile_put<DH>(sK, tid, kr);
    tile_put<DH>(sV, tid, vr);
    __syncthreads();
    if (kt < qb) {
      tile_fetch<DH>(Kg, ld, (kt + 1) * 64, T, tid, kr);
      tile_fetch<DH>(Vg, ld, (kt + 1) * 64, T, tid, vr);
    }
    const bool diag = kt == qb;
    const int nsub = diag ? wid + 1 : 4;     // 16-key sub-tiles at or below this wave's queries (every wave has sub-tile 0)
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
      } else if (diag && t == wid) {
#pragma unroll
        for (int r = 0; r < 4; ++r) s[t][r] = (4 * fg + r <= fq) ? s[t][r] : CA_MASKED;
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
  if (q < T) {
    const float inv = inv_keep / l;
    bf16* orow = ctx + ((size_t)b * T + q) * d + h * DH + 4 * fg;
#pragma unroll
    for (int n = 0; n < Cf::NT; ++n)
      *reinterpret_cast<bf16x4*>(orow + 16 * n) =
          bf16x4{(bf16)(o[n][0] * inv), (bf16)(o[n][1] * inv), (bf16)(o[n][2] * inv), (bf16)(o[n][3] * inv)};
    if (fg == 0) lse[(size_t)bh * T + q] = m + __logf(l);
  }
}

// ---------------------------------------------------------------------------------------
// backward, query blocks (same orientation as the forward).  DQ = false: D[t] = sum_j p_tj dPd_tj, parked in the dq slot;
// DQ = true: dS^T from the parked D, dQ^T[d][q] = sum_key K[key][d] dS[q][key], times qscale (q was stored pre-scaled).
// ---------------------------------------------------------------------------------------
template <int DH, bool DQ>
__global__ __launch_bounds__(256) void attn_causal_bwd_q_kernel(const bf16* __restrict__ qkv, int ld, const bf16* __restrict__ dctx,
                                                               const float* __restrict__ lse, bf16* __restrict__ dqkv, int ld_dq,
                                                               int T, int H, int BH, int nqb, float qscale, uint32_t seed,
                                                               uint32_t thresh24, float inv_keep) {
  using Cf = CaCfg<DH>;
  __shared__ __attribute__((aligned(16))) char sK[Cf::TILEB];
  __shared__ __attribute__((aligned(16))) char sV[Cf::TILEB];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fq = lane & 15, fg = lane >> 4;
  const int qb = nqb - 1 - (int)(blockIdx.x / BH);
  const int bh = (int)(blockIdx.x % BH), b = bh / H, h = bh - b * H;
  const int d = H * DH;
  const bf16* Qg = qkv + (size_t)b * T * ld + h * DH;
  const bf16* Kg = Qg + d;
  const bf16* Vg = Qg + 2 * d;
  const int q = qb * 64 + wid * 16 + fq;
  const bool qok = q < T;
  bf16x8 qf[Cf::KK], gf[Cf::KK];
#pragma unroll
  for (int kk = 0; kk < Cf::KK; ++kk) {
    qf[kk] = qok ? *reinterpret_cast<const bf16x8*>(Qg + (size_t)q * ld + 32 * kk + 8 * fg) : ca_zero8();
    gf[kk] = qok ? *reinterpret_cast<const bf16x8*>(dctx + ((size_t)b * T + q) * d + h * DH + 32 * kk + 8 * fg) : ca_zero8();
  }
  bf16* dqrow = dqkv + ((size_t)b * T + (qok ? q : 0)) * ld_dq + h * DH;
  const float lq = qok ? lse[(size_t)bh * T + q] : INFINITY;       // a row behind the sequence: p = exp(s - inf) = 0
  float Dq = (DQ && qok) ? *reinterpret_cast<const float*>(dqrow) : 0.f;
  int k_off[Cf::KK], v_off[Cf::NT];
#pragma unroll
  for (int kk = 0; kk < Cf::KK; ++kk) k_off[kk] = fq * Cf::ROWB + Cf::swz(4 * kk + fg, fq) * 16;
  const int vrow = 4 * fg + (fq >> 2);
#pragma unroll
  for (int n = 0; n < Cf::NT; ++n) v_off[n] = vrow * Cf::ROWB + Cf::swz(2 * n + ((fq & 3) >> 1), vrow) * 16 + 8 * (fq & 1);
  f32x4 dq[Cf::NT];
#pragma unroll
  for (int n = 0; n < Cf::NT; ++n) dq[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  const uint32_t rbase = (uint32_t)(bh * T + q) * (uint32_t)T;
  bf16x8 kr[Cf::CPT], vr[Cf::CPT];
  tile_fetch<DH>(Kg, ld, 0, T, tid, kr);
  tile_fetch<DH>(Vg, ld, 0, T, tid, vr);
  for (int kt = 0; kt <= qb; ++kt) {
    __syncthreads();
    tile_put<DH>(sK, tid, kr);
    tile_put<DH>(sV, tid, vr);
    __syncthreads();
    if (kt < qb) {
      tile_fetch<DH>(Kg, ld, (kt + 1) * 64, T, tid, kr);
      tile_fetch<DH>(Vg, ld, (kt + 1) * 64, T, tid, vr);
    }
    const bool diag = kt == qb;
    const int nsub = diag ? wid + 1 : 4;
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
          if (diag && t == wid) p = (4 * fg + r <= fq) ? p : 0.f;
          const float dpd = dp[t][r] * kf4[r];       // gradient wrt p through the dropout
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
            dq[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kT, sf, dq[n], 0, 0, 0);
          }
        }
    }
  }
  if (DQ) {
    if (qok) {
#pragma unroll
      for (int n = 0; n < Cf::NT; ++n)
        *reinterpret_cast<bf16x4*>(dqrow + 16 * n + 4 * fg) = bf16x4{(bf16)(dq[n][0] * qscale), (bf16)(dq[n][1] * qscale),
                                                                     (bf16)(dq[n][2] * qscale), (bf16)(dq[n][3] * qscale)};
    }
  } else {
    Dq += __shfl_xor(Dq, 16, 64);
    Dq += __shfl_xor(Dq, 32, 64);
    if (qok && fg == 0) *reinterpret_cast<float*>(dqrow) = Dq;
  }
}

// ---------------------------------------------------------------------------------------
// backward, key blocks: workgroup = (sequence, head, 64-key block), wave = 16 keys, lane = key column fq, queries 4 fg + r of
// a 16-query sub-tile.  dV^T[d][key] = sum_q dO[q][d] Pd[q][key], dK^T[d][key] = sum_q Q[q][d] dS[q][key] over the query
// tiles at and behind the diagonal; P and dS of a tile go from the accumulators straight into the B operands.
// ---------------------------------------------------------------------------------------
// (two waves per SIMD asked for: left alone the DH = 64 instantiation takes 276 registers - one wave per SIMD - and with
//  the cap 198, still without scratch)
template <int DH>
__global__ __launch_bounds__(256, 2) void attn_causal_bwd_kv_kernel(const bf16* __restrict__ qkv, int ld, const bf16* __restrict__ dctx,
                                                                const float* __restrict__ lse, bf16* __restrict__ dqkv, int ld_dq,
                                                                int T, int H, int BH, int nqb, uint32_t seed, uint32_t thresh24,
                                                                float inv_keep) {
  using Cf = CaCfg<DH>;
  __shared__ __attribute__((aligned(16))) char sQ[Cf::TILEB];
  __shared__ __attribute__((aligned(16))) char sG[Cf::TILEB];      // dO
  __shared__ __attribute__((aligned(16))) float sL[64];            // lse of the tile's queries (+inf behind the sequence)
  __shared__ __attribute__((aligned(16))) float sD[64];            // their D
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fq = lane & 15, fg = lane >> 4;
  const int kb = (int)(blockIdx.x / BH);                    // heaviest (first) key blocks first
  const int bh = (int)(blockIdx.x % BH), b = bh / H, h = bh - b * H;
  const int d = H * DH;
  const bf16* Qg = qkv + (size_t)b * T * ld + h * DH;
  const bf16* Gg = dctx + (size_t)b * T * d + h * DH;
  const int key = kb * 64 + wid * 16 + fq;
  const bool kok = key < T;
  bf16x8 kf[Cf::KK], vf[Cf::KK];
#pragma unroll
  for (int kk = 0; kk < Cf::KK; ++kk) {
    kf[kk] = kok ? *reinterpret_cast<const bf16x8*>(Qg + d + (size_t)key * ld + 32 * kk + 8 * fg) : ca_zero8();
    vf[kk] = kok ? *reinterpret_cast<const bf16x8*>(Qg + 2 * d + (size_t)key * ld + 32 * kk + 8 * fg) : ca_zero8();
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
  bf16x8 qr[Cf::CPT], gr[Cf::CPT];
  tile_fetch<DH>(Qg, ld, kb * 64, T, tid, qr);
  tile_fetch<DH>(Gg, d, kb * 64, T, tid, gr);
  for (int qt = kb; qt < nqb; ++qt) {
    __syncthreads();
    tile_put<DH>(sQ, tid, qr);
    tile_put<DH>(sG, tid, gr);
    if (tid < 64) {
      const int qq = qt * 64 + tid;
      const bool ok = qq < T;
      sL[tid] = ok ? lse[(size_t)bh * T + qq] : INFINITY;
      sD[tid] = ok ? *reinterpret_cast<const float*>(dqkv + ((size_t)b * T + qq) * ld_dq + h * DH) : 0.f;
    }
    __syncthreads();
    if (qt + 1 < nqb) {
      tile_fetch<DH>(Qg, ld, (qt + 1) * 64, T, tid, qr);
      tile_fetch<DH>(Gg, d, (qt + 1) * 64, T, tid, gr);
    }
    const bool diag = qt == kb;
    const int t0 = diag ? wid : 0;           // first 16-query sub-tile at or behind this wave's keys
    f32x4 sc[4], dp[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) sc[t] = dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < Cf::KK; ++kk) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (t >= t0) {
          const bf16x8 qf = *reinterpret_cast<const bf16x8*>(sQ + t * 16 * Cf::ROWB + r_off[kk]);
          const bf16x8 gf = *reinterpret_cast<const bf16x8*>(sG + t * 16 * Cf::ROWB + r_off[kk]);
          sc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf, kf[kk], sc[t], 0, 0, 0);      // S[query 4fg + r][key fq]
          dp[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gf, vf[kk], dp[t], 0, 0, 0);      // dPd[query][key]
        }
    }
    float pd[4][4], ds[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (t >= t0) {
        const f32x4 l4 = *reinterpret_cast<const f32x4*>(sL + 16 * t + 4 * fg);
        const f32x4 d4 = *reinterpret_cast<const f32x4*>(sD + 16 * t + 4 * fg);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qq = qt * 64 + 16 * t + 4 * fg + r;
          float p = __expf(sc[t][r] - l4[r]);
          if (diag && t == wid) p = (4 * fg + r >= fq) ? p : 0.f;
          float keepf = 1.f;
          if (thresh24 != 0)
            keepf = m3p_keep((uint32_t)(bh * T + qq) * (uint32_t)T + (uint32_t)key, seed, thresh24) ? inv_keep : 0.f;
          pd[t][r] = p * keepf;
          ds[t][r] = p * (dp[t][r] * keepf - d4[r]);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) pd[t][r] = ds[t][r] = 0.f;
      }
    }
#pragma unroll
    for (int kk2 = 0; kk2 < 2; ++kk2)
      if (2 * kk2 + 1 >= t0) {
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
  if (kok) {
    bf16* krow = dqkv + ((size_t)b * T + key) * ld_dq + d + h * DH + 4 * fg;
#pragma unroll
    for (int n = 0; n < Cf::NT; ++n) {
      *reinterpret_cast<bf16x4*>(krow + 16 * n) = bf16x4{(bf16)dk[n][0], (bf16)dk[n][1], (bf16)dk[n][2], (bf16)dk[n][3]};
      *reinterpret_cast<bf16x4*>(krow + d + 16 * n) = bf16x4{(bf16)dv[n][0], (bf16)dv[n][1], (bf16)dv[n][2], (bf16)dv[n][3]};
    }
  }
}

// shapes outside the tiled kernels' range are "not implemented", so that a caller can take the rows kernels instead
int ca_admit(int B, int T, int H, int dh) {
  if (B <= 0 || T <= 0 || H <= 0) return M3P_EINVAL;
  if ((dh != 32 && dh != 64) || T > CA_MAX_T) return M3P_ENOTIMPL;
  if ((unsigned long long)B * H * T * T >= (1ull << 32)) return M3P_ENOTIMPL;       // 32-bit dropout stream index
  return M3P_OK;
}

}  // namespace

extern "C" {

int m3p_attn_causal_fwd(const void* qkv, int ld_qkv, void* ctx, float* lse, int B, int T, int H, int dh, uint32_t seed,
                        uint32_t thresh24, float inv_keep, void* stream) {
  if (!qkv || !ctx || !lse) return M3P_EINVAL;
  const int rc = ca_admit(B, T, H, dh);
  if (rc != M3P_OK) return rc;
  if ((ld_qkv % 8) != 0 || ld_qkv < 3 * H * dh || ((uintptr_t)qkv & 15) || ((uintptr_t)ctx & 15)) return M3P_ENOTIMPL;
  const int nqb = (T + 63) / 64, BH = B * H;
  const dim3 grid((unsigned)(nqb * BH)), block(256);
  if (dh == 64)
    hipLaunchKernelGGL(attn_causal_fwd_kernel<64>, grid, block, 0, (hipStream_t)stream, (const bf16*)qkv, ld_qkv, (bf16*)ctx, lse,
                       T, H, BH, nqb, seed, thresh24, inv_keep);
  else
    hipLaunchKernelGGL(attn_causal_fwd_kernel<32>, grid, block, 0, (hipStream_t)stream, (const bf16*)qkv, ld_qkv, (bf16*)ctx, lse,
                       T, H, BH, nqb, seed, thresh24, inv_keep);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

int m3p_attn_causal_bwd(const void* qkv, int ld_qkv, const void* dctx, const float* lse, void* dqkv, int ld_dqkv, int B, int T,
                        int H, int dh, float qscale, uint32_t seed, uint32_t thresh24, float inv_keep, void* stream) {
  if (!qkv || !dctx || !lse || !dqkv) return M3P_EINVAL;
  const int rc = ca_admit(B, T, H, dh);
  if (rc != M3P_OK) return rc;
  if ((ld_qkv % 8) != 0 || ld_qkv < 3 * H * dh || (ld_dqkv % 8) != 0 || ld_dqkv < 3 * H * dh || ((uintptr_t)qkv & 15) ||
      ((uintptr_t)dctx & 15) || ((uintptr_t)dqkv & 15))
    return M3P_ENOTIMPL;
  const int nqb = (T + 63) / 64, BH = B * H;
  const dim3 grid((unsigned)(nqb * BH)), block(256);
  hipStream_t st = (hipStream_t)stream;
#define CA_BWD(DH_)                                                                                                              \
  do {                                                                                                                           \
    hipLaunchKernelGGL((attn_causal_bwd_q_kernel<DH_, false>), grid, block, 0, st, (const bf16*)qkv, ld_qkv, (const bf16*)dctx,  \
                       lse, (bf16*)dqkv, ld_dqkv, T, H, BH, nqb, qscale, seed, thresh24, inv_keep);                              \
    hipLaunchKernelGGL(attn_causal_bwd_kv_kernel<DH_>, grid, block, 0, st, (const bf16*)qkv, ld_qkv, (const bf16*)dctx, lse,     \
                       (bf16*)dqkv, ld_dqkv, T, H, BH, nqb, seed, thresh24, inv_keep);                                           \
    hipLaunchKernelGGL((attn_causal_bwd_q_kernel<DH_, true>), grid, block, 0, st, (const bf16*)qkv, ld_qkv, (const bf16*)dctx,   \
                       lse, (bf16*)dqkv, ld_dqkv, T, H, BH, nqb, qscale, seed, thresh24, inv_keep);                              \
  } while (0)
  if (dh == 64) CA_BWD(64);
  else CA_BWD(32);
#undef CA_BWD
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

}  // extern "C"
