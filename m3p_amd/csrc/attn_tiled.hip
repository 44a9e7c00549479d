// Tiled attention (forward + backward) of the teacher-forced decoder passes on gfx950, one kernel body for both masks:
//   CAUSAL   the self-attention: the decoder-only pass of the causal language-model objective (crossfwd(stream_='text',
//            causal=True) without a source encoding: xtrainer.py:694-732) and the self-attention sub-layer of the seq2seq
//            steps' pass over a source encoding, training and cache-less scoring alike.  T rows of a packed q | k | v
//            buffer, query t attends keys <= t.
//   source   the encoder-attention sub-layer of the seq2seq steps (crossfwd(..., src_enc=...), transformer.py:149-210 with
//            kv = the source encoding): Tq query rows of every (sequence, head) attend the first nk = min(klen[b], Lk) rows
//            of a separate key | value tensor, no causal mask.
//   prefix   (forward only) the prefill of a prompted decoding call: Tq new queries behind pos0 positions of a key | value
//            cache that already holds the new rows; query t attends keys 0 .. pos0 + t.  The causal mask shifted by pos0, so
//            the diagonal is not tile-aligned: it is classified per wave and 16-key sub-tile (attn_fwd_body).
//
// The rows kernels of decode.hip serve short target sequences: a wave per (sequence, head, query), no MFMAs, and a backward
// that adds dk / dv with two 64-float atomics per (query, key) pair.  This file computes what m3p_attn_rows_fwd / _bwd
// (pos0 = 0; causal = 1, klen = NULL, Lk = T for the self-attention, causal = 0 over the source) compute, with their layouts
// and their dropout stream index ((b*H + h)*Tq + t)*Lk + key, on v_mfma_f32_16x16x32_bf16 with no atomics and nothing
// Tq x Lk stored.  The kernels know one addressing - q, k | v with a batch stride and a row pitch, dq, dk | dv - and the
// causal launchers describe the packed buffer in it: k | v = qkv + d, dk | dv = dqkv + d, Lk = T, no klen.
//
// Blocks of 64: a workgroup (four waves) owns 64 queries - or, for dk / dv, 64 keys - of one (sequence, head), a wave 16 of
// them, and walks the 64-row tiles of the other side that the mask leaves.
//   CAUSAL   keys at and below the diagonal for a query block, queries at and behind it for a key block.  Tiles wholly above
//            the diagonal are never visited, and inside the diagonal tile a wave skips the 16-row sub-tiles above its own
//            rows and masks its own sub-tile per element (one compare: a lane owns a column).  Causal work grows with the
//            query block: query block ids are handed out heaviest first.
//   source   the loop bounds come from klen[b] and are workgroup-uniform (scalar): key tiles wholly at or past nk are never
//            visited, in the last one the 16-key sub-tiles past nk are skipped and the ragged one is masked per element.
//            Waves whose 16 rows all lie behind Tq (or nk) only move tiles.  klen[b] == 0: ctx = 0, lse = 0, dq = 0,
//            dkv = 0, like the rows kernels.
// A tile goes global -> registers -> LDS, row-major with the 16-byte chunk swizzle of attention.hip; the next tile's loads
// are in flight while the current one is computed on.  Key / value rows at or past nk enter LDS and registers as ZEROS (the
// bound of the fetch is nk, not Lk): the source encoding may hold anything there, NaN included, and a masked probability of
// 0 would not stop 0 x NaN.
//   forward     S^T = K Q^T (lane = query column), online softmax over the key tiles in fp32, P -> bf16 straight back as the
//               B operand of O^T = V^T P^T (V through transposing LDS reads, same k-slot permutation as attention.hip)
//   backward 1  query blocks: D[t] = sum_j p_tj dPd_tj in fp32 (there is no ctx argument to take rowsum(dO * O) from), parked
//               as one float in the first four bytes of the row's dq slot of (b, t, h) - dq is the only buffer the ABI has
//   backward 2  key blocks over all Lk keys: S = Q K^T and dPd = dO V^T un-swapped (lane = key column), p = exp(S - lse),
//               then dV^T += dO^T Pd, dK^T += Q^T dS over the query tiles; the owner rounds its fp32 accumulators once and
//               stores the row - exact zeros for keys >= nk, so the caller zeroes nothing and casts nothing
//   backward 3  query blocks again: dS^T recomputed from the parked D, dQ^T += K^T dS^T, then every dq row is written over
//               its parked D (a lane reads the D of its own row only, before the loop)
#include "common.hpp"

namespace {

constexpr int CA_MAX_T = 512;            // query rows: the position table of the model has 514 rows
constexpr int XA_MAX_KEYS = 1024;        // source keys: the rows kernels' own cap (QA_MAX_KEYS), they stay a complete fallback
constexpr float CA_MASKED = -1.0e30f;    // score of a masked key: exp of it minus any finite maximum is exactly 0

// A 64-row tile of one head slice in LDS, row-major with the 16-byte chunk swizzle of attention.hip; fragments come back as
// row reads (A operands) or transposing reads (ds_read_tr16_b64).
template <int DH> struct CaCfg {
  static constexpr int ROWB = DH * 2;        // bytes per row of a tile in LDS
  static constexpr int CH = DH / 8;          // 16-B chunks per row
  static constexpr int KK = DH / 32;         // MFMA k-steps across the head dim
  static constexpr int NT = DH / 16;         // 16-wide tiles across the head dim
  static constexpr int CPT = 64 * CH / 256;  // chunks of a 64-row tile per thread
  static constexpr int TILEB = 64 * ROWB;
  // chunk swizzle (only needed, and only bijective within a row, for 128-B rows): as AttnCfg of attention.hip
  static __device__ __forceinline__ int swz(int chunk, int row) { return DH == 64 ? (chunk ^ (row & 7)) : chunk; }
};

__device__ __forceinline__ bf16x4 ca_tr16(const char* p) {
  s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(p));
  return __builtin_bit_cast(bf16x4, v);
}
__device__ __forceinline__ bf16x8 ca_cat8(bf16x4 a, bf16x4 b) {
  return bf16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}
__device__ __forceinline__ bf16x8 ca_pack8(const float (&p)[8]) {
  return bf16x8{(bf16)p[0], (bf16)p[1], (bf16)p[2], (bf16)p[3], (bf16)p[4], (bf16)p[5], (bf16)p[6], (bf16)p[7]};
}
__device__ __forceinline__ bf16x8 ca_zero8() { return bf16x8{0, 0, 0, 0, 0, 0, 0, 0}; }
__device__ __forceinline__ bf16x4 ca_round4(f32x4 v, float s) {
  return bf16x4{(bf16)(v[0] * s), (bf16)(v[1] * s), (bf16)(v[2] * s), (bf16)(v[3] * s)};
}

// rows row0 .. row0 + 63 of a head slice (rows `ld` elements apart) into registers, rows >= T as zeros ...
template <int DH>
__device__ __forceinline__ void tile_fetch(const bf16* __restrict__ g, size_t ld, int row0, int T, int tid,
                                           bf16x8 (&r)[CaCfg<DH>::CPT]) {
  using Cf = CaCfg<DH>;
#pragma unroll
  for (int j = 0; j < Cf::CPT; ++j) {
    const int i = tid + 256 * j, row = row0 + i / Cf::CH, c = i % Cf::CH;
    r[j] = row < T ? *reinterpret_cast<const bf16x8*>(g + (size_t)row * ld + c * 8) : ca_zero8();
  }
}
// ... and from there into the LDS tile [64][DH], chunks swizzled
template <int DH>
__device__ __forceinline__ void tile_put(char* lds, int tid, const bf16x8 (&r)[CaCfg<DH>::CPT]) {
  using Cf = CaCfg<DH>;
#pragma unroll
  for (int j = 0; j < Cf::CPT; ++j) {
    const int i = tid + 256 * j, row = i / Cf::CH, c = i % Cf::CH;
    *reinterpret_cast<bf16x8*>(lds + row * Cf::ROWB + Cf::swz(c, row) * 16) = r[j];
  }
}
// rows 32 kk2 .. 32 kk2 + 31 of a tile, transposed, as the A operand of d-tile n
template <int DH> __device__ __forceinline__ bf16x8 tr_frag(const char* tile, int kk2, int tr_off) {
  const char* p = tile + kk2 * 32 * CaCfg<DH>::ROWB + tr_off;
  return ca_cat8(ca_tr16(p), ca_tr16(p + 16 * CaCfg<DH>::ROWB));
}

// keep factors (inv_keep or 0) of four consecutive keys of one query row
__device__ __forceinline__ void keep4(uint32_t base, uint32_t seed, uint32_t thresh24, float inv_keep, float (&f)[4]) {
  bool k4[4];
  m3p_keep_run<4>(base, seed, thresh24, k4);
#pragma unroll
  for (int r = 0; r < 4; ++r) f[r] = k4[r] ? inv_keep : 0.f;
}

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

// Waves per SIMD asked of the compiler (0 = not asked), per kernel and mask:
//   forward       source 4: left alone the DH = 64 instantiation takes 160 registers - three - and with the cap 128, still
//                 without scratch, like the causal forward, which gets there unasked
//   query blocks  source three (D) / two (dQ): one more than that spills at DH = 64, left alone both passes take two
//   prefix fwd    not asked (CA_PREFIX_WAVES = 0, launch bounds 256 threads): DH = 64 takes 108 registers - four waves -, DH = 32
//                 72 - five -, both without scratch: the occupancy of the causal forward
//   key blocks    two for both: left alone the DH = 64 instantiation takes 276 registers - one wave per SIMD - and with the
//                 cap 198 (causal), still without scratch
// (The causal query-block kernels are also told that the pitches are positive, which the launchers have checked: row * pitch in the tile
//  fetches then stays the one 32 x 32 -> 64 multiply it was in these kernels, not three instructions.  The source kernels are
//  left as they were compiled.)
enum CaKernel { CA_FWD, CA_BWD_D, CA_BWD_DQ, CA_BWD_KV };
constexpr int ca_waves(CaKernel k, bool causal) {
  return k == CA_BWD_KV ? 2 : causal ? 0 : k == CA_FWD ? 4 : k == CA_BWD_D ? 3 : 2;
}
// The forward body knows three masks; the third, the prefix mask of a prefill (m3p_attn_prefix_fwd: Tq new queries behind pos0
// cached positions, query t sees keys 0 .. pos0 + t), has a forward only and its own kernel name around the same body.
enum CaMask { CA_SOURCE = 0, CA_CAUSAL = 1, CA_PREFIX = 2 };
constexpr int CA_PREFIX_WAVES = 0;

// query block of a workgroup.  Causal work grows with the query block: heaviest (last) query blocks first.  (Key blocks are
// handed out in plain order under both masks: causal work shrinks with the key block.)
template <bool CAUSAL> __device__ __forceinline__ int query_block(int BH, int Tq) {
  const int i = (int)(blockIdx.x / BH);
  if constexpr (CAUSAL) return ((Tq + 63) >> 6) - 1 - i;
  else return i;
}

// ---------------------------------------------------------------------------------------
// forward: workgroup = (sequence, head, 64-query block), wave = 16 queries, lane = query column fq, keys 4 fg + r of a tile
// ---------------------------------------------------------------------------------------
template <int DH, int MASK>
__device__ __forceinline__ void attn_fwd_body(
    const bf16* __restrict__ q, int ld_q, const bf16* __restrict__ kv, long long kv_bstride, int ld_kv,
    const int32_t* __restrict__ klen, bf16* __restrict__ ctx, float* __restrict__ lse, int Tq, int H, int BH, int Lk,
    uint32_t seed, uint32_t thresh24, float inv_keep) {
  using Cf = CaCfg<DH>;
  constexpr bool CAUSAL = MASK == CA_CAUSAL, PREFIX = MASK == CA_PREFIX;
  __shared__ __attribute__((aligned(16))) char sK[Cf::TILEB];
  __shared__ __attribute__((aligned(16))) char sV[Cf::TILEB];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fq = lane & 15, fg = lane >> 4;
  const int qb = query_block<CAUSAL || PREFIX>(BH, Tq);
  const int bh = (int)(blockIdx.x % BH), b = bh / H, h = bh - b * H;
  const int d = H * DH;
  if constexpr (CAUSAL || PREFIX) __builtin_assume(ld_q > 0 && ld_kv > 0);      // (see ca_waves)
  const int nk = (CAUSAL || PREFIX) ? Lk : xa_nkeys(klen, b, Lk);      // (causal, prefix: every key exists, klen is not read)
  const int pos0 = Lk - Tq;      // prefix: query t sits at position pos0 + t of the cache
  // key tiles: up to the diagonal (prefix: of the block's last existing row) / holding a key
  const int nkt = CAUSAL ? qb + 1 : PREFIX ? ((pos0 + min(64 * qb + 63, Tq - 1)) >> 6) + 1 : (nk + 63) >> 6;
  const bf16* Qg = q + (size_t)b * Tq * ld_q + h * DH;
  const bf16* Kg = kv + (size_t)b * kv_bstride + h * DH;
  const bf16* Vg = Kg + d;
  const int qrow = qb * 64 + wid * 16 + fq;
  const bool wave_on = CAUSAL || qb * 64 + wid * 16 < Tq;      // source, prefix: (wave-uniform) at least one of this wave's rows exists
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
    // 16-key sub-tiles 0 .. nsub - 1 are computed (every wave has sub-tile 0), the last of them masked per element where
    // the tile is the diagonal one (causal: sub-tiles at or below this wave's queries) or the ragged last one (source).
    // Prefix: the diagonal of this wave's first row enters the tile at key dlt (wave-uniform; negative: the tile lies above
    // the wave, beyond 63: below it).  Sub-tiles 0 .. nfull - 1 are wholly visible to all 16 rows, nfull .. nsub - 1 (at most
    // two, and they may fall into two key tiles) are crossed by the diagonal and masked per element, the rest is skipped;
    // tile 0 always has nsub >= 1 (key 0 is visible to every query), so m is finite from the first tile on.
    const bool diag = CAUSAL && kt == qb;
    const int rem = (CAUSAL || PREFIX) ? 64 : nk - 64 * kt;        // keys of this tile that exist (>= 1)
    const int dlt = PREFIX ? pos0 + qb * 64 + wid * 16 - 64 * kt : 0;
    const int nfull = PREFIX ? (dlt + 1) >> 4 : 0;
    const int nsub = CAUSAL ? (diag ? wid + 1 : 4) : PREFIX ? min(max((dlt + 31) >> 4, 0), 4) : (rem >= 64 ? 4 : (rem + 15) >> 4);
    if (PREFIX && nsub == 0) continue;
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
      } else if (CAUSAL ? diag && t == wid : PREFIX ? t >= nfull : t == nsub - 1 && rem < 64) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          s[t][r] = (CAUSAL ? 4 * fg + r <= fq : PREFIX ? 16 * t + 4 * fg + r <= dlt + fq : 16 * t + 4 * fg + r < rem) ? s[t][r]
                                                                                                                    : CA_MASKED;
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
        if (!PREFIX && thresh24 != 0 && t < nsub) keep4(rbase + (uint32_t)(64 * kt + 16 * t + 4 * fg), seed, thresh24, 1.f, kf4);
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
        for (int n = 0; n < Cf::NT; ++n)
          o[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag<DH>(sV, kk2, v_off[n]), pf[kk2], o[n], 0, 0, 0);
      }
  }
  if (qrow < Tq) {
    // (nk == 0 - a sequence without keys: the loop never ran, l = 0 - gives ctx = 0 and lse = 0 like the rows kernels)
    const bool keys = CAUSAL || PREFIX || nk > 0;
    const float inv = keys ? inv_keep / l : 0.f;
    bf16* orow = ctx + ((size_t)b * Tq + qrow) * d + h * DH + 4 * fg;
#pragma unroll
    for (int n = 0; n < Cf::NT; ++n) *reinterpret_cast<bf16x4*>(orow + 16 * n) = ca_round4(o[n], inv);
    if (fg == 0 && (!PREFIX || lse)) lse[(size_t)bh * Tq + qrow] = keys ? m + __logf(l) : 0.f;      // (prefix: lse may be NULL)
  }
}

// The kernels around the one body.  attn_fwd_kernel<DH, CAUSAL> keeps its name, template parameters and arguments: the
// resource test reads its four instantiations off their mangled names.
template <int DH, bool CAUSAL>
__global__ __launch_bounds__(256, ca_waves(CA_FWD, CAUSAL)) void attn_fwd_kernel(
    const bf16* __restrict__ q, int ld_q, const bf16* __restrict__ kv, long long kv_bstride, int ld_kv,
    const int32_t* __restrict__ klen, bf16* __restrict__ ctx, float* __restrict__ lse, int Tq, int H, int BH, int Lk,
    uint32_t seed, uint32_t thresh24, float inv_keep) {
  attn_fwd_body<DH, CAUSAL ? CA_CAUSAL : CA_SOURCE>(q, ld_q, kv, kv_bstride, ld_kv, klen, ctx, lse, Tq, H, BH, Lk, seed, thresh24,
                                                    inv_keep);
}
// the prefix mask: Lk = pos0 + Tq keys, no klen, no dropout
template <int DH>
__global__ __launch_bounds__(256, CA_PREFIX_WAVES) void attn_prefix_fwd_kernel(
    const bf16* __restrict__ q, int ld_q, const bf16* __restrict__ kv, long long kv_bstride, int ld_kv, bf16* __restrict__ ctx,
    float* __restrict__ lse, int Tq, int H, int BH, int Lk) {
  attn_fwd_body<DH, CA_PREFIX>(q, ld_q, kv, kv_bstride, ld_kv, nullptr, ctx, lse, Tq, H, BH, Lk, 0u, 0u, 1.f);
}

// ---------------------------------------------------------------------------------------
// backward, query blocks (same orientation as the forward).  DQ = false: D[t] = sum_j p_tj dPd_tj, parked in the dq slot;
// DQ = true: dS^T from the parked D, dQ^T[d][q] = sum_key K[key][d] dS[q][key], times qscale (q was stored pre-scaled).
// ---------------------------------------------------------------------------------------
template <int DH, bool CAUSAL, bool DQ>
__global__ __launch_bounds__(256, ca_waves(DQ ? CA_BWD_DQ : CA_BWD_D, CAUSAL)) void attn_bwd_q_kernel(
    const bf16* __restrict__ q, int ld_q, const bf16* __restrict__ kv, long long kv_bstride, int ld_kv,
    const int32_t* __restrict__ klen, const bf16* __restrict__ dctx, const float* __restrict__ lse, bf16* __restrict__ dq,
    int ld_dq, int Tq, int H, int BH, int Lk, float qscale, uint32_t seed, uint32_t thresh24, float inv_keep) {
  using Cf = CaCfg<DH>;
  __shared__ __attribute__((aligned(16))) char sK[Cf::TILEB];
  __shared__ __attribute__((aligned(16))) char sV[Cf::TILEB];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fq = lane & 15, fg = lane >> 4;
  const int qb = query_block<CAUSAL>(BH, Tq);
  const int bh = (int)(blockIdx.x % BH), b = bh / H, h = bh - b * H;
  const int d = H * DH;
  if constexpr (CAUSAL) __builtin_assume(ld_q > 0 && ld_kv > 0);      // (see ca_waves)
  const int nk = CAUSAL ? Lk : xa_nkeys(klen, b, Lk);      // (causal: every key exists, klen is not read)
  const int nkt = CAUSAL ? qb + 1 : (nk + 63) >> 6;
  const bf16* Qg = q + (size_t)b * Tq * ld_q + h * DH;
  const bf16* Kg = kv + (size_t)b * kv_bstride + h * DH;
  const bf16* Vg = Kg + d;
  const int qrow = qb * 64 + wid * 16 + fq;
  const bool qok = qrow < Tq;
  const bool wave_on = CAUSAL || qb * 64 + wid * 16 < Tq;
  bf16x8 qf[Cf::KK], gf[Cf::KK];
#pragma unroll
  for (int kk = 0; kk < Cf::KK; ++kk) {
    qf[kk] = qok ? *reinterpret_cast<const bf16x8*>(Qg + (size_t)qrow * ld_q + 32 * kk + 8 * fg) : ca_zero8();
    gf[kk] = qok ? *reinterpret_cast<const bf16x8*>(dctx + ((size_t)b * Tq + qrow) * d + h * DH + 32 * kk + 8 * fg) : ca_zero8();
  }
  bf16* dqrow = dq + ((size_t)b * Tq + (qok ? qrow : 0)) * ld_dq + h * DH;
  const float lq = qok ? lse[(size_t)bh * Tq + qrow] : INFINITY;       // a row behind the sequence: p = exp(s - inf) = 0
  // (source: without keys the loop never runs and no barrier separates this read from the row's store: D is not read then)
  float Dq = (DQ && qok && (CAUSAL || nk > 0)) ? *reinterpret_cast<const float*>(dqrow) : 0.f;
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
    const bool diag = CAUSAL && kt == qb;              // sub-tiles and their masks as in the forward
    const int rem = CAUSAL ? 64 : nk - 64 * kt;
    const int nsub = CAUSAL ? (diag ? wid + 1 : 4) : (rem >= 64 ? 4 : (rem + 15) >> 4);
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
          if (CAUSAL ? diag && t == wid : t == nsub - 1 && rem < 64)
            p = (CAUSAL ? 4 * fg + r <= fq : 16 * t + 4 * fg + r < rem) ? p : 0.f;
          // gradient wrt p through the dropout (causal: left to the fusion as it always was, kept for bit-compatibility)
          const float dpd = CAUSAL ? dp[t][r] * kf4[r] : xa_rounded(dp[t][r] * kf4[r]);
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
          for (int n = 0; n < Cf::NT; ++n)
            dqa[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag<DH>(sK, kk2, v_off[n]), sf, dqa[n], 0, 0, 0);
        }
    }
  }
  if (DQ) {
    if (qok) {
#pragma unroll
      for (int n = 0; n < Cf::NT; ++n) *reinterpret_cast<bf16x4*>(dqrow + 16 * n + 4 * fg) = ca_round4(dqa[n], qscale);
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
// over the query tiles the mask leaves - causal: at and behind the diagonal; source: all of them, none for a block wholly at
// or past nk; P and dS of a tile go from the accumulators straight into the B operands.  Every key < Lk is stored, the ones
// >= nk as zeros.
// ---------------------------------------------------------------------------------------
template <int DH, bool CAUSAL>
__global__ __launch_bounds__(256, ca_waves(CA_BWD_KV, CAUSAL)) void attn_bwd_kv_kernel(
    const bf16* __restrict__ q, int ld_q, const bf16* __restrict__ kv, long long kv_bstride, int ld_kv,
    const int32_t* __restrict__ klen, const bf16* __restrict__ dctx, const float* __restrict__ lse,
    const bf16* __restrict__ dq, int ld_dq, bf16* __restrict__ dkv, int ld_dkv, int Tq, int H, int BH, int Lk, uint32_t seed,
    uint32_t thresh24, float inv_keep) {
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
  const int nk = CAUSAL ? Lk : xa_nkeys(klen, b, Lk);      // (causal: every key exists, klen is not read)
  // (causal: as many key blocks as query blocks, and the count is read off the grid.  Computed from Tq its range is known
  //  to the compiler, which then strength-reduces the query loop: DH = 32 goes from 114 to 148 registers, 4 waves to 3)
  const int nqb = CAUSAL ? (int)(gridDim.x / BH) : (Tq + 63) >> 6;
  const bf16* Qg = q + (size_t)b * Tq * ld_q + h * DH;
  const bf16* Gg = dctx + (size_t)b * Tq * d + h * DH;
  const bf16* Kg = kv + (size_t)b * kv_bstride + h * DH;
  const int key = kb * 64 + wid * 16 + fq;
  const bool kok = key < nk;
  const bool wave_on = CAUSAL || kb * 64 + wid * 16 < nk;      // source: (wave-uniform) at least one of this wave's keys exists
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
  // (workgroup-uniform) query tiles qt0 .. nqt - 1: causal from the diagonal on; source all, and a block without keys walks
  // nothing and fetches nothing
  const int qt0 = CAUSAL ? kb : 0;
  const int nqt = (CAUSAL || kb * 64 < nk) ? nqb : 0;
  bf16x8 qr[Cf::CPT], gr[Cf::CPT];
  tile_fetch<DH>(Qg, ld_q, qt0 * 64, nqt > 0 ? Tq : 0, tid, qr);
  tile_fetch<DH>(Gg, d, qt0 * 64, nqt > 0 ? Tq : 0, tid, gr);
  for (int qt = qt0; qt < nqt; ++qt) {
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
    // 16-query sub-tiles t0 .. nsub - 1 are computed
    int t0 = 0, nsub = 4;
    bool diag = false;
    if constexpr (CAUSAL) {
      diag = qt == kb;
      t0 = diag ? wid : 0;                       // first 16-query sub-tile at or behind this wave's keys
    } else {
      const int remq = Tq - 64 * qt;             // queries of this tile that exist (>= 1)
      nsub = remq >= 64 ? 4 : (remq + 15) >> 4;  // 16-query sub-tiles holding one
    }
    f32x4 sc[4], dp[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) sc[t] = dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < Cf::KK; ++kk) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (t >= t0 && t < nsub) {
          const bf16x8 qf = *reinterpret_cast<const bf16x8*>(sQ + t * 16 * Cf::ROWB + r_off[kk]);
          const bf16x8 gf = *reinterpret_cast<const bf16x8*>(sG + t * 16 * Cf::ROWB + r_off[kk]);
          sc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf, kf[kk], sc[t], 0, 0, 0);      // S[query 4fg + r][key fq]
          dp[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gf, vf[kk], dp[t], 0, 0, 0);      // dPd[query][key]
        }
    }
    float pd[4][4], ds[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (t >= t0 && t < nsub) {
        const f32x4 l4 = *reinterpret_cast<const f32x4*>(sL + 16 * t + 4 * fg);
        const f32x4 d4 = *reinterpret_cast<const f32x4*>(sD + 16 * t + 4 * fg);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qq = qt * 64 + 16 * t + 4 * fg + r;
          float p = __expf(sc[t][r] - l4[r]);
          if constexpr (CAUSAL) {
            if (diag && t == wid) p = (4 * fg + r >= fq) ? p : 0.f;
          } else {
            p = kok ? p : 0.f;       // (a key >= nk: its column is not part of the softmax)
          }
          float keepf = 1.f;
          if (thresh24 != 0)
            keepf = m3p_keep((uint32_t)(bh * Tq + qq) * (uint32_t)Lk + (uint32_t)key, seed, thresh24) ? inv_keep : 0.f;
          const float dpd = CAUSAL ? dp[t][r] * keepf : xa_rounded(dp[t][r] * keepf);      // (as in the query-block kernel)
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
      if (2 * kk2 + 1 >= t0 && 2 * kk2 < nsub) {      // one of the pair's two sub-tiles was computed
        const float p8[8] = {pd[2 * kk2][0], pd[2 * kk2][1], pd[2 * kk2][2], pd[2 * kk2][3],
                             pd[2 * kk2 + 1][0], pd[2 * kk2 + 1][1], pd[2 * kk2 + 1][2], pd[2 * kk2 + 1][3]};
        const float s8[8] = {ds[2 * kk2][0], ds[2 * kk2][1], ds[2 * kk2][2], ds[2 * kk2][3],
                             ds[2 * kk2 + 1][0], ds[2 * kk2 + 1][1], ds[2 * kk2 + 1][2], ds[2 * kk2 + 1][3]};
        const bf16x8 pf = ca_pack8(p8), sf = ca_pack8(s8);
#pragma unroll
        for (int n = 0; n < Cf::NT; ++n) {
          const bf16x8 gT = tr_frag<DH>(sG, kk2, t_off[n]), qT = tr_frag<DH>(sQ, kk2, t_off[n]);
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
int ca_admit(int B, int Tq, int H, int dh, int Lk) {
  if (B <= 0 || Tq <= 0 || H <= 0 || Lk <= 0) return M3P_EINVAL;
  if ((dh != 32 && dh != 64) || Tq > CA_MAX_T || Lk > XA_MAX_KEYS) return M3P_ENOTIMPL;
  if ((unsigned long long)B * H * Tq * Lk >= (1ull << 32)) return M3P_ENOTIMPL;       // 32-bit dropout stream index
  return M3P_OK;
}
inline bool ca_misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

template <int DH, bool CAUSAL>
void ca_launch_fwd(hipStream_t st, const bf16* q, int ld_q, const bf16* kv, long long kv_bstride, int ld_kv, const int32_t* klen,
                   bf16* ctx, float* lse, int B, int Tq, int H, int Lk, uint32_t seed, uint32_t thresh24, float inv_keep) {
  const int BH = B * H;
  hipLaunchKernelGGL((attn_fwd_kernel<DH, CAUSAL>), dim3((unsigned)((Tq + 63) / 64 * BH)), dim3(256), 0, st, q, ld_q, kv,
                     kv_bstride, ld_kv, klen, ctx, lse, Tq, H, BH, Lk, seed, thresh24, inv_keep);
}
template <int DH, bool CAUSAL>
void ca_launch_bwd(hipStream_t st, const bf16* q, int ld_q, const bf16* kv, long long kv_bstride, int ld_kv, const int32_t* klen,
                   const bf16* dctx, const float* lse, bf16* dq, int ld_dq, bf16* dkv, int ld_dkv, int B, int Tq, int H, int Lk,
                   float qscale, uint32_t seed, uint32_t thresh24, float inv_keep) {
  const int BH = B * H;
  const dim3 gridq((unsigned)((Tq + 63) / 64 * BH)), gridk((unsigned)((Lk + 63) / 64 * BH)), block(256);
  hipLaunchKernelGGL((attn_bwd_q_kernel<DH, CAUSAL, false>), gridq, block, 0, st, q, ld_q, kv, kv_bstride, ld_kv, klen, dctx, lse,
                     dq, ld_dq, Tq, H, BH, Lk, qscale, seed, thresh24, inv_keep);
  hipLaunchKernelGGL((attn_bwd_kv_kernel<DH, CAUSAL>), gridk, block, 0, st, q, ld_q, kv, kv_bstride, ld_kv, klen, dctx, lse,
                     (const bf16*)dq, ld_dq, dkv, ld_dkv, Tq, H, BH, Lk, seed, thresh24, inv_keep);
  hipLaunchKernelGGL((attn_bwd_q_kernel<DH, CAUSAL, true>), gridq, block, 0, st, q, ld_q, kv, kv_bstride, ld_kv, klen, dctx, lse,
                     dq, ld_dq, Tq, H, BH, Lk, qscale, seed, thresh24, inv_keep);
}
// the launch of one mask at the head dim asked for (32 or 64: ca_admit has seen to that)
template <bool CAUSAL, class... A> int ca_fwd(int dh, A... a) {
  if (dh == 64) ca_launch_fwd<64, CAUSAL>(a...);
  else ca_launch_fwd<32, CAUSAL>(a...);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}
template <int DH>
void ca_launch_prefix_fwd(hipStream_t st, const bf16* q, int ld_q, const bf16* kv, long long kv_bstride, int ld_kv, bf16* ctx,
                          float* lse, int B, int Tq, int H, int Lk) {
  const int BH = B * H;
  hipLaunchKernelGGL((attn_prefix_fwd_kernel<DH>), dim3((unsigned)((Tq + 63) / 64 * BH)), dim3(256), 0, st, q, ld_q, kv, kv_bstride,
                     ld_kv, ctx, lse, Tq, H, BH, Lk);
}
template <bool CAUSAL, class... A> int ca_bwd(int dh, A... a) {
  if (dh == 64) ca_launch_bwd<64, CAUSAL>(a...);
  else ca_launch_bwd<32, CAUSAL>(a...);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

}  // namespace

extern "C" {

// The causal pair hands the packed q | k | v (and dq | dk | dv) rows to the kernels as q = qkv, k | v = qkv + d with the same
// pitch and a batch stride of T rows, no klen, Lk = T.

int m3p_attn_causal_fwd(const void* qkv, int ld_qkv, void* ctx, float* lse, int B, int T, int H, int dh, uint32_t seed,
                        uint32_t thresh24, float inv_keep, void* stream) {
  if (!qkv || !ctx || !lse) return M3P_EINVAL;
  const int rc = ca_admit(B, T, H, dh, T);
  if (rc != M3P_OK) return rc;
  if ((ld_qkv % 8) != 0 || ld_qkv < 3 * H * dh || ca_misaligned(qkv) || ca_misaligned(ctx)) return M3P_ENOTIMPL;
  const bf16* q = (const bf16*)qkv;
  return ca_fwd<true>(dh, (hipStream_t)stream, q, ld_qkv, q + H * dh, (long long)T * ld_qkv, ld_qkv, (const int32_t*)nullptr,
                      (bf16*)ctx, lse, B, T, H, T, seed, thresh24, inv_keep);
}

int m3p_attn_causal_bwd(const void* qkv, int ld_qkv, const void* dctx, const float* lse, void* dqkv, int ld_dqkv, int B, int T,
                        int H, int dh, float qscale, uint32_t seed, uint32_t thresh24, float inv_keep, void* stream) {
  if (!qkv || !dctx || !lse || !dqkv) return M3P_EINVAL;
  const int rc = ca_admit(B, T, H, dh, T);
  if (rc != M3P_OK) return rc;
  if ((ld_qkv % 8) != 0 || ld_qkv < 3 * H * dh || (ld_dqkv % 8) != 0 || ld_dqkv < 3 * H * dh || ca_misaligned(qkv) ||
      ca_misaligned(dctx) || ca_misaligned(dqkv))
    return M3P_ENOTIMPL;
  const bf16* q = (const bf16*)qkv;
  bf16* dq = (bf16*)dqkv;
  return ca_bwd<true>(dh, (hipStream_t)stream, q, ld_qkv, q + H * dh, (long long)T * ld_qkv, ld_qkv, (const int32_t*)nullptr,
                      (const bf16*)dctx, lse, dq, ld_dqkv, dq + H * dh, ld_dqkv, B, T, H, T, qscale, seed, thresh24, inv_keep);
}

int m3p_attn_cross_fwd(const void* q, int ld_q, const void* kv, long long kv_bstride, int ld_kv, const int32_t* klen, void* ctx,
                       float* lse, int B, int Tq, int H, int dh, int Lk, uint32_t seed, uint32_t thresh24, float inv_keep,
                       void* stream) {
  if (!q || !kv || !ctx || !lse) return M3P_EINVAL;
  const int rc = ca_admit(B, Tq, H, dh, Lk);
  if (rc != M3P_OK) return rc;
  if (ld_q < H * dh || ld_kv < 2 * H * dh) return M3P_EINVAL;
  if ((ld_q % 8) != 0 || (ld_kv % 8) != 0 || (kv_bstride % 8) != 0 || ca_misaligned(q) || ca_misaligned(kv) || ca_misaligned(ctx))
    return M3P_ENOTIMPL;
  return ca_fwd<false>(dh, (hipStream_t)stream, (const bf16*)q, ld_q, (const bf16*)kv, kv_bstride, ld_kv, klen, (bf16*)ctx, lse, B,
                       Tq, H, Lk, seed, thresh24, inv_keep);
}

// The prefill: the queries are the last Tq of Lk = pos0 + Tq positions, and the kernel reads pos0 back as Lk - Tq.
int m3p_attn_prefix_fwd(const void* q, int ld_q, const void* kv, long long kv_bstride, int ld_kv, void* ctx, float* lse, int B,
                        int Tq, int H, int dh, int pos0, void* stream) {
  if (!q || !kv || !ctx || B <= 0 || Tq <= 0 || H <= 0 || pos0 < 0) return M3P_EINVAL;
  // (no dropout, so no bound from the stream index; pos0 is compared on its own before pos0 + Tq could overflow)
  if ((dh != 32 && dh != 64) || Tq > CA_MAX_T || pos0 > XA_MAX_KEYS || pos0 + Tq > XA_MAX_KEYS) return M3P_ENOTIMPL;
  if (ld_q < H * dh || ld_kv < 2 * H * dh) return M3P_EINVAL;
  if ((ld_q % 8) != 0 || (ld_kv % 8) != 0 || (kv_bstride % 8) != 0 || ca_misaligned(q) || ca_misaligned(kv) || ca_misaligned(ctx))
    return M3P_ENOTIMPL;
  const hipStream_t st = (hipStream_t)stream;
  if (dh == 64) ca_launch_prefix_fwd<64>(st, (const bf16*)q, ld_q, (const bf16*)kv, kv_bstride, ld_kv, (bf16*)ctx, lse, B, Tq, H, pos0 + Tq);
  else ca_launch_prefix_fwd<32>(st, (const bf16*)q, ld_q, (const bf16*)kv, kv_bstride, ld_kv, (bf16*)ctx, lse, B, Tq, H, pos0 + Tq);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

int m3p_attn_cross_bwd(const void* q, int ld_q, const void* kv, long long kv_bstride, int ld_kv, const int32_t* klen,
                       const void* dctx, const float* lse, void* dq, int ld_dq, void* dkv, int ld_dkv, int B, int Tq, int H,
                       int dh, int Lk, float qscale, uint32_t seed, uint32_t thresh24, float inv_keep, void* stream) {
  if (!q || !kv || !dctx || !lse || !dq || !dkv) return M3P_EINVAL;
  const int rc = ca_admit(B, Tq, H, dh, Lk);
  if (rc != M3P_OK) return rc;
  if (ld_q < H * dh || ld_kv < 2 * H * dh || ld_dq < H * dh || ld_dkv < 2 * H * dh) return M3P_EINVAL;
  if ((ld_q % 8) != 0 || (ld_kv % 8) != 0 || (kv_bstride % 8) != 0 || (ld_dq % 8) != 0 || (ld_dkv % 8) != 0 ||
      ca_misaligned(q) || ca_misaligned(kv) || ca_misaligned(dctx) || ca_misaligned(dq) || ca_misaligned(dkv))
    return M3P_ENOTIMPL;
  return ca_bwd<false>(dh, (hipStream_t)stream, (const bf16*)q, ld_q, (const bf16*)kv, kv_bstride, ld_kv, klen, (const bf16*)dctx,
                       lse, (bf16*)dq, ld_dq, (bf16*)dkv, ld_dkv, B, Tq, H, Lk, qscale, seed, thresh24, inv_keep);
}

}  // extern "C"
