// Tile helpers shared by the tiled decoder attentions (attn_causal.hip, attn_cross.hip): a 64-row tile of one head slice
// goes global -> registers (rows behind a bound as zeros) -> LDS, row-major with the 16-byte chunk swizzle of
// attention.hip; fragments come back as row reads (A operands) or transposing reads (ds_read_tr16_b64).
#pragma once
#include "common.hpp"

namespace {

constexpr float CA_MASKED = -1.0e30f;    // score of a masked key: exp of it minus any finite maximum is exactly 0

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

// keep factors (inv_keep or 0) of four consecutive keys of one query row
__device__ __forceinline__ void keep4(uint32_t base, uint32_t seed, uint32_t thresh24, float inv_keep, float (&f)[4]) {
  bool k4[4];
  m3p_keep_run<4>(base, seed, thresh24, k4);
#pragma unroll
  for (int r = 0; r < 4; ++r) f[r] = k4[r] ? inv_keep : 0.f;
}

}  // namespace
