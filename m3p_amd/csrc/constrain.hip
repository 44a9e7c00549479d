// Decoding constraints of the search loops (decoder.py: generate / generate_beam with min_len, repetition_penalty,
// no_repeat_ngram, banned_words): one small kernel that edits the step's bf16 logits IN PLACE, in front of the selection
// kernels of csrc/select.hip - which take a -inf logit as "never chosen, mass 0" - so that greedy selection, beam search,
// seeded sampling and nucleus sampling run unchanged behind it.  The contract is in include/m3p_hip.h (m3p_logits_constrain);
// the torch twin is decoder.constrain_scores_.
//
// At the step that decodes position cur_len, row r has the history H = generated[1:cur_len, r], L = cur_len - 1 words (the
// <EOS> at position 0 that serves as <BOS> is not part of it).  `hist` points at generated[1]: element (p, r) is
// hist[p * hist_ld + r], int64 - ROW r of the logits reads COLUMN r of the history; no host copy, no transpose.
//
// A workgroup per row, one launch per step.  The work is a few hundred history words per row - latency, not bandwidth:
//   load     the row's L words into LDS, once (int64 as they are: two words outside [0, V) that differ must not compare equal)
//   penalty  every DISTINCT word w of H with 0 <= w < V:  x[w] <- bf16_rne(fl32(x[w] * (x[w] > 0 ? inv_theta : theta))).
//            One writer per distinct word: the thread that holds the word's FIRST occurrence, found by a scan of the LDS copy
//            below its own position.  (A read-modify-write per occurrence would race, or penalise twice.)  One fp32 multiply,
//            no divide: theta and inv_theta = fl32(1 / theta) both come from the host.  0, -0 and -inf keep their bits.
//   barrier  the ban phases come behind the penalty phase: a word that is penalised and banned ends as -inf
//   n-gram   for every j in [0, L - n] whose n - 1 words H[j .. j + n - 2] equal the last n - 1 words H[L - n + 1 .. L - 1]:
//            x[H[j + n - 1]] <- -inf.  The loop stops at j = L - n: the suffix does not match itself.  n = 1 bans all of H.
//   <EOS>    x[eos] <- -inf when the caller says so (cur_len <= min_len);  banned words: x[id] <- -inf for every listed id.
// The ban phases only ever store the one value -inf, so their order among themselves and two threads that ban the same word
// do not matter.  Plain 2-byte vector stores, no atomics.  A history word or banned id outside [0, V) is skipped, so nothing is
// written outside the row's V columns: columns V .. ld - 1 and the other rows keep their bits.
#include "common.hpp"
#include <math.h>

namespace {

constexpr int LC_THREADS = 256;
constexpr int LC_MAX_HIST = 1024;      // history words per row (8 KB of LDS); generate asks once, with max_len - 1
constexpr int LC_MAX_NGRAM = 16;
constexpr int LC_MAX_BANNED = 4096;
constexpr unsigned short LC_NEG_INF = 0xFF80u;

// fp32 -> bf16 bits, round to nearest even (the rounding of torch's .to(bfloat16)); inf stays inf, NaN stays a quiet NaN
__device__ __forceinline__ unsigned short lc_bf16_rne(float f) {
  const uint32_t u = __float_as_uint(f);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (unsigned short)((u >> 16) | 0x0040u);
  return (unsigned short)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

__global__ __launch_bounds__(LC_THREADS) void lc_constrain_kernel(unsigned short* __restrict__ logits, int ld, int V,
                                                                  const long long* __restrict__ hist, long long hist_ld, int L,
                                                                  float theta, float inv_theta, int ngram, int eos,
                                                                  const long long* __restrict__ banned, int n_banned) {
  __shared__ long long h[LC_MAX_HIST];
  const int tid = threadIdx.x;
  const long long row = blockIdx.x;
  unsigned short* x = logits + (size_t)row * (size_t)ld;
  for (int p = tid; p < L; p += LC_THREADS) h[p] = hist[(size_t)p * (size_t)hist_ld + (size_t)row];
  __syncthreads();
  if (theta != 1.f || inv_theta != 1.f) {
    for (int p = tid; p < L; p += LC_THREADS) {
      const long long w = h[p];
      if (w < 0 || w >= (long long)V) continue;
      bool first = true;                                   // (no early exit: the loads of the scan stay independent)
#pragma unroll 4
      for (int q = 0; q < p; ++q) first = first && h[q] != w;
      if (!first) continue;
      const float v = __uint_as_float((uint32_t)x[w] << 16);
      x[w] = lc_bf16_rne(__fmul_rn(v, v > 0.f ? inv_theta : theta));
    }
  }
  __syncthreads();
  if (ngram >= 1 && L >= ngram) {
    const int s0 = L - ngram + 1;                          // the suffix H[s0 .. L - 1]: ngram - 1 words
    for (int j = tid; j <= L - ngram; j += LC_THREADS) {
      bool match = true;
      for (int i = 0; i < ngram - 1; ++i) match = match && h[j + i] == h[s0 + i];
      const long long w = h[j + ngram - 1];
      if (match && w >= 0 && w < (long long)V) x[w] = LC_NEG_INF;
    }
  }
  if (tid == 0 && eos >= 0) x[eos] = LC_NEG_INF;
  for (int b = tid; b < n_banned; b += LC_THREADS) {
    const long long w = banned[b];
    if (w >= 0 && w < (long long)V) x[w] = LC_NEG_INF;
  }
}

int lc_plan(int n, int V, int ld, int hist_len, int ngram, int n_banned) {
  if (n <= 0 || V <= 0 || ld < V || hist_len < 0 || ngram < 0 || n_banned < 0) return M3P_EINVAL;
  if (hist_len > LC_MAX_HIST || ngram > LC_MAX_NGRAM || n_banned > LC_MAX_BANNED) return M3P_ENOTIMPL;
  return M3P_OK;
}

}  // namespace

extern "C" {

int m3p_logits_constrain_plan(int n, int V, int ld, int hist_len, int ngram, int n_banned) {
  return lc_plan(n, V, ld, hist_len, ngram, n_banned);
}

int m3p_logits_constrain(void* logits, int ld, int n, int V, const long long* hist, long long hist_ld, int hist_len, float theta,
                         float inv_theta, int ngram, int eos_or_minus1, const long long* banned, int n_banned, void* stream) {
  const int rc = lc_plan(n, V, ld, hist_len, ngram, n_banned);
  if (rc != M3P_OK) return rc;
  if (!logits || ((uintptr_t)logits & 1) || (hist_len > 0 && (!hist || hist_ld < n || ((uintptr_t)hist & 7)))) return M3P_EINVAL;
  if (n_banned > 0 && (!banned || ((uintptr_t)banned & 7))) return M3P_EINVAL;
  if (!(theta > 0.f) || isinf(theta) || !(inv_theta > 0.f) || isinf(inv_theta)) return M3P_EINVAL;
  if (eos_or_minus1 < -1 || eos_or_minus1 >= V) return M3P_EINVAL;
  const bool penalty = (theta != 1.f || inv_theta != 1.f) && hist_len > 0;
  const bool grams = ngram >= 1 && hist_len >= ngram;
  if (!penalty && !grams && eos_or_minus1 < 0 && n_banned == 0) return M3P_OK;       // nothing to edit at this step
  hipLaunchKernelGGL(lc_constrain_kernel, dim3((unsigned)n), dim3(LC_THREADS), 0, (hipStream_t)stream, (unsigned short*)logits, ld, V,
                     hist, hist_ld, hist_len, theta, inv_theta, ngram, eos_or_minus1, banned, n_banned);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

}  // extern "C"
