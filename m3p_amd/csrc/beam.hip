// Hypothesis bookkeeping of a beam-search step on the device (decoder.py: generate_beam with BEAM_HYPS_ON_DEVICE): what the
// loop did on the host with the step's 2 * beam candidates per sentence - finished hypotheses into a bounded list, the next
// beams, the done flag - and, in the same launch, the step's re-ordering of `generated` and of the cache's owner table.  The
// contract is in include/m3p_hip.h (m3p_beam_advance); the host twin, which this kernel equals bit for bit, is
// decoder.beam_advance_host.
//
// One wave per sentence, grid = bs: the work is a walk over k <= 64 candidates whose every decision depends on the one before
// (the list changes as hypotheses arrive), so it is serial by nature and a few hundred instructions long - latency, like
// csrc/constrain.hip.  All 64 lanes walk together: the candidate, the list (LDS) and every decision are the same in every
// lane, control flow is uniform; lane 0 alone writes the list, between two barriers.  The lanes part only where there is
// width: the copy of a finished hypothesis's tokens, and the re-ordering of `generated` and the owner table at the end.
//
//   done      done[s] |= the list is full and (early_stopping or min score >= next_scores[s, 0] / norm_max)
//   frozen    a done sentence emits beam x (0.0, pad, row 0) and leaves its list alone: further steps change nothing
//   walk      candidate c = (value, flat_idx): beam = flat_idx / V, word = flat_idx % V, row = s * beam_size + beam.
//             word == eos, or the last step (cur_len + 1 == max_len): offered to the list with score = double(value) /
//             norm[cur_len] and the next arrival number - the next free slot while count < beam, else the slot that is minimal
//             by (score, arrival), and only for a strictly larger score.  Otherwise it is the next continuation; the walk ends
//             at `beam` of them.  Missing continuations are (0.0, pad, row 0); before the last step that sets status.
//   tokens    an accepted hypothesis copies generated[0 .. cur_len - 1, row] into hyp_tok[s, slot, :], lanes striding over
//             positions.  Positions from cur_len on hold pad already: hypotheses only get longer from step to step.
//   re-order  gen_out[p, r] = gen_in[p, beam_idx[r]] (p < cur_len), gen_out[cur_len, r] = word;
//             owner_out[r, :] = owner_in[beam_idx[r], :] with column cur_len = r  (decoder.advance_owner).
// gen_in / gen_out and owner_in / owner_out are different buffers: a done sentence reads row 0, which another workgroup owns
// and, in place, would be rewriting.  The normalisers come from the host as doubles (norm[l] = l ** length_penalty): the kernel
// only converts fp32 -> fp64 (exact), divides and compares in fp64 (IEEE, correctly rounded) - no pow, no fused operation.
// No atomics; plain vector stores.
#include "common.hpp"
#include <math.h>

namespace {

constexpr int BA_THREADS = 64;         // one wave
constexpr int BA_MAX_BEAM = 32;
constexpr int BA_MAX_K = 64;
constexpr int BA_MAX_LEN = 1025;

struct BeamAdvanceArgs {
  const float* next_scores;
  const long long* flat_idx;
  const double* norm;
  const long long* gen_in;
  long long* gen_out;
  const int32_t* owner_in;
  int32_t* owner_out;
  float* beam_scores;
  long long* beam_words;
  long long* beam_idx;
  long long* hyp_tok;
  int32_t* hyp_len;
  double* hyp_score;
  float* hyp_sum;
  int32_t* hyp_arrival;
  int32_t* hyp_count;
  int32_t* arrivals;
  uint8_t* done;
  int32_t* status;
  double norm_max;
  long long gen_ld;
  int owner_ld, bs, beam, k, V, cur_len, max_len, eos, pad, early_stopping;
};

__global__ __launch_bounds__(BA_THREADS) void ba_advance_kernel(const BeamAdvanceArgs a) {
  __shared__ double l_score[BA_MAX_BEAM];
  __shared__ int l_arrival[BA_MAX_BEAM];
  __shared__ float n_score[BA_MAX_BEAM];
  __shared__ long long n_word[BA_MAX_BEAM];
  __shared__ int n_row[BA_MAX_BEAM];
  const int lane = threadIdx.x;
  const int s = blockIdx.x;
  const int beam = a.beam, cur_len = a.cur_len;
  const int row0 = s * beam;                          // the sentence's first row, and its first list slot
  for (int j = lane; j < beam; j += BA_THREADS) {
    l_score[j] = a.hyp_score[row0 + j];
    l_arrival[j] = a.hyp_arrival[row0 + j];
  }
  __syncthreads();
  int count = a.hyp_count[s];
  int arrivals = a.arrivals[s];
  int status = a.status[s];
  bool done = a.done[s] != 0;
  if (!done && count >= beam) {
    double worst = l_score[0];
    for (int j = 1; j < beam; ++j) worst = l_score[j] < worst ? l_score[j] : worst;
    done = a.early_stopping != 0 || worst >= (double)a.next_scores[(size_t)s * a.k] / a.norm_max;
  }
  int found = 0;
  if (!done) {
    const bool last = cur_len + 1 == a.max_len;
    const double norm_len = a.norm[cur_len];
    for (int c = 0; c < a.k && found < beam; ++c) {
      const float value = a.next_scores[(size_t)s * a.k + c];
      const long long idx = a.flat_idx[(size_t)s * a.k + c];
      long long b = idx / a.V;
      const long long word = idx - b * a.V;
      if (idx < 0 || b >= beam) {                     // not an entry of this sentence: flagged, and read from beam 0
        status |= 2;
        b = 0;
      }
      const int row = row0 + (int)b;
      if (word == a.eos || last) {
        const double score = (double)value / norm_len;
        const int arrival = arrivals++;
        int slot = -1;
        if (count < beam) {
          slot = count++;
        } else {
          int m = 0;
          for (int j = 1; j < beam; ++j)
            if (l_score[j] < l_score[m] || (l_score[j] == l_score[m] && l_arrival[j] < l_arrival[m])) m = j;
          if (score > l_score[m]) slot = m;
        }
        if (slot >= 0) {                              // (uniform: every lane holds the same slot)
          __syncthreads();                            // every lane has read the list
          if (lane == 0) {
            l_score[slot] = score;
            l_arrival[slot] = arrival;
            a.hyp_score[row0 + slot] = score;
            a.hyp_arrival[row0 + slot] = arrival;
            a.hyp_sum[row0 + slot] = value;
            a.hyp_len[row0 + slot] = cur_len;
          }
          long long* tok = a.hyp_tok + (size_t)(row0 + slot) * (size_t)a.max_len;
          for (int p = lane; p < cur_len; p += BA_THREADS) tok[p] = a.gen_in[(size_t)p * (size_t)a.gen_ld + (size_t)row];
          __syncthreads();
        }
      } else {
        if (lane == 0) {
          n_score[found] = value;
          n_word[found] = word;
          n_row[found] = row;
        }
        ++found;
      }
    }
    if (found < beam && !last) status |= 1;
  }
  if (done) found = 0;
  for (int r = found + lane; r < beam; r += BA_THREADS) {       // missing continuations, a done sentence, the last step
    n_score[r] = 0.f;
    n_word[r] = a.pad;
    n_row[r] = 0;
  }
  __syncthreads();
  if (lane == 0) {
    a.hyp_count[s] = count;
    a.arrivals[s] = arrivals;
    a.status[s] = status;
    a.done[s] = done ? 1 : 0;
  }
  for (int r = lane; r < beam; r += BA_THREADS) {
    a.beam_scores[row0 + r] = n_score[r];
    a.beam_words[row0 + r] = n_word[r];
    a.beam_idx[row0 + r] = n_row[r];
  }
  // `generated`: consecutive lanes take the sentence's consecutive rows of one position
  for (int i = lane; i < beam * cur_len; i += BA_THREADS) {
    const int p = i / beam, r = i - p * beam;
    a.gen_out[(size_t)p * (size_t)a.gen_ld + (size_t)(row0 + r)] = a.gen_in[(size_t)p * (size_t)a.gen_ld + (size_t)n_row[r]];
  }
  for (int r = lane; r < beam; r += BA_THREADS) a.gen_out[(size_t)cur_len * (size_t)a.gen_ld + (size_t)(row0 + r)] = n_word[r];
  // the owner table: consecutive lanes take consecutive positions of one row
  for (int i = lane; i < beam * a.max_len; i += BA_THREADS) {
    const int r = i / a.max_len, p = i - r * a.max_len;
    a.owner_out[(size_t)(row0 + r) * (size_t)a.owner_ld + p] =
        p == cur_len ? row0 + r : a.owner_in[(size_t)n_row[r] * (size_t)a.owner_ld + p];
  }
}

int ba_plan(int bs, int beam, int k, int max_len) {
  if (bs <= 0 || beam <= 0 || k <= 0 || max_len < 2) return M3P_EINVAL;
  if (beam > BA_MAX_BEAM || k > BA_MAX_K || max_len > BA_MAX_LEN) return M3P_ENOTIMPL;
  if ((long long)bs * beam > 0x7FFFFFFFll / BA_MAX_LEN) return M3P_ENOTIMPL;        // 32-bit row * position products
  return M3P_OK;
}

}  // namespace

extern "C" {

int m3p_beam_advance_plan(int bs, int beam, int k, int max_len) { return ba_plan(bs, beam, k, max_len); }

int m3p_beam_advance(const float* next_scores, const long long* flat_idx, int bs, int beam, int k, int V, int cur_len, int max_len,
                     int eos, int pad, int early_stopping, const double* norm, double norm_max, const long long* gen_in,
                     long long* gen_out, long long gen_ld, const int32_t* owner_in, int32_t* owner_out, int owner_ld,
                     float* beam_scores, long long* beam_words, long long* beam_idx, long long* hyp_tok, int32_t* hyp_len,
                     double* hyp_score, float* hyp_sum, int32_t* hyp_arrival, int32_t* hyp_count, int32_t* arrivals,
                     uint8_t* done, int32_t* status, void* stream) {
  const int rc = ba_plan(bs, beam, k, max_len);
  if (rc != M3P_OK) return rc;
  if (V <= 0 || cur_len < 1 || cur_len >= max_len || gen_ld < (long long)bs * beam || owner_ld < max_len) return M3P_EINVAL;
  if (!next_scores || !flat_idx || !norm || !gen_in || !gen_out || !owner_in || !owner_out || !beam_scores || !beam_words ||
      !beam_idx || !hyp_tok || !hyp_len || !hyp_score || !hyp_sum || !hyp_arrival || !hyp_count || !arrivals || !done || !status)
    return M3P_EINVAL;
  if (gen_in == gen_out || owner_in == owner_out) return M3P_EINVAL;                 // (a done sentence reads another one's row 0)
  if (((uintptr_t)flat_idx | (uintptr_t)norm | (uintptr_t)gen_in | (uintptr_t)gen_out | (uintptr_t)beam_words |
       (uintptr_t)beam_idx | (uintptr_t)hyp_tok | (uintptr_t)hyp_score) & 7)
    return M3P_EINVAL;
  if (((uintptr_t)next_scores | (uintptr_t)owner_in | (uintptr_t)owner_out | (uintptr_t)beam_scores | (uintptr_t)hyp_len |
       (uintptr_t)hyp_sum | (uintptr_t)hyp_arrival | (uintptr_t)hyp_count | (uintptr_t)arrivals | (uintptr_t)status) & 3)
    return M3P_EINVAL;
  BeamAdvanceArgs a;
  a.next_scores = next_scores; a.flat_idx = flat_idx; a.norm = norm; a.gen_in = gen_in; a.gen_out = gen_out;
  a.owner_in = owner_in; a.owner_out = owner_out; a.beam_scores = beam_scores; a.beam_words = beam_words; a.beam_idx = beam_idx;
  a.hyp_tok = hyp_tok; a.hyp_len = hyp_len; a.hyp_score = hyp_score; a.hyp_sum = hyp_sum; a.hyp_arrival = hyp_arrival;
  a.hyp_count = hyp_count; a.arrivals = arrivals; a.done = done; a.status = status; a.norm_max = norm_max; a.gen_ld = gen_ld;
  a.owner_ld = owner_ld; a.bs = bs; a.beam = beam; a.k = k; a.V = V; a.cur_len = cur_len; a.max_len = max_len; a.eos = eos;
  a.pad = pad; a.early_stopping = early_stopping;
  hipLaunchKernelGGL(ba_advance_kernel, dim3((unsigned)bs), dim3(BA_THREADS), 0, (hipStream_t)stream, a);
  M3P_CHECK_LAUNCH();
  return M3P_OK;
}

}  // extern "C"
