"""Seeded top-k sampling over more than 16 candidates (csrc/select.hip: m3p_vocab_sample_wide; ops.vocab_sample_wide;
decoder.generate(sample_top_k=40, ...)): the part that needs no GPU - the tolerance of the nucleus cut, the device's sums
and its selection restated in NumPy against the twin, and the rule for a class of equal logits at the k-th place.

The contract (include/m3p_hip.h) is that of tests/test_vocab_nucleus.py with 1 <= top_k <= 1024: the candidate set K is the
row's first top_k words under (logit descending, word ascending) - of the class of equal logits at the k-th place the lowest
word ids, as many as still fit -, masses, C, Z and the cut x* are taken over K, and a class that is only partly inside K
counts the words that are in K.  The twin (rng.sample_allowed / nucleus_cut / nucleus_mass / sample_words) is unchanged.

A device cut c of a row is accepted by the per-row rule of tests/test_vocab_nucleus.py (_cut_accepted) with WIDE_NUCLEUS_TOL in
place of NUCLEUS_TOL.  wide_nucleus_tol(V, top_k) bounds |device C / Z - fp64 C / Z| for every set of candidates C, from the
documented accuracy of what vsw_draw_kernel calls (u = 2^-24, the unit roundoff of fp32).  The mass of a word is computed
against m' = fl(max_K x * inv_t); the reference point is common to every word of the row and cancels in C / Z.
d_w = m' - x_w * inv_t >= 0 is the word's depth.
  every word       arg = fma(x, inv_t, -m'): ONE rounding, |error| <= d_w u - a relative error d_w u of the mass;
                   expf: OCML documents 1 ulp <= 2 u relative.  Relative error of a mass: (d_w + 2) u.
  weighted         the error of a sum of masses, over Z, is at most sum_w p_w (d_w + 2) u with p = softmax over K; and
                   sum_w p_w d_w = H(p) - ln Z <= ln |K| (H the entropy, Z >= 1 against the maximum).  So (ln |K| + 2) u.
  the sums         every mass is rounded to an integer of the grid 2^-40 (vnuc_mass, the all-words route's): 2^-41 absolute
                   each, |K| 2^-41 over Z >= 1; at most 1024 integers below 2^40 (1 + 2^-20) stay below 2^51 and are added
                   EXACTLY, in any order - plain fp32 running sums would add 2 * 1023 u = 1.2e-4, which is why they are not
                   used; the comparison is (double) C >= (double) top_p * (double) Z: 3 * 2^-53, nothing.
  the ratio        |C'/Z' - C/Z| <= (|dC| + |dZ|) / Z': twice the above (and 1e-3 of it for the second order).
wide_nucleus_tol is that: 1.07e-6 at top_k = 1024 for any V, 7.2e-7 at 50.  WIDE_NUCLEUS_TOL = 2e-6 covers every shape of
tests/test_vocab_sample_wide.py, below the 1e-5 at which the twin's margins were surveyed (smallest margin of the small cases
3.3e-5; >= 99 % of the 4096-row case outside 1e-5).  The bound is proved below by a fixed-point NumPy restatement of the
kernel's sums against the twin, on the very rows of the GPU cases."""
import math

import numpy as np
import pytest
import torch

from m3p_amd import rng
from tests.test_vocab_sample import CHUNK, U32, _logits

WIDE_NUCLEUS_TOL = 2e-6
WIDE_SHIFT = 40                 # VSW_SHIFT of csrc/select.hip
WIDE_MAX_K = 1024               # VSW_MAX_K

# (V, ld, n) -> the top_k of the GPU cases
CASES = [((1000, 1024, 3), (17, 40, 64, 1000)),
         ((2 * CHUNK + 2, 8448, 5), (17, 50, 256, 1024)),
         ((250002, 250112, 2), (17, 50, 1024)),
         ((40, 40, 4096), (17, 40)),
         ((2059, 2304, 3), (17, 64, 1024))]          # a chunk's second half: one whole load, a 3-column tail, the rest past V
TEMPERATURES = (4.0, 1.0, 0.25)


def wide_nucleus_tol(V, top_k):
    assert 1 <= top_k <= min(V, WIDE_MAX_K)
    per_sum = (math.log(top_k) + 2.0) * U32 + top_k * 2.0 ** -(WIDE_SHIFT + 1)
    return 2.0 * per_sum * (1.0 + 1e-3) + 4 * 2.0 ** -53


def case_rows(V, ld, n):
    """The fp32 values of the V real columns of a GPU case (the seed of tests/test_vocab_sample.py: V + n)."""
    return _logits(n, V, ld, seed=V + n)[:, :V].float().numpy()


def test_wide_nucleus_tol_is_what_the_docstring_says():
    assert wide_nucleus_tol(250002, 1024) <= 1.07e-6 and wide_nucleus_tol(1000, 50) <= 7.2e-7
    for (V, ld, n), ks in CASES:
        for top_k in tuple(ks) + (5, 16):
            assert wide_nucleus_tol(V, top_k) <= WIDE_NUCLEUS_TOL <= 1e-5, (V, top_k)
    assert WIDE_MAX_K * 2 ** WIDE_SHIFT * (1 + 2.0 ** -20) < 2 ** 51
    assert 2 * 1023 * U32 > 1e-4                                       # the fp32 running sums that are not used


def _device_prefix_ratios(x32, inv_t, top_k):
    """vsw_draw_kernel's sums restated in NumPy, for EVERY prefix of every row's candidates in the order of the cumulated mass
    (logit descending): m' = fl32(max x * inv_t), arg = fl32(x * inv_t - m') in one rounding (the product of a bf16 and an fp32
    number is exact in fp64), the exponential rounded to fp32, rint(mass * 2^40) as integers, summed exactly.
    -> (device prefix / Z, fp64 prefix / Z), [n, top_k] each."""
    f32, f64 = np.float32, np.float64
    xs = -np.sort(-x32.astype(f64), axis=1)[:, :top_k]
    it = f64(f32(inv_t))
    m32 = (xs[:, :1] * it).astype(f32)
    arg = (xs * it - m32.astype(f64)).astype(f32)
    mass = np.exp(arg.astype(f64)).astype(f32)
    exact = np.exp(xs * it - xs[:, :1] * it)
    ref = np.cumsum(exact, axis=1) / exact.sum(1)[:, None]
    fixed = np.rint(mass.astype(f64) * 2.0 ** WIDE_SHIFT).astype(np.uint64)          # (a mass <= 1 + 2^-20: below 2^53, exact)
    cs = np.cumsum(fixed, axis=1, dtype=np.uint64)
    return cs.astype(f64) / cs[:, -1:].astype(f64), ref


@pytest.mark.parametrize('case', range(len(CASES)))
def test_wide_error_model_holds_on_the_rows_of_the_gpu_cases(case):
    (V, ld, n), ks = CASES[case]
    x32 = case_rows(V, ld, n)
    for T in TEMPERATURES:
        for top_k in ks:
            dev, ref = _device_prefix_ratios(x32, rng.inv_temperature(T), top_k)
            worst = float(np.abs(dev - ref).max())
            print('V %d n %d inv_t %.2f top_k %d: worst |C/Z - fp64| over %d prefixes %.3g; wide_nucleus_tol %.3g' % (
                V, n, 1 / T, top_k, dev.size, worst, wide_nucleus_tol(V, top_k)))
            assert worst <= wide_nucleus_tol(V, top_k) <= WIDE_NUCLEUS_TOL


def _sortable16(x32):
    """vs_sortable16 of csrc/select.hip on bf16-valued fp32 numbers (-0 folded into +0): unsigned order = order of the values."""
    b = (np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32) >> np.uint32(16)).astype(np.int64)
    b = np.where(b == 0x8000, 0, b)
    return np.where(b & 0x8000, ~b & 0xFFFF, b | 0x8000)


def _device_candidates(x32, top_k):
    """The selection of m3p_vocab_sample_wide restated in NumPy: two levels of 256 counts over the sortable key give the k-th
    value v_k and above = #{x > v_k}; of the class at v_k the quota top_k - above goes out in column order - an exclusive sum
    over the row's chunks of 4096 columns, then a prefix sum inside the chunk.  -> bool [n, V]."""
    n, V = x32.shape
    out = np.zeros((n, V), dtype=bool)
    for r in range(n):
        sk = _sortable16(x32[r])
        need, hi = top_k, None
        for level in (0, 1):
            inside = sk if level == 0 else sk[(sk >> 8) == hi]
            cnt = np.bincount((inside >> 8) if level == 0 else (inside & 0xFF), minlength=256)
            from_top = np.cumsum(cnt[::-1])[::-1]                        # words in this bin and above
            b = int(np.flatnonzero((from_top >= need) & (cnt > 0)).max())
            need -= int(from_top[b] - cnt[b])
            hi = b if level == 0 else hi
        kth, quota = hi << 8 | b, need
        assert 1 <= quota <= int((sk == kth).sum())
        rank = np.zeros(V, dtype=np.int64)
        before = 0
        for c0 in range(0, V, CHUNK):
            eq = sk[c0:c0 + CHUNK] == kth
            rank[c0:c0 + CHUNK] = before + np.cumsum(eq) - eq
            before += int(eq.sum())
        out[r] = (sk > kth) | ((sk == kth) & (rank < quota))
    return out


def test_device_selection_restated_is_the_twins_candidate_set():
    for (V, ld, n), ks in CASES[:3]:
        x32 = case_rows(V, ld, n)
        x32[0, 3], x32[0, 9] = 0.0, -0.0                                 # one value to the twin and to the kernel
        for top_k in tuple(ks) + (1, 5, 16):
            assert np.array_equal(_device_candidates(x32, top_k), rng.sample_allowed(x32, top_k)), (V, top_k)
    x32 = case_rows(40, 40, 4096)[:64]
    x32[:, 5] = -np.inf
    for top_k in (17, 40):
        assert np.array_equal(_device_candidates(x32, top_k), rng.sample_allowed(x32, top_k)), top_k


def test_twin_over_the_candidates_is_the_twin_on_their_sub_row():
    """Masses, cut and draw "over K" are the twin's on the sub-row of K's columns in word order with every column a candidate:
    the GPU tests compute K once per row and then work on [n, top_k] arrays."""
    V, ld, n = 2 * CHUNK + 2, 8448, 5
    x32 = case_rows(V, ld, n)
    seed = rng.stream_seed(V, n, 1)
    key64 = rng.sample_keys(x32, 1.0, seed)
    for top_k in (17, 256):
        cols = np.nonzero(rng.sample_allowed(x32, top_k))[1].reshape(n, top_k)
        xk = np.take_along_axis(x32, cols, 1)
        assert rng.sample_allowed(xk, top_k).all()
        for p in (0.5, 0.99):
            full, sub = rng.nucleus_cut(x32, 1.0, p, top_k), rng.nucleus_cut(xk, 1.0, p, top_k)
            assert np.array_equal(full[0], sub[0]) and np.abs(full[1] - sub[1]).max() <= 1e-15 and np.abs(full[2] - sub[2]).max() <= 1e-15
            allowed = rng.sample_allowed(x32, top_k, top_p=p, inv_t=1.0)
            assert np.array_equal(np.take_along_axis(allowed, cols, 1), xk >= sub[0][:, None]) and allowed.sum() == (xk >= sub[0][:, None]).sum()
            words = rng.sample_words(x32, 1.0, seed, top_k, top_p=p)[0]
            sub_keys = np.where(xk >= sub[0][:, None], np.take_along_axis(key64, cols, 1), -np.inf)
            assert np.array_equal(words, cols[np.arange(n), sub_keys.argmax(1)])


def test_gpu_cases_have_the_ties_the_issue_counts():
    """Uniform bf16 data put the k-th place inside a class of equal logits as a rule: at the full width the top class (16.0)
    holds 232 and 251 words, so top_k = 17 and 50 lie wholly inside it; at 1024 the quota cuts the class of 15.875."""
    x32 = case_rows(250002, 250112, 2)
    assert (x32 == 16.0).sum(1).tolist() == [232, 251]
    assert (x32 == 15.875).sum(1).tolist() == [467, 512] and (x32 > 15.875).sum(1).tolist() == [732, 776]
    chunks = [np.unique(np.flatnonzero(rng.sample_allowed(x32, 50)[r]) // CHUNK).size for r in range(2)]
    assert min(chunks) >= 2, chunks


def test_twin_on_a_hand_built_row_for_the_tie_quota():
    """inv_t = ln 2: a word of logit v weighs 2^(v - 3).  Values 3, 2, 1 with 2, 5, 9 words, the class of 2 on both sides of the
    middle of the row.  top_k = 4: both 3s and the two lowest-id 2s - masses 1, 1, 1/2, 1/2, Z = 3; C(3) / Z = 2/3, C(2) / Z = 1
    with the class of 2 counted as the TWO words inside K (all five would give Z = 9/2 and C(3) / Z = 4/9)."""
    inv_t = float(np.float32(math.log(2.0)))
    vals = [1, 3, 1, 2, 1, 1, 2, 1, 2, 1, 3, 2, 1, 1, 2, 1]
    assert [vals.count(v) for v in (3, 2, 1)] == [2, 5, 9]
    twos = [i for i, v in enumerate(vals) if v == 2]
    assert twos[1] < len(vals) // 2 <= twos[2]
    x = np.array([vals], dtype=np.float32)
    K = rng.sample_allowed(x, 4)
    assert np.flatnonzero(K[0]).tolist() == [1, 3, 6, 10] and np.array_equal(_device_candidates(x, 4), K)
    tol = 1e-6                                                        # (fl32(ln 2) is not ln 2)
    cut, inside, above = rng.nucleus_cut(x, inv_t, 0.8, top_k=4)      # 2/3 < 0.8: the cut falls on 2
    assert cut.tolist() == [2.0] and abs(inside[0] - 1.0) <= tol and abs(above[0] - 2 / 3) <= tol
    assert np.array_equal(rng.sample_allowed(x, 4, top_p=0.8, inv_t=inv_t), K)
    cut, inside, above = rng.nucleus_cut(x, inv_t, 0.6, top_k=4)      # 2/3 >= 0.6: the 3s alone
    assert cut.tolist() == [3.0] and abs(inside[0] - 2 / 3) <= tol and above[0] == 0.0
    assert np.flatnonzero(rng.sample_allowed(x, 4, top_p=0.6, inv_t=inv_t)[0]).tolist() == [1, 10]
    # the log-probability is over the allowed set: 3 of mass, a 2 weighs 1/2
    for seed in range(8):
        words, logprob, _ = rng.sample_words(x, inv_t, seed, 4, top_p=0.8)
        w = int(words[0])
        assert K[0, w] and abs(logprob[0] - ((vals[w] - 3.0) * math.log(2.0) - math.log(3.0))) <= tol
    # a wider set takes the third 2 before any 1
    assert np.flatnonzero(rng.sample_allowed(x, 5)[0]).tolist() == [1, 3, 6, 8, 10]
    assert np.array_equal(_device_candidates(x, 7), rng.sample_allowed(x, 7)) and rng.sample_allowed(x, 7)[0, twos].all()
    assert np.array_equal(_device_candidates(x, 9), rng.sample_allowed(x, 9))
    assert torch.from_numpy(x).to(torch.bfloat16).float().numpy().tolist() == x.tolist()
