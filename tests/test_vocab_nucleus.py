"""Nucleus (top-p) sampling of the seeded decoding loop (csrc/select.hip: m3p_vocab_nucleus_sample; m3p_amd/rng.py:
nucleus_cut / nucleus_mass / sample_allowed(top_p=...) / sample_words(top_p=...); decoder.generate(sample_top_p=...)).

The contract (include/m3p_hip.h): over the candidate set K of a row (top_k = 0: every word; otherwise the row's first top_k
words under (logit descending, word ascending)), with y = float(logit) * inv_t and m = max_K y:  mass(v) = #{w in K : x_w == v}
* exp(v * inv_t - m) for each distinct logit value v,  C(v) = the sum of mass(v') over v' >= v,  C_above(v) the same over
v' > v,  Z = C(-inf);  the cut x* = max{v : C(v) >= top_p * Z};  the allowed set A = {w in K : x_w >= x*} - whole classes of
equal logits.  The draw, logprob and key are those of tests/test_vocab_sample.py with A as the allowed set.

The device sums where the twin (fp64) is exact, so a row whose cumulated mass lands on top_p to within rounding may cut one
class earlier or later.  No row is excluded: a device cut c of a row is accepted iff (1) c is a logit value present in the
row's candidate set, (2) C(c) / Z >= top_p - NUCLEUS_TOL and (3) C_above(c) / Z < top_p + NUCLEUS_TOL, with the fp64 sums of
the twin - so a row whose twin margin min(C(x*) / Z - top_p, top_p - C_above(x*) / Z) exceeds NUCLEUS_TOL admits exactly the
twin's cut.  The draw is then held to (a) - (d) of tests/test_vocab_sample.py with the allowed set = candidates with x >= c.

NUCLEUS_TOL bounds |device C / Z - fp64 C / Z| for every set of words C, from the documented accuracy of what the kernels
call (u = 2^-24, the unit roundoff of fp32).  The mass of a word is computed against m' = fl(max x * inv_t); the reference
point is common to every word of the row and cancels in C / Z.  d_w = m' - x_w * inv_t >= 0 is the word's depth.
  every word       arg = fma(x, inv_t, -m'): ONE rounding, |error| <= d_w u - a relative error d_w u of the mass;
                   expf: OCML documents 1 ulp <= 2 u relative.  Relative error of a mass: (d_w + 2) u.
  weighted         the error of a sum of masses, over Z, is at most sum_w p_w (d_w + 2) u with p = softmax over K; and
                   sum_w p_w d_w = H(p) - ln Z <= ln |K| (H the entropy, Z >= 1 against the maximum).  So (ln |K| + 2) u.
  top_k = 0        the mass is rounded to the integer grid 2^-s, s = min(40, 63 - bits(V)): V 2^-(s+1) over Z >= 1; the
                   integer sums (LDS and global atomics, two levels of 256 bins) are exact, in any order; the scan compares
                   (double) C >= (double) top_p * (double) Z: 3 * 2^-53, nothing.
  1 <= top_k <= 16 the masses are added in fp32 in lane order: at most 15 further roundings, 15 u relative.
  the ratio        |C'/Z' - C/Z| <= (|dC| + |dZ|) / Z': twice the above (and 1e-3 of it for the second order).
nucleus_tol(V, top_k) is that; at V = 250 002 it is 2.0e-6 for top_k = 0 and at top_k = 16 it is 2.4e-6 for any V.
NUCLEUS_TOL = 4e-6 covers every shape here, far inside the 1e-4 the per-row check needs to keep its sight: the tests assert
from the twin alone, before they look at a device result, that every row of the small cases and >= 98 % of the 4096-row
case (>= 95 % at top_p = 0.99) have a margin above it.  The bound is proved on the CPU by an fp32 / fixed-point NumPy
restatement of the kernels' sums against the twin."""
import math

import numpy as np
import pytest
import torch

from m3p_amd import rng, synth
from tests.test_vocab_sample import (CHUNK, KEY_ATOL, U32, _check_rows, _chi2, _chi2_quantile, _dist_rows, _hip_model, _logits,
                                     _oracle_backed, _unfinished_before, lse_bar)
from tests.util import assert_bits_equal, poisoned_outputs

BF16 = torch.bfloat16
NUCLEUS_TOL = 4e-6


def _shift(V):
    """The fixed-point grid of the all-words route (vnuc_layout of csrc/select.hip): masses are integers of 2^-shift."""
    return min(40, 63 - int(V).bit_length())


def nucleus_tol(V, top_k):
    cand = top_k if top_k else V
    per_sum = (math.log(cand) + 2.0) * U32 + (15 * U32 if top_k else V * 2.0 ** -(_shift(V) + 1))
    return 2.0 * per_sum * (1.0 + 1e-3) + 4 * 2.0 ** -53


def test_nucleus_tol_is_what_the_docstring_says():
    assert nucleus_tol(250002, 0) <= 2.0e-6 and nucleus_tol(250002, 16) <= 2.4e-6 and nucleus_tol(40, 5) <= 2.4e-6
    for V in (40, 1000, 2059, 2 * CHUNK + 2, 250002):
        for top_k in (0, 5, 16):
            assert nucleus_tol(V, top_k) <= NUCLEUS_TOL <= 1e-4
    assert _shift(250002) == 40 and _shift(2 ** 24) == 38 and (2 ** 24) * 2 ** _shift(2 ** 24) < 2 ** 63


def _margin(inside, above, p):
    return np.minimum(inside - p, p - above)


def _cut_accepted(x32, inv_t, p, top_k, cut, tol=NUCLEUS_TOL):
    """The per-row rule -> (accepted bool [n], C(c) / Z, C_above(c) / Z)."""
    cand = rng.sample_allowed(x32, top_k)
    present = (cand & (x32 == np.asarray(cut, np.float32)[:, None])).any(1)
    inside, above = rng.nucleus_mass(x32, inv_t, cut, top_k)
    return present & (inside >= p - tol) & (above < p + tol), inside, above


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_twin_on_a_hand_built_row():
    """inv_t = ln 2: a word of logit v weighs 2^(v - 3).  Values 3, 2, 1, 0, -1 with 1, 2, 4, 3, 8 words: class masses 1, 1, 1,
    3/8, 1/2, Z = 31/8;  C / Z = 8/31, 16/31, 24/31, 27/31, 1.  top_p = 0.8 cuts at 0 - a class of three tied words, all in."""
    inv_t = float(np.float32(math.log(2.0)))
    vals = [-1, 1, 0, -1, 2, 1, -1, 3, -1, 0, 1, -1, 2, -1, 0, 1, -1, -1]
    x = np.array([vals, vals[::-1]], dtype=np.float32)
    assert [vals.count(v) for v in (3, 2, 1, 0, -1)] == [1, 2, 4, 3, 8]
    tol = 1e-6                                                        # (fl32(ln 2) is not ln 2: 4 * 0.7 * 3e-8)
    for p, cut, inside, above, size in ((0.8, 0.0, 27 / 31, 24 / 31, 10), (0.5, 2.0, 16 / 31, 8 / 31, 3), (0.2, 3.0, 8 / 31, 0.0, 1),
                                        (0.78, 0.0, 27 / 31, 24 / 31, 10), (0.77, 1.0, 24 / 31, 16 / 31, 7), (0.9, -1.0, 1.0, 27 / 31, 18)):
        c, i, a = rng.nucleus_cut(x, inv_t, p)
        assert c.dtype == i.dtype == a.dtype == np.float64
        assert c.tolist() == [cut, cut] and np.abs(i - inside).max() <= tol and np.abs(a - above).max() <= tol, p
        allowed = rng.sample_allowed(x, 0, top_p=p, inv_t=inv_t)
        assert np.array_equal(allowed, x >= cut) and allowed.sum(1).tolist() == [size, size], p
        i2, a2 = rng.nucleus_mass(x, inv_t, c)
        assert np.array_equal(i2, i) and np.array_equal(a2, a)
    # the log-probability is taken over the cut set: top_p = 0.8 leaves 27/8 of mass, a word of logit v weighs 2^(v - 3)
    for seed in range(8):
        words, logprob, key = rng.sample_words(x, inv_t, seed, top_p=0.8)
        keys = rng.sample_keys(x, inv_t, seed)
        for r in range(2):
            w = int(words[r])
            assert x[r, w] >= 0.0 and w == int(np.where(x[r] >= 0.0, keys[r], -np.inf).argmax()) and key[r] == keys[r, w]
            assert abs(logprob[r] - ((float(x[r, w]) - 3.0) * math.log(2.0) - math.log(27 / 8))) <= tol
    # with top_k the masses are over the candidates alone: the first four words by (logit, word) weigh 1, 1/2, 1/2, 1/4
    c, i, a = rng.nucleus_cut(x, inv_t, 0.8, top_k=4)
    assert c.tolist() == [2.0, 2.0] and np.abs(i - 8 / 9).max() <= tol and np.abs(a - 4 / 9).max() <= tol
    assert rng.sample_allowed(x, 4, top_p=0.8, inv_t=inv_t).sum(1).tolist() == [3, 3]
    c, i, a = rng.nucleus_cut(x, inv_t, 0.9, top_k=4)                 # the class of 1 holds four words, ONE of them a candidate
    assert c.tolist() == [1.0, 1.0] and np.abs(a - 8 / 9).max() <= tol and rng.sample_allowed(x, 4, top_p=0.9, inv_t=inv_t).sum(1).tolist() == [4, 4]
    # a -inf logit has mass 0 and is never inside before a finite one
    y = x.copy()
    y[:, 7 if vals[7] == 3 else 0] = -np.inf
    assert vals[7] == 3 and not rng.sample_allowed(y, 0, top_p=0.999, inv_t=inv_t)[0, 7]
    # off: None and >= 1.0 are today's arrays, exactly
    for top_k in (0, 4):
        base = rng.sample_allowed(x, top_k)
        for off in (None, 1.0, 1.5):
            assert np.array_equal(rng.sample_allowed(x, top_k, top_p=off, inv_t=inv_t), base)
            for u, v in zip(rng.sample_words(x, inv_t, 3, top_k), rng.sample_words(x, inv_t, 3, top_k, top_p=off)):
                assert u.dtype == v.dtype and np.array_equal(u, v)
    assert rng.nucleus_top_p(None) is None and rng.nucleus_top_p(1.0) is None and rng.nucleus_top_p(0.9) == float(np.float32(0.9))
    for bad in (0.0, -0.5, float('nan')):
        with pytest.raises(ValueError):
            rng.nucleus_top_p(bad)


@pytest.fixture(scope='module')
def err_model_rows():
    g = torch.Generator().manual_seed(512)
    return ((torch.rand((512, 1000), generator=g) * 2 - 1) * 16).to(BF16).float().numpy()


def _device_prefix_ratios(x32, inv_t, top_k):
    """The kernels' sums restated in NumPy, for EVERY prefix of every row's candidates in the order of the cumulated mass
    (logit descending): m' = fl32(max x * inv_t), arg = fl32(x * inv_t - m') in one rounding (the product of a bf16 and an fp32
    number is exact in fp64), the exponential rounded to fp32;  top_k = 0: rint(mass * 2^shift) as integers, summed exactly;
    top_k >= 1: fp32 sums in lane order.  -> (device prefix / Z, fp64 prefix / Z), [n, candidates] each."""
    f32, f64 = np.float32, np.float64
    n, V = x32.shape
    xs = -np.sort(-x32.astype(f64), axis=1)
    if top_k:
        xs = xs[:, :top_k]
    it = f64(f32(inv_t))
    m32 = (xs[:, :1] * it).astype(f32)
    arg = (xs * it - m32.astype(f64)).astype(f32)
    mass = np.exp(arg.astype(f64)).astype(f32)
    exact = np.exp(xs * it - xs[:, :1] * it)
    ref = np.cumsum(exact, axis=1) / exact.sum(1)[:, None]
    if top_k:
        cs = np.cumsum(mass, axis=1, dtype=f32)
        assert cs.dtype == f32
        return cs.astype(f64) / cs[:, -1:].astype(f64), ref
    fixed = np.rint(mass.astype(f64) * 2.0 ** _shift(V)).astype(np.uint64)           # (a mass <= 1 + 2^-20: below 2^53, exact)
    cs = np.cumsum(fixed, axis=1, dtype=np.uint64)
    return cs.astype(f64) / cs[:, -1:].astype(f64), ref


@pytest.mark.parametrize('inv_t', [0.25, 1.0, 4.0])
def test_nucleus_error_model_holds_for_the_fp32_restatement(err_model_rows, inv_t):
    x32 = err_model_rows
    for top_k in (0, 16, 5):
        dev, ref = _device_prefix_ratios(x32, inv_t, top_k)
        worst = float(np.abs(dev - ref).max())
        print('inv_t %.2f top_k %d: worst |C/Z - fp64| over %d prefixes %.3g; nucleus_tol %.3g, NUCLEUS_TOL %.3g' % (
            inv_t, top_k, dev.size, worst, nucleus_tol(x32.shape[1], top_k), NUCLEUS_TOL))
        assert worst <= nucleus_tol(x32.shape[1], top_k) <= NUCLEUS_TOL


def test_per_row_rule_sees_a_dropped_tie_class_a_looser_rule_passes(err_model_rows):
    """The fault: the class of equal logits at the cut is left out (a kernel that stops at C_above).  The sets differ by a
    sliver of mass, so a looser rule - the drawn words agree with the twin's in 98 % of the rows, the set's mass is within
    3e-2 of top_p - passes; the per-row rule fails practically every row."""
    x32, inv_t, p = err_model_rows, 1.0, 0.9
    cut, inside, above = rng.nucleus_cut(x32, inv_t, p)
    ok, _, _ = _cut_accepted(x32, inv_t, p, 0, cut)
    assert ok.all() and (_margin(inside, above, p) > NUCLEUS_TOL).all()
    higher = np.where(x32 > cut.astype(np.float32)[:, None], x32, np.inf).min(1)      # the next class up: the fault's cut
    assert np.isfinite(higher).all()
    bad_ok, bad_inside, _ = _cut_accepted(x32, inv_t, p, 0, higher)
    keys = rng.sample_keys(x32, inv_t, 77)
    good = np.where(x32 >= cut.astype(np.float32)[:, None], keys, -np.inf).argmax(1)
    bad = np.where(x32 >= higher[:, None], keys, -np.inf).argmax(1)
    agree = float((good == bad).mean())
    print('fault: words agree in %.2f %% of rows, the faulty set holds %.4f .. %.4f of the mass; the per-row rule accepts %d of %d rows'
          % (100 * agree, bad_inside.min(), bad_inside.max(), bad_ok.sum(), len(bad_ok)))
    assert agree >= 0.98 and np.abs(bad_inside - p).max() <= 3e-2                      # the loose rule passes
    assert bad_ok.mean() <= 0.01                                                       # the per-row rule does not


def test_nucleus_generate_on_the_oracle_step(monkeypatch):
    from m3p_amd import decoder
    c, P, sd, src_enc, src_len, x, lengths = synth.decoder_case('multi')
    record = []
    stub = _oracle_backed(monkeypatch, c, sd, record)
    bs, max_len = c['bs'], c['max_len']
    run = lambda **kw: decoder.generate(stub, src_enc, src_len, c['tgt_lang_id'], max_len=max_len, **kw)   # noqa: E731
    state = torch.random.get_rng_state()
    for T, top_k, p in ((1.0, None, 0.9), (0.8, None, 0.5), (0.8, 4, 0.7)):
        inv_t = rng.inv_temperature(T)
        del record[:]
        gen, ln, lp = run(sample_seed=5, sample_temperature=T, sample_top_k=top_k, sample_top_p=p, return_logprobs=True)
        assert lp.dtype == torch.float32 and lp.shape == gen.shape and len(record) == gen.shape[0] - 1
        open_ = _unfinished_before(gen)
        smaller = 0
        for pos in range(1, gen.shape[0]):
            s = record[pos - 1].numpy()
            seed = rng.stream_seed(5, pos, decoder.SAMPLE_SITE)
            allowed = rng.sample_allowed(s, top_k or 0, top_p=p, inv_t=inv_t)
            smaller += int((allowed.sum(1) < (top_k or s.shape[1])).sum())
            words, logprob, _ = rng.sample_words(s, inv_t, seed, top_k or 0, top_p=p)
            y = np.where(allowed, s.astype(np.float64) * inv_t, -np.inf)
            lse = np.log(np.exp(y - y.max(1)[:, None]).sum(1)) + y.max(1)
            for b in range(bs):
                forced = pos == max_len - 1 and gen[pos, b] == synth.EOS and float(lp[pos, b]) == 0.0
                if open_[pos, b] and not forced:
                    w = int(gen[pos, b])
                    assert allowed[b, w] and w == int(words[b]), (pos, b)              # only inside the twin's set
                    assert abs(float(lp[pos, b]) - (y[b, w] - lse[b])) <= 1e-5, (pos, b)
                else:
                    assert float(lp[pos, b]) == 0.0, (pos, b)
        assert smaller > 0, 'the cut never removed a word: the case shows nothing'
        again = run(sample_seed=5, sample_temperature=T, sample_top_k=top_k, sample_top_p=p, return_logprobs=True)
        assert torch.equal(again[0], gen) and torch.equal(again[1], ln) and torch.equal(again[2], lp)          # replayable
    assert torch.equal(torch.random.get_rng_state(), state), 'the seeded path consumed torch\'s generator'
    # off is today's run, bit for bit; a vanishing top_p is greedy where the maximum is unique
    base = run(sample_seed=5, sample_temperature=0.8, return_logprobs=True)
    for off in (None, 1.0, 2.0):
        got = run(sample_seed=5, sample_temperature=0.8, sample_top_p=off, return_logprobs=True)
        assert all(torch.equal(u, v) for u, v in zip(base, got)), off
    del record[:]
    greedy = run()
    assert all(int((s == s.max(1, keepdim=True)[0]).sum()) == bs for s in record)
    tiny = run(sample_seed=9, sample_temperature=1.5, sample_top_p=1e-6)
    assert torch.equal(tiny[0], greedy[0]) and torch.equal(tiny[1], greedy[1])
    # the modes that need a seed, and the values that are no probability mass
    with pytest.raises(ValueError):
        run(sample_top_p=0.9)
    with pytest.raises(ValueError):
        run(sample_temperature=0.7, sample_top_p=0.9)
    for bad in (0.0, -0.1, float('nan')):
        with pytest.raises(ValueError):
            run(sample_seed=5, sample_top_p=bad)


# ------------------------------------------------------------------------------------------------------------------ GPU
def _run(dev, V, T, seed, top_p, top_k):
    from m3p_amd import ops
    n = dev.shape[0]
    with poisoned_outputs():
        res = ops.vocab_nucleus_sample(dev, V, T, seed, top_p, top_k)
    assert res is not None
    torch.cuda.synchronize()
    words, logprob, key, cut = res
    assert words.shape == logprob.shape == key.shape == cut.shape == (n,)
    assert words.dtype == torch.int64 and logprob.dtype == key.dtype == cut.dtype == torch.float32
    return res


def _hold_to_twin(full, dev, V, T, seed, top_p, top_k, key64, what, min_outside=None):
    """One launch against the twin: the vacuity condition from the twin alone, then the cut rule and (a) - (d) for every row.
    -> (the four outputs, the twin's cut, which rows have a margin above NUCLEUS_TOL)."""
    x32 = full[:, :V].float().numpy()
    n = x32.shape[0]
    inv_t = rng.inv_temperature(T)
    p = float(np.float32(top_p))
    cut_t, inside_t, above_t = rng.nucleus_cut(x32, inv_t, p, top_k)
    clear = _margin(inside_t, above_t, p) > NUCLEUS_TOL
    if min_outside is None:
        min_outside = 1.0 if n <= 5 else 0.98
    assert clear.mean() >= min_outside, (what, float(clear.mean()), float(_margin(inside_t, above_t, p).min()))
    got = _run(dev, V, T, seed, top_p, top_k)
    words, logprob, key, cut = (t.cpu().numpy() for t in got)
    ok, inside, above = _cut_accepted(x32, inv_t, p, top_k, cut)
    bad = np.flatnonzero(~ok)
    assert ok.all(), (what, 'rows', bad[:5], 'cut', cut[bad[:5]], 'twin', cut_t[bad[:5]], inside[bad[:5]], above[bad[:5]])
    assert np.array_equal(cut[clear].astype(np.float64), cut_t[clear]), what
    allowed = rng.sample_allowed(x32, top_k) & (x32 >= cut[:, None])
    a = float(np.abs(x32[np.isfinite(x32)]).max()) * inv_t
    atol = KEY_ATOL(a)
    assert ((words >= 0) & (words < V)).all(), what                                          # (c)
    err, short = _check_rows(key, words, key64, allowed, atol)                               # (c): inside the set
    assert err <= atol, (what, err, atol)                                                    # (a)
    assert short <= 2 * atol, (what, short, atol)                                            # (b)
    rows = np.arange(n)
    y = np.where(allowed, x32.astype(np.float64) * inv_t, -np.inf)
    mx = y.max(1)
    lp64 = y[rows, words] - (mx + np.log(np.exp(y - mx[:, None]).sum(1)))
    lerr = float(np.nan_to_num(np.abs(logprob.astype(np.float64) - lp64), nan=np.inf).max())
    assert lerr <= lse_bar(a), (what, lerr, lse_bar(a))                                      # (d)
    return got, cut_t, clear


@pytest.mark.gpu
@pytest.mark.parametrize('V,ld,n', [
    (1000, 1024, 3),                                # one partial chunk
    (2 * CHUNK + 2, 8448, 5),                       # whole chunks plus two columns
    (1000, 1024, 1),                                # a single row
    (250002, 250112, 2),                            # the full width
    (40, 40, 4096),                                 # many rows, tiny V
    (2059, 2304, 3),                                # a chunk's second half: one whole load, a 3-column tail, the rest past V
])
def test_vocab_nucleus_against_the_twin(V, ld, n):
    full = _logits(n, V, ld, seed=V + n)
    dev = full.cuda()
    x32 = full[:, :V].float().numpy()
    seed, other = rng.stream_seed(V, n, 1), rng.stream_seed(V, n, 2)
    sizes = []
    for T in (4.0, 1.0, 0.25):                      # inv_t 0.25, 1, 4
        key64 = rng.sample_keys(x32, rng.inv_temperature(T), seed)
        for top_k in (0, 5, 16):
            if top_k > V:
                continue
            for top_p in (0.5, 0.9):
                what = 'V %d n %d inv_t %.2f top_k %d top_p %.2f' % (V, n, 1 / T, top_k, top_p)
                got, cut_t, clear = _hold_to_twin(full, dev, V, T, seed, top_p, top_k, key64, what)
                again = _run(dev, V, T, seed, top_p, top_k)
                for g, h, name in zip(got, again, ('words', 'logprob', 'key', 'cut')):
                    assert_bits_equal(g, h, what + ': a second launch, ' + name)
                diff = _run(dev, V, T, other, top_p, top_k)
                assert_bits_equal(diff[3], got[3], what + ': another seed, the cut')
                assert not torch.equal(diff[2], got[2]), what + ': another seed, the same keys'
                sizes.append(float((x32 >= got[3].cpu().numpy()[:, None]).sum(1).mean()))
    print('V %d ld %d n %d: mean words at or above the cut per launch %s' % (V, ld, n, ' '.join('%.1f' % s for s in sizes)))


@pytest.mark.gpu
def test_vocab_nucleus_flat_rows_at_top_p_099():
    """top_p = 0.99 is ill-conditioned on flat rows; it is held at the 4096 tiny rows with T in {1, 0.25}, where at most
    2.2 % of the rows lie within 1e-4 of the cut: >= 95 % outside NUCLEUS_TOL."""
    V, ld, n = 40, 40, 4096
    full = _logits(n, V, ld, seed=V + n)
    dev = full.cuda()
    x32 = full[:, :V].float().numpy()
    seed = rng.stream_seed(V, n, 1)
    for T in (1.0, 0.25):
        key64 = rng.sample_keys(x32, rng.inv_temperature(T), seed)
        for top_k in (0, 5, 16):
            _hold_to_twin(full, dev, V, T, seed, 0.99, top_k, key64, 'top_p 0.99 inv_t %.2f top_k %d' % (1 / T, top_k), min_outside=0.95)


@pytest.mark.gpu
def test_vocab_nucleus_off_and_vanishing_top_p():
    from m3p_amd import ops
    V, ld, n = 2 * CHUNK + 2, 8448, 5
    full = _logits(n, V, ld, seed=23)
    for r, col in enumerate((0, CHUNK - 1, CHUNK, 2 * CHUNK + 1, 777)):
        full[r, col] = 17.0 + r                     # a unique maximum per row
    dev = full.cuda()
    seed = rng.stream_seed(23, 0, 5)
    for T in (1.0, 0.5):
        for top_k in (0, 5):
            base = ops.vocab_sample(dev, V, T, seed, top_k)
            for off in (None, 1.0, 1.25):
                with poisoned_outputs():
                    got = ops.vocab_nucleus_sample(dev, V, T, seed, off, top_k)
                for g, h, name in zip(got, base, ('words', 'logprob', 'key')):
                    assert_bits_equal(g, h, 'top_p %r top_k %d: %s' % (off, top_k, name))
                assert (got[3] == float('-inf')).all()
            greedy = ops.vocab_select(dev, V, None, 1, 1)[1].squeeze(1)
            words, logprob, _, cut = _run(dev, V, T, seed, 1e-6, top_k)
            assert torch.equal(words, greedy) and words.tolist() == [0, CHUNK - 1, CHUNK, 2 * CHUNK + 1, 777]
            assert cut.tolist() == [17.0, 18.0, 19.0, 20.0, 21.0] and float(logprob.abs().max()) <= 1e-6
    for bad in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError):
            ops.vocab_nucleus_sample(dev, V, 1.0, seed, bad)


@pytest.mark.gpu
def test_vocab_nucleus_planted_cases():
    from m3p_amd import ops
    V, ld, n = 2 * CHUNK + 2, 8448, 5
    full = _logits(n, V, ld, seed=11, amp=1.0)       # |x| <= 1: 8192 words of at most e^-11 against a planted 12.0
    T, p = 1.0, 0.9
    full[0, 100] = 12.25                             # row 0: the cut class split over two chunks, columns 7 and 4096 + 9
    full[0, 7] = full[0, CHUNK + 9] = 12.0
    full[1, 50] = 12.25                              # row 1: the cut class in the two-column last chunk
    full[1, 2 * CHUNK] = full[1, 2 * CHUNK + 1] = 12.0
    full[2, 3000] = 20.0                             # row 2: the top word alone exceeds top_p
    order = np.argsort(-full[3, :V].float().numpy(), kind='stable')
    full[3, torch.from_numpy(order[:3].copy())] = float('-inf')       # row 3: -inf where the largest logits were, and in the last column
    full[3, V - 1] = float('-inf')
    dev = full.cuda()
    x32 = full[:, :V].float().numpy()
    cut_t, _, _ = rng.nucleus_cut(x32, 1.0, p)
    assert cut_t[:3].tolist() == [12.0, 12.0, 20.0] and np.isfinite(cut_t).all()
    sets = [set(np.flatnonzero(x32[r] >= cut_t[r]).tolist()) for r in range(3)]
    assert sets == [{100, 7, CHUNK + 9}, {50, 2 * CHUNK, 2 * CHUNK + 1}, {3000}]
    seen = [set(), set()]
    for s in range(16):
        seed = rng.stream_seed(s, 1, 7)
        got, _, clear = _hold_to_twin(full, dev, V, T, seed, p, 0, rng.sample_keys(x32, 1.0, seed), 'planted, seed %d' % s)
        assert clear.all() and got[3].tolist()[:3] == [12.0, 12.0, 20.0]
        words = got[0].tolist()
        assert words[0] in sets[0] and words[1] in sets[1] and words[2] == 3000, words
        assert abs(float(got[1][2])) <= 1e-6 and all(math.isfinite(float(v)) for t in got[1:] for v in t)
        seen[0].add(words[0])
        seen[1].add(words[1])
    assert seen[0] >= {7, CHUNK + 9} and seen[1] >= {2 * CHUNK, 2 * CHUNK + 1}, seen
    seed = rng.stream_seed(3, 1, 7)
    key64 = rng.sample_keys(x32, 1.0, seed)
    for top_k in (2, 3, 16):                         # top_k = 2 cuts inside the class of 12.0: ONE of its words is a candidate
        got, _, _ = _hold_to_twin(full, dev, V, T, seed, p, top_k, key64, 'planted, top_k %d' % top_k)
        assert got[0][2] == 3000 and got[3].tolist()[:3] == [12.0, 12.0, 20.0]
        assert top_k > 2 or (got[0][0] in (100, 7) and got[0][1] in (50, 2 * CHUNK))
    # more than VS_MAX_K words: declined, and the plan says so
    assert ops.vocab_nucleus_sample(dev, V, T, seed, p, top_k=17) is None
    assert not ops.vocab_nucleus_takes(n, V, ld, 17) and ops.vocab_nucleus_takes(n, V, ld, 16) and ops.vocab_nucleus_takes(n, V, ld, 0)


@pytest.mark.gpu
def test_vocab_nucleus_distribution_on_the_device():
    """65 536 draws from one 40-word row at top_p = 0.9: Pearson's chi-square against the renormalised twin set at the
    1 - 1e-6 quantile, and no draw outside the set."""
    x16 = _dist_rows()
    x32 = x16.float().numpy()
    n, V = x32.shape
    p = float(np.float32(0.9))
    cut_t, inside, above = rng.nucleus_cut(x32[:1], 1.0, p)
    assert _margin(inside, above, p)[0] > NUCLEUS_TOL
    inset = x32[0] >= cut_t[0]
    seed = rng.stream_seed(1, 5, 0)
    words, _, _, cut = _run(x16.cuda(), V, 1.0, seed, 0.9, 0)
    assert (cut == float(cut_t[0])).all()
    counts = np.bincount(words.cpu().numpy(), minlength=V)
    assert counts[~inset].sum() == 0 and 1 < inset.sum() < V
    e = np.where(inset, np.exp(x32[0].astype(np.float64) - x32[0].max()), 0.0)
    stat, dof = _chi2(counts, e / e.sum())
    print('device, top_p 0.9: %d of %d words in the set, chi-square %.1f at %d degrees of freedom (bar %.1f)' % (
        inset.sum(), V, stat, dof, _chi2_quantile(dof)))
    assert dof >= 5 and stat <= _chi2_quantile(dof)


@pytest.mark.gpu
def test_nucleus_generate_end_to_end(monkeypatch):
    from m3p_amd import decoder
    m, c, src_enc, src_len = _hip_model('multi')
    bs, max_len, T, p = c['bs'], c['max_len'], 0.8, 0.9
    inv_t, p32 = rng.inv_temperature(T), float(np.float32(p))
    record = []
    real = decoder.word_logits16

    def recording(model, tensor):
        logits, V = real(model, tensor)
        record.append((logits.clone(), V))
        return logits, V

    monkeypatch.setattr(decoder, 'word_logits16', recording)

    def run(**kw):
        del record[:]
        with torch.no_grad():
            return m.generate(src_enc, src_len, c['tgt_lang_id'], max_len=max_len, sample_temperature=T, sample_seed=5,
                              return_logprobs=True, **kw)

    def check(gen, lp, top_k):
        """Every step and open row against the recorded logits -> the first step at which some row lies inside a band (the
        twin's margin within NUCLEUS_TOL, or its two best keys within 2 KEY_ATOL), None if there is none."""
        gen_h, open_, lp = gen.cpu().numpy(), _unfinished_before(gen.cpu()), lp.cpu()
        first_close, cut_some = None, 0
        for pos in range(1, gen_h.shape[0]):
            logits, V = record[pos - 1]
            x32 = logits[:, :V].float().cpu().numpy()
            a = float(np.abs(x32).max()) * inv_t
            key64 = rng.sample_keys(x32, inv_t, rng.stream_seed(5, pos, decoder.SAMPLE_SITE))
            cut_t, inside, above = rng.nucleus_cut(x32, inv_t, p32, top_k)
            allowed = rng.sample_allowed(x32, top_k) & (x32 >= cut_t.astype(np.float32)[:, None])
            cut_some += int((allowed.sum(1) < (top_k or V)).sum())
            best = np.sort(np.where(allowed, key64, -np.inf), axis=1)[:, -2:]
            y = np.where(allowed, x32.astype(np.float64) * inv_t, -np.inf)
            lse = np.log(np.exp(y - y.max(1)[:, None]).sum(1)) + y.max(1)
            for b in range(bs):
                forced = pos == max_len - 1 and gen_h[pos, b] == synth.EOS and float(lp[pos, b]) == 0.0
                if not open_[pos, b] or forced:
                    assert float(lp[pos, b]) == 0.0, (pos, b)
                    continue
                close = _margin(inside, above, p32)[b] <= NUCLEUS_TOL or best[b, 1] - best[b, 0] < 2 * KEY_ATOL(a)
                if close:
                    first_close = pos if first_close is None else first_close
                    continue
                w = int(gen_h[pos, b])
                assert w == int(np.where(allowed[b], key64[b], -np.inf).argmax()), (pos, b, w)     # the twin's word
                assert abs(float(lp[pos, b]) - (y[b, w] - lse[b])) <= lse_bar(a), (pos, b)
        assert cut_some > 0, 'the cut never removed a word: the case shows nothing'
        return first_close

    cuda_state = torch.cuda.get_rng_state()
    for top_k in (0, 4):
        kw = dict(sample_top_p=p, sample_top_k=top_k or None)
        gen_d, ln_d, lp_d = run(**kw)
        assert len(record) == gen_d.shape[0] - 1 and int((gen_d == synth.EOS).sum()) == 2 * bs
        first_close = check(gen_d, lp_d, top_k)
        gen_2, ln_2, lp_2 = run(**kw)
        assert torch.equal(gen_d, gen_2) and torch.equal(ln_d, ln_2)
        assert_bits_equal(lp_d, lp_2, 'log-probabilities of a second run')
        with monkeypatch.context() as mp:           # the twin route on the device logits
            mp.setattr(decoder, 'VOCAB_SELECT_MAX_K', 0)
            called = []
            mp.setattr(decoder.ops, 'vocab_nucleus_sample', lambda *a, **k: called.append(a))
            gen_t, ln_t, lp_t = run(**kw)
        assert not called, 'VOCAB_SELECT_MAX_K = 0 must take the twin'
        stop = min(gen_d.shape[0], gen_t.shape[0]) if first_close is None else first_close
        assert torch.equal(gen_d[:stop], gen_t[:stop]), (top_k, first_close)
        if first_close is None:
            assert torch.equal(gen_d, gen_t) and torch.equal(ln_d, ln_t)
        # off: the plain seeded run, bit for bit
        base = run(sample_top_k=top_k or None)
        for off in (None, 1.0):
            got = run(sample_top_p=off, sample_top_k=top_k or None)
            assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
            assert_bits_equal(got[2], base[2], 'top_p %r: log-probabilities' % (off,))
    assert torch.equal(torch.cuda.get_rng_state(), cuda_state), 'the seeded path consumed torch\'s CUDA generator'
