"""Seeded top-k sampling over more than 16 candidates on the device (csrc/select.hip: m3p_vocab_sample_wide;
ops.vocab_sample_wide; decoder.generate(sample_seed=..., sample_top_k=40[, sample_top_p=0.9])).

The contract, the tolerance WIDE_NUCLEUS_TOL and the CPU part are in tests/test_vocab_sample_wide_cpu.py.  Here every row of
every launch is held to the NumPy twin: conditions (a) - (d) of tests/test_vocab_sample.py (the key within KEY_ATOL of the
fp64 key of the drawn word, that key within 2 KEY_ATOL of the row's best, the word inside the allowed set, logprob within
lse_bar), and with top_p the per-row rule of tests/test_vocab_nucleus.py for the cut - the vacuity of that rule is asserted
from the twin alone before a device result is looked at."""
import math

import numpy as np
import pytest
import torch

from m3p_amd import rng, synth
from tests.test_vocab_nucleus import NUCLEUS_TOL, _cut_accepted, _margin
from tests.test_vocab_sample import CHUNK, KEY_ATOL, _check_rows, _hip_model, _logits, _unfinished_before, lse_bar
from tests.test_vocab_sample_wide_cpu import CASES, TEMPERATURES, WIDE_MAX_K, WIDE_NUCLEUS_TOL
from tests.util import assert_bits_equal, poisoned_outputs

BF16 = torch.bfloat16
NAMES = ('words', 'logprob', 'key', 'cut')


def _run(dev, V, T, seed, top_k, top_p=None):
    from m3p_amd import ops
    n = dev.shape[0]
    with poisoned_outputs():
        res = ops.vocab_sample_wide(dev, V, T, seed, top_k, top_p)
    assert res is not None
    torch.cuda.synchronize()
    words, logprob, key, cut = res
    assert words.shape == logprob.shape == key.shape == cut.shape == (n,)
    assert words.dtype == torch.int64 and logprob.dtype == key.dtype == cut.dtype == torch.float32
    return res


def _clear_rows(x32, inv_t, top_p, top_k, n, what, min_outside=None, tol=WIDE_NUCLEUS_TOL):
    """From the twin alone: the rows whose margin exceeds the tolerance, and that enough of them do."""
    p = float(np.float32(top_p))
    cut_t, inside_t, above_t = rng.nucleus_cut(x32, inv_t, p, top_k)
    margin = _margin(inside_t, above_t, p)
    clear = margin > tol
    if min_outside is None:
        min_outside = 1.0 if n <= 6 else (0.95 if top_p >= 0.99 else 0.98)
    assert clear.mean() >= min_outside, (what, float(clear.mean()), float(margin.min()))
    return cut_t, clear


def _hold_to_twin(x32, dev, V, T, seed, top_k, top_p, key64, what, cand=None):
    """One launch against the twin -> the four outputs.  top_p None: the plain draw over the candidates, cut = -inf.
    The candidate set K is the twin's on the whole row; masses, cut and keys are then taken on the sub-row of K's columns in
    word order (xk, k64: [n, top_k]) - the twin's functions with every column a candidate, which is what "over K" means
    (tests/test_vocab_sample_wide_cpu.py holds the two against each other) and spares a sort of the whole row per launch."""
    n = x32.shape[0]
    inv_t = rng.inv_temperature(T)
    cand = rng.sample_allowed(x32, top_k) if cand is None else cand
    cols = np.nonzero(cand)[1].reshape(n, top_k)
    xk, k64 = np.take_along_axis(x32, cols, 1), np.take_along_axis(key64, cols, 1)
    if top_p is not None:
        cut_t, clear = _clear_rows(xk, inv_t, top_p, top_k, n, what)
    got = _run(dev, V, T, seed, top_k, top_p)
    words, logprob, key, cut = (t.cpu().numpy() for t in got)
    rows = np.arange(n)
    assert ((words >= 0) & (words < V)).all() and cand[rows, words].all(), what              # (c): a candidate
    at = (cols == words[:, None]).argmax(1)
    if top_p is None:
        assert (cut == -np.inf).all(), what
        allowed = np.ones_like(xk, dtype=bool)
    else:
        p = float(np.float32(top_p))
        ok, inside, above = _cut_accepted(xk, inv_t, p, top_k, cut, tol=WIDE_NUCLEUS_TOL)
        bad = np.flatnonzero(~ok)
        assert ok.all(), (what, 'rows', bad[:5], 'cut', cut[bad[:5]], 'twin', cut_t[bad[:5]], inside[bad[:5]], above[bad[:5]])
        assert np.array_equal(cut[clear].astype(np.float64), cut_t[clear]), what
        allowed = xk >= cut[:, None]
    a = float(np.abs(x32[np.isfinite(x32)]).max()) * inv_t
    atol = KEY_ATOL(a)
    err, short = _check_rows(key, at, k64, allowed, atol)                                    # (c): inside the allowed set
    print('%s: |key - key64| %.3g (bar %.3g), shortfall %.3g' % (what, err, atol, short))
    assert err <= atol, (what, err, atol)                                                    # (a)
    assert short <= 2 * atol, (what, short, atol)                                            # (b)
    y = np.where(allowed, xk.astype(np.float64) * inv_t, -np.inf)
    mx = y.max(1)
    lp64 = y[rows, at] - (mx + np.log(np.exp(y - mx[:, None]).sum(1)))
    lerr = float(np.nan_to_num(np.abs(logprob.astype(np.float64) - lp64), nan=np.inf).max())
    assert lerr <= lse_bar(a), (what, lerr, lse_bar(a))                                      # (d)
    return got


def _against_the_twin(full, V, n, ks, top_ps):
    dev = full.cuda()
    x32 = full[:, :V].float().numpy()
    seed, other = rng.stream_seed(V, n, 1), rng.stream_seed(V, n, 2)
    cands = {top_k: rng.sample_allowed(x32, top_k) for top_k in ks}
    for T in TEMPERATURES:
        key64 = rng.sample_keys(x32, rng.inv_temperature(T), seed)
        for top_k in ks:
            for top_p in top_ps:
                what = 'V %d n %d inv_t %.2f top_k %d top_p %r' % (V, n, 1 / T, top_k, top_p)
                got = _hold_to_twin(x32, dev, V, T, seed, top_k, top_p, key64, what, cands[top_k])
                again = _run(dev, V, T, seed, top_k, top_p)
                for g, h, name in zip(got, again, NAMES):
                    assert_bits_equal(g, h, what + ': a second launch, ' + name)
                diff = _run(dev, V, T, other, top_k, top_p)
                assert_bits_equal(diff[3], got[3], what + ': another seed, the cut')
                assert not torch.equal(diff[2], got[2]), what + ': another seed, the same keys'


@pytest.mark.gpu
@pytest.mark.parametrize('case', range(len(CASES)))
def test_vocab_sample_wide_against_the_twin(case):
    (V, ld, n), ks = CASES[case]
    _against_the_twin(_logits(n, V, ld, seed=V + n), V, n, ks, (None,))


@pytest.mark.gpu
def test_vocab_sample_wide_on_mostly_distinct_top_values():
    """randn * 4 at the full width: the top of a row is mostly distinct values, the k-th place rarely inside a tie."""
    V, ld, n = 250002, 250112, 2
    full = _logits(n, V, ld, seed=V + n)
    g = torch.Generator().manual_seed(V)
    full[:, :V] = (torch.randn((n, V), generator=g) * 4).to(BF16)
    x32 = full[:, :V].float().numpy()
    assert all(np.unique(np.sort(x32[r])[-17:]).size >= 12 for r in range(n))
    _against_the_twin(full, V, n, (17, 50, 1024), (None, 0.9))


@pytest.mark.gpu
@pytest.mark.parametrize('case', range(len(CASES)))
def test_vocab_sample_wide_nucleus_against_the_twin(case):
    (V, ld, n), ks = CASES[case]
    full = _logits(n, V, ld, seed=V + n)
    _against_the_twin(full, V, n, ks, (0.5, 0.9, 0.99))
    # off: None and >= 1 are the plain wide draw, bit for bit, with cut = -inf
    dev = full.cuda()
    seed = rng.stream_seed(V, n, 1)
    for top_k in ks[:2]:
        base = _run(dev, V, 1.0, seed, top_k)
        assert (base[3] == float('-inf')).all()
        for off in (1.0, 1.25):
            got = _run(dev, V, 1.0, seed, top_k, off)
            for g, h, name in zip(got, base, NAMES):
                assert_bits_equal(g, h, 'top_p %r top_k %d: %s' % (off, top_k, name))


@pytest.mark.gpu
def test_vocab_sample_wide_planted_cases():
    from m3p_amd import lib, ops
    V, ld, n = 2 * CHUNK + 2, 8448, 6
    full = _logits(n, V, ld, seed=11, amp=1.0)       # |x| <= 1 under the planted values
    T, top_k = 1.0, 17
    hi, tie = 10.0625, 10.0                          # neighbouring bf16 values: nearly equal masses
    # row 0: 2 words above, the class at the k-th place in all three chunks (6 + 12 + 2 words); the quota of 15 ends inside
    # the middle chunk, after its ninth member
    ties0 = [7, 100, 900, 2047, 2048, 4095] + [CHUNK + c for c in (0, 9, 500, 2047, 2048, 2049, 3000, 3001, 3500, 3600, 4000, 4095)] + [2 * CHUNK, 2 * CHUNK + 1]
    full[0, torch.tensor([200, CHUNK + 1000])] = hi
    full[0, torch.tensor(ties0)] = tie
    # row 1: 14 words above; the class holds the last column of chunk 0 and the first of chunk 1, and the quota of 3 ends
    # exactly between them
    ties1 = [10, 20, CHUNK - 1, CHUNK, CHUNK + 200, 2 * CHUNK]
    full[1, torch.tensor([3, 50, 300, 2047, 2048, 4000, CHUNK + 1, CHUNK + 77, CHUNK + 2048, CHUNK + 4095, 2 * CHUNK + 1, 1000, 1001, 1002])] = hi
    full[1, torch.tensor(ties1)] = tie
    # row 2: 20 finite logits, the rest -inf
    finite2 = [0, 5, 2047, 2048, 4095, CHUNK, CHUNK + 1, CHUNK + 3000, 2 * CHUNK, 2 * CHUNK + 1] + list(range(600, 610))
    keep = full[2, torch.tensor(finite2)].clone()
    full[2, :V] = float('-inf')
    full[2, torch.tensor(finite2)] = keep
    # rows 3 - 5: the winner forced into column 0, column V - 1 and the first column of the last chunk
    forced = [0, V - 1, 2 * CHUNK]
    for r, col in zip((3, 4, 5), forced):
        full[r, col] += 40.0
    dev = full.cuda()
    x32 = full[:, :V].float().numpy()
    K = rng.sample_allowed(x32, top_k)
    in0 = sorted(set(np.flatnonzero(K[0]).tolist()) & set(ties0))
    in1 = sorted(set(np.flatnonzero(K[1]).tolist()) & set(ties1))
    assert in0 == ties0[:15] and CHUNK < in0[-1] < 2 * CHUNK and in1 == [10, 20, CHUNK - 1] and K.sum(1).tolist() == [top_k] * n
    seeds = [rng.stream_seed(s, 1, 7) for s in range(64)]
    twin = np.stack([rng.sample_words(x32[:2], 1.0, s, top_k)[0] for s in seeds])
    assert {in0[0], in0[-1]} <= set(twin[:, 0].tolist()) and in1[-1] in set(twin[:, 1].tolist())        # (the twin alone)
    seen = [set(), set()]
    for i, seed in enumerate(seeds):
        if i < 4:
            got = _hold_to_twin(x32, dev, V, T, seed, top_k, None, rng.sample_keys(x32, 1.0, seed), 'planted, seed %d' % i, K)
        else:
            got = _run(dev, V, T, seed, top_k)
        words = got[0].tolist()
        assert K[0, words[0]] and K[1, words[1]] and words[3:] == forced, words
        assert all(math.isfinite(float(v)) for t in got[1:3] for v in t)
        seen[0].add(words[0])
        seen[1].add(words[1])
    assert {in0[0], in0[-1]} <= seen[0] and in1[-1] in seen[1] and CHUNK not in seen[1], seen
    # the cut on the class at the k-th place: row 0 holds 2 + 15 nearly equal words, 0.5 of the mass ends inside the class
    seed = seeds[0]
    key64 = rng.sample_keys(x32, 1.0, seed)
    got = _hold_to_twin(x32, dev, V, T, seed, top_k, 0.5, key64, 'planted, top_p 0.5', K)
    assert got[3].tolist()[:2] == [tie, hi] and got[3].tolist()[3:] == [float(x32[r, c]) for r, c in zip((3, 4, 5), forced)]
    # row 2 at top_k = 50: K holds the 20 finite words and 30 of -inf; the word is one of the 20, their probabilities sum to 1
    a = float(np.abs(x32[np.isfinite(x32)]).max())
    for i, seed in enumerate(seeds[:8]):
        got = _hold_to_twin(x32, dev, V, T, seed, 50, None if i % 2 else 0.9, rng.sample_keys(x32, 1.0, seed), 'planted, top_k 50, seed %d' % i)
        w = int(got[0][2])
        assert w in finite2
        if i % 2:
            lse_dev = float(x32[2, w]) - float(got[1][2])
            total = float(np.exp(x32[2, finite2].astype(np.float64) - lse_dev).sum())
            assert abs(math.log(total)) <= lse_bar(a), (total, lse_bar(a))
    # limits: more than max_k words is declined and the plan says so; top_k = 0 and top_k > V raise
    max_k = ops.vocab_sample_wide_max_k()
    assert max_k == WIDE_MAX_K >= 1024
    assert ops.vocab_sample_wide(dev, V, T, seed, max_k + 1) is None
    assert not ops.vocab_sample_wide_takes(n, V, ld, max_k + 1) and ops.vocab_sample_wide_takes(n, V, ld, max_k)
    assert ops.vocab_sample_wide_takes(n, V, ld, 1) and ops.vocab_sample_wide_takes(n, V, ld, 17)
    for bad in (0, -1, V + 1):
        with pytest.raises(lib.M3PError):
            ops.vocab_sample_wide(dev, V, T, seed, bad)
        with pytest.raises(lib.M3PError):
            ops.vocab_sample_wide_takes(n, V, ld, bad)
    for bad in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError):
            ops.vocab_sample_wide(dev, V, T, seed, 17, bad)


@pytest.mark.gpu
@pytest.mark.parametrize('case', range(3))
def test_vocab_sample_wide_beside_the_narrow_route(case):
    """top_k = 16 and 5 through both entries: equal words, bit-equal keys (one function on the same inputs), logprob within
    twice the bar; with top_p = 0.9 the same against m3p_vocab_nucleus_sample, on the rows that the twin puts outside the
    larger of the two tolerances - all of them in these cases, asserted from the twin first."""
    from m3p_amd import ops
    (V, ld, n), _ = CASES[case]
    full = _logits(n, V, ld, seed=V + n)
    dev = full.cuda()
    x32 = full[:, :V].float().numpy()
    seed = rng.stream_seed(V, n, 1)
    for T in (1.0, 0.25):
        inv_t = rng.inv_temperature(T)
        bar = 2 * lse_bar(float(np.abs(x32).max()) * inv_t)
        for top_k in (16, 5):
            what = 'V %d inv_t %.2f top_k %d' % (V, inv_t, top_k)
            wide, narrow = _run(dev, V, T, seed, top_k), ops.vocab_sample(dev, V, T, seed, top_k)
            assert torch.equal(wide[0], narrow[0]), what
            assert_bits_equal(wide[2], narrow[2], what + ': keys')
            assert float((wide[1] - narrow[1]).abs().max()) <= bar, what
            _, clear = _clear_rows(x32, inv_t, 0.9, top_k, n, what, tol=max(NUCLEUS_TOL, WIDE_NUCLEUS_TOL))
            assert int((~clear).sum()) == 0, what                          # (the cap on rows that may differ by a class: none)
            wide, narrow = _run(dev, V, T, seed, top_k, 0.9), ops.vocab_nucleus_sample(dev, V, T, seed, 0.9, top_k)
            assert torch.equal(wide[0], narrow[0]) and torch.equal(wide[3], narrow[3]), what
            assert_bits_equal(wide[2], narrow[2], what + ': keys, top_p 0.9')
            assert float((wide[1] - narrow[1]).abs().max()) <= bar, what


@pytest.mark.gpu
@pytest.mark.parametrize('tag', ['multi', 'wide'])
def test_wide_generate_end_to_end(monkeypatch, tag):
    from m3p_amd import decoder
    m, c, src_enc, src_len = _hip_model(tag)
    bs, max_len, T, top_k = c['bs'], c['max_len'], 0.8, 40
    inv_t = rng.inv_temperature(T)
    record, wide_calls = [], []
    real_wide = decoder.ops.vocab_sample_wide

    def spy(logits, V, *a, **k):                     # (the logits the draw sees: behind the constraint kernel)
        record.append((logits.clone(), V))
        wide_calls.append(a)
        return real_wide(logits, V, *a, **k)

    def no_twin(*a, **k):
        raise AssertionError('the seeded draw left the device')

    monkeypatch.setattr(decoder.ops, 'vocab_sample_wide', spy)

    def run(**kw):
        del record[:]
        with torch.no_grad():
            return m.generate(src_enc, src_len, c['tgt_lang_id'], max_len=max_len, sample_temperature=T, sample_seed=5, **kw)

    def check(gen, lp, p):
        """Every step and open row against the recorded logits -> the first step at which some row lies inside a band (the
        twin's margin within WIDE_NUCLEUS_TOL, or its two best keys within 2 KEY_ATOL), None if there is none."""
        gen_h, open_, lp = gen.cpu().numpy(), _unfinished_before(gen.cpu()), lp.cpu()
        first_close = None
        for pos in range(1, gen_h.shape[0]):
            logits, V = record[pos - 1]
            x32 = logits[:, :V].float().cpu().numpy()
            a = float(np.abs(x32[np.isfinite(x32)]).max()) * inv_t
            key64 = rng.sample_keys(x32, inv_t, rng.stream_seed(5, pos, decoder.SAMPLE_SITE))
            allowed = rng.sample_allowed(x32, top_k)
            margin = np.full(bs, np.inf)
            if p is not None:
                cut_t, inside, above = rng.nucleus_cut(x32, inv_t, p, top_k)
                allowed &= x32 >= cut_t.astype(np.float32)[:, None]
                margin = _margin(inside, above, p)
            best = np.sort(np.where(allowed, key64, -np.inf), axis=1)[:, -2:]
            y = np.where(allowed, x32.astype(np.float64) * inv_t, -np.inf)
            lse = np.log(np.exp(y - y.max(1)[:, None]).sum(1)) + y.max(1)
            for b in range(bs):
                forced = pos == max_len - 1 and gen_h[pos, b] == synth.EOS and float(lp[pos, b]) == 0.0
                if not open_[pos, b] or forced:
                    assert float(lp[pos, b]) == 0.0, (pos, b)
                    continue
                if margin[b] <= WIDE_NUCLEUS_TOL or best[b, 1] - best[b, 0] < 2 * KEY_ATOL(a):
                    first_close = pos if first_close is None else first_close
                    continue
                w = int(gen_h[pos, b])
                assert w == int(np.where(allowed[b], key64[b], -np.inf).argmax()), (pos, b, w)     # the twin's word
                assert abs(float(lp[pos, b]) - (y[b, w] - lse[b])) <= lse_bar(a), (pos, b)
        return first_close

    cuda_state = torch.cuda.get_rng_state()
    for p in (None, 0.9):
        p32 = None if p is None else float(np.float32(p))
        kw = dict(sample_top_k=top_k, sample_top_p=p, return_logprobs=True)
        del wide_calls[:]
        with monkeypatch.context() as mp:
            mp.setattr(decoder, '_sample_twin', no_twin)
            gen_d, ln_d, lp_d = run(**kw)
            assert len(wide_calls) == len(record) == gen_d.shape[0] - 1 and int((gen_d == synth.EOS).sum()) == 2 * bs
            first_close = check(gen_d, lp_d, p32)
            gen_2, ln_2, lp_2 = run(**kw)
        assert torch.equal(gen_d, gen_2) and torch.equal(ln_d, ln_2)
        assert_bits_equal(lp_d, lp_2, 'log-probabilities of a second run')
        del wide_calls[:]
        with monkeypatch.context() as mp:           # the twin route on the device logits
            mp.setattr(decoder, 'VOCAB_SELECT_MAX_K', 0)
            gen_t, ln_t, lp_t = run(**kw)
        assert not wide_calls, 'VOCAB_SELECT_MAX_K = 0 must take the twin'
        stop = min(gen_d.shape[0], gen_t.shape[0]) if first_close is None else first_close
        assert torch.equal(gen_d[:stop], gen_t[:stop]), (p, first_close)
        if first_close is None:
            assert torch.equal(gen_d, gen_t) and torch.equal(ln_d, ln_t)
    assert torch.equal(torch.cuda.get_rng_state(), cuda_state), 'the seeded path consumed torch\'s CUDA generator'
    # the constraint kernel in front of the wide route
    cons_calls = []
    real_cons = decoder.ops.logits_constrain
    monkeypatch.setattr(decoder.ops, 'logits_constrain', lambda *a, **k: cons_calls.append(1) or real_cons(*a, **k))
    del wide_calls[:]
    with monkeypatch.context() as mp:
        mp.setattr(decoder, '_sample_twin', no_twin)
        gen_c, ln_c, lp_c = run(sample_top_k=top_k, sample_top_p=0.9, return_logprobs=True, no_repeat_ngram=2, min_len=4)
    assert len(wide_calls) == len(cons_calls) == gen_c.shape[0] - 1
    check(gen_c, lp_c, float(np.float32(0.9)))
    gen_h = gen_c.cpu().numpy()
    assert int(ln_c.min()) >= 4 + 2
    for b in range(bs):
        words = gen_h[1:int(ln_c[b]) - 1, b].tolist()
        grams = list(zip(words, words[1:]))
        assert len(grams) == len(set(grams)), (b, words)
    # 16 words and fewer keep their routes
    del wide_calls[:]
    run(sample_top_k=4)
    run(sample_top_k=4, sample_top_p=0.9)
    run(sample_top_k=16)
    run()
    assert not wide_calls
