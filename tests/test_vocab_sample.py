"""Seeded temperature / top-k sampling of the decoding loop (csrc/select.hip: m3p_vocab_sample; m3p_amd/rng.py: sample_*;
m3p_amd/decoder.py: generate(sample_seed=...)).

The contract (include/m3p_hip.h): for row r and word w < V,  m = hash32(r * V + w, seed) >> 8,  u = (m + 0.5) 2^-24,
E = -log(u),  key(r, w) = float(logit[r, w]) * inv_t - log(E);  the sampled word is the argmax of key over the allowed set
(top_k = 0: every word; otherwise the row's first top_k words under (logit descending, word ascending)), ties to the lowest
word;  logprob = x_w * inv_t - log-sum-exp of x * inv_t over the allowed set.  The NumPy twin computes all of it in fp64
from the very random numbers a launch uses, so every row of every launch is bounded, none excluded:

KEY_ATOL(a), a = max|x| * inv_t, bounds |fp32 key - fp64 key| from the documented accuracy of what the kernel calls:
  a u                the rounding of the product x * inv_t (u = 2^-24, the unit roundoff; the kernel's fma does not even round it)
  2 * 2 u            E = -logf(u) or -log1pf(-(1 - u)) from an EXACT argument: OCML documents logf at 1 ulp and log1pf at 2 ulp;
                     an ulp is at most 2 u relative, and a relative error of E is an absolute error of log(E)
  1 * 2 u * LMAX     the outer logf at 1 ulp of |log E| <= LMAX = 25 ln 2 = 17.33 (E >= -log(1 - 2^-25))
  (a + LMAX) u       the rounding of the difference, |key| <= a + LMAX
At a = 64 that is 1.1e-5.  It has to stay below 1e-4: the gap between the two largest keys of a row is about Exp(1)-
distributed, so among 4096 rows the smallest gap is around 1e-4 and a wider bound would leave the per-row checks blind."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from m3p_amd import rng, synth
from oracle import ref_cpu
from tests.util import assert_bits_equal, poisoned_outputs

BF16 = torch.bfloat16
CHUNK = 4096                    # VS_CHUNK of csrc/select.hip
U32 = 2.0 ** -24
LMAX = 25 * math.log(2.0)
INNER_ULP, OUTER_ULP = 2.0, 1.0


def KEY_ATOL(a):
    return a * U32 + INNER_ULP * 2 * U32 + OUTER_ULP * 2 * U32 * LMAX + (a + LMAX) * U32


def lse_bar(a):
    """The project's bar on a log-sum-exp (1e-5 at |x| <= 16, tests/test_vocab_select.py) scaled by the argument's magnitude."""
    return 1e-5 * max(1.0, a / 16.0)


def _hash32_py(idx, seed):
    """m3p_hash32 of csrc/common.hpp on Python integers."""
    h = (idx + seed) & 0xFFFFFFFF
    for k in (0x9E3779, 0x85EBCB, 0xC2B2AF):
        h ^= h >> 16
        h = (h + (h & 0xFFFFFF) * k) & 0xFFFFFFFF
    return h ^ (h >> 16)


def _chi2_quantile(dof, tail=1e-6):
    """The (1 - tail) quantile of chi-square with dof degrees of freedom."""
    try:
        from scipy import stats
        return float(stats.chi2.ppf(1.0 - tail, dof))
    except ImportError:
        assert tail == 1e-6
        z = 4.753424                                       # the (1 - 1e-6) quantile of the standard normal
        return dof * (1.0 - 2.0 / (9.0 * dof) + z * math.sqrt(2.0 / (9.0 * dof))) ** 3        # Wilson-Hilferty


def _chi2(counts, p):
    """Pearson's chi-square of counts against the probabilities p, bins with an expected count below 5 pooled into one.
    -> (statistic, degrees of freedom)."""
    n = counts.sum()
    exp = n * p
    small = exp < 5
    c, e = counts[~small].astype(np.float64), exp[~small]
    if small.any():
        c, e = np.append(c, counts[small].sum()), np.append(e, exp[small].sum())
    keep = e > 0
    assert counts[small].sum() == 0 or e[-1] > 0
    return float((((c - e) ** 2)[keep] / e[keep]).sum()), int(keep.sum()) - 1


def _softmax64(y):
    y = np.asarray(y, np.float64)
    e = np.exp(y - y.max())
    return e / e.sum()


def _dist_rows(V=40, n=65536):
    """n identical rows of V bf16-valued logits, normal with sigma 1.5."""
    g = torch.Generator().manual_seed(40)
    row = (torch.randn(V, generator=g) * 1.5).to(BF16)
    return row[None, :].expand(n, V).contiguous()


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_twin_uniform_follows_the_formula_on_hand_computed_hashes():
    s5 = rng.stream_seed(1, 5, 0)
    assert s5 == 2773082255
    # (row, word, V, seed, hash32(row * V + word, seed)): the last two have m >= 2^23, the upper half of u
    cases = [(0, 1, 40, 0, 0x5E90BCB0), (0, 7, 40, 12345, 0x7CEC1AAC), (0, 0, 40, 0, 0x0), (3, 5, 40, s5, 0xD8CBB3CB), (0, 2, 40, 7, 0xFCD1B011)]
    for r, w, V, seed, h in cases:
        assert _hash32_py(r * V + w, seed) == h == int(rng.hash32(r * V + w, seed))
        m = h >> 8
        u = rng.sample_uniform(r + 1, V, seed)
        assert u.shape == (r + 1, V) and u.dtype == np.float64
        assert u[r, w] == (m + 0.5) / 2.0 ** 24 and 0.0 < u[r, w] < 1.0
    assert (0xD8CBB3CB >> 8) >= 2 ** 23 and (0xFCD1B011 >> 8) >= 2 ** 23 > (0x7CEC1AAC >> 8)
    assert rng.sample_uniform(1, 1, 0)[0, 0] == 2.0 ** -25                                  # m = 0: the smallest u
    # keys and the whole contract on a small example, against a restatement with Python floats
    x = np.array([[0.5, -1.25, 3.0, 0.0], [2.0, 2.0, -0.75, 1.5]], dtype=np.float32)
    keys = rng.sample_keys(x, 0.5, 9)
    for r in range(2):
        for w in range(4):
            u = ((_hash32_py(r * 4 + w, 9) >> 8) + 0.5) / 2.0 ** 24
            assert abs(keys[r, w] - (float(x[r, w]) * 0.5 - math.log(-math.log(u)))) <= 1e-14
    words, logprob, key = rng.sample_words(x, 0.5, 9)
    assert words.dtype == np.int64 and words.tolist() == keys.argmax(1).tolist() and np.array_equal(key, keys.max(1))
    for r in range(2):
        p = _softmax64(x[r].astype(np.float64) * 0.5)
        assert abs(logprob[r] - math.log(p[words[r]])) <= 1e-14
    # top_k: the allowed set is the first top_k under (logit descending, word ascending)
    assert rng.sample_allowed(x, 2).tolist() == [[True, False, True, False], [True, True, False, False]]
    assert rng.sample_allowed(x, 3)[1].tolist() == [True, True, False, True]
    w2, lp2, _ = rng.sample_words(x, 0.5, 9, top_k=2)
    assert w2[0] in (0, 2) and w2[1] in (0, 1)
    p = _softmax64(np.array([0.5, 3.0]) * 0.5)
    assert abs(lp2[0] - math.log(p[[0, 2].index(int(w2[0]))])) <= 1e-14
    assert rng.sample_words(x, 0.5, 9, top_k=1)[0].tolist() == [2, 0]                       # top_k = 1 is greedy, ties to the lowest word


def test_twin_breaks_an_exact_key_tie_by_the_lowest_word(monkeypatch):
    x = np.array([[1.0, 3.0, 3.0, 0.5, 3.0], [0.5, -np.inf, 2.0, 2.0, -np.inf]], dtype=np.float32)
    monkeypatch.setattr(rng, 'sample_uniform', lambda n, V, seed: np.full((n, V), 0.3))
    keys = rng.sample_keys(x, 1.0, 0)
    assert keys[0, 1] == keys[0, 2] == keys[0, 4] and keys[1, 2] == keys[1, 3]
    for top_k in (0, 2, 3):
        words, logprob, _ = rng.sample_words(x, 1.0, 0, top_k=top_k)
        assert words.tolist() == [1, 2], top_k
    # -inf logits have probability 0 and do not disturb the log-probability
    _, logprob, _ = rng.sample_words(x, 1.0, 0)
    assert abs(logprob[1] - math.log(_softmax64([0.5, 2.0, 2.0])[1])) <= 1e-14


@pytest.mark.parametrize('T', [1.0, 2.0])
def test_twin_samples_the_tempered_distribution(T):
    """Pearson's chi-square of 65 536 draws against softmax(x / T) (and against the renormalised top 5), at the 1 - 1e-6
    quantile (96.1 at 39 degrees of freedom); the seeds are fixed, so this is deterministic.  (Observed: 24.8 - 43.7.)"""
    x16 = _dist_rows()
    x32 = x16.float().numpy()
    inv_t = rng.inv_temperature(T)
    p = _softmax64(x32[0].astype(np.float64) / T)
    top5 = rng.sample_allowed(x32[:1], 5)[0]
    p5 = np.where(top5, p, 0.0) / p[top5].sum()
    for s in (1, 2, 3):
        seed = rng.stream_seed(s, 5, 0)
        words, _, _ = rng.sample_words(x32, inv_t, seed)
        stat, dof = _chi2(np.bincount(words, minlength=x32.shape[1]), p)
        print('T %.1f seed %d: chi-square %.1f at %d degrees of freedom (bar %.1f)' % (T, s, stat, dof, _chi2_quantile(dof)))
        assert dof >= 30 and stat <= _chi2_quantile(dof), (T, s, stat, dof)
        words, _, _ = rng.sample_words(x32, inv_t, seed, top_k=5)
        counts = np.bincount(words, minlength=x32.shape[1])
        assert counts[~top5].sum() == 0
        stat, dof = _chi2(counts, p5)
        print('T %.1f seed %d top 5: chi-square %.1f at %d degrees of freedom (bar %.1f)' % (T, s, stat, dof, _chi2_quantile(dof)))
        assert dof == 4 and stat <= _chi2_quantile(dof), (T, s, stat, dof)


def _keys32(x32, inv_t, seed, fault=False):
    """The kernel's arithmetic restated in fp32 NumPy (vsmp_log_e of csrc/select.hip: logf of the exact u in the lower half of
    m, log1pf of the exact -(1 - u) in the upper half; the product rounded, then the difference).  fault: the upper half
    takes logf of u ROUNDED to fp32 - what a kernel without the log1pf branch would compute."""
    f32 = np.float32
    n, V = x32.shape
    m = (rng.hash32(np.arange(n * V, dtype=np.uint64), seed) >> np.uint32(8)).astype(np.int64).reshape(n, V)
    upper = m >= 2 ** 23
    lo = (2 * m + 1).astype(f32) * f32(2.0 ** -25)                      # u, exact where m < 2^23
    hi = (2 ** 25 - 2 * m - 1).astype(f32) * f32(2.0 ** -25)            # 1 - u, exact where m >= 2^23
    with np.errstate(divide='ignore', invalid='ignore'):
        e_hi = -np.log(lo) if fault else -np.log1p(-hi)
        E = np.where(upper, e_hi, -np.log(lo)).astype(f32)
        assert E.dtype == f32
        return ((x32 * f32(inv_t)).astype(f32) - np.log(E)).astype(f32)


def _check_rows(key_got, words_got, key64, allowed, atol):
    """(a) and (b) of the per-row contract -> (worst |key - key64[word]|, worst shortfall of key64[word] below the row's best)."""
    rows = np.arange(key64.shape[0])
    at = key64[rows, words_got]
    best = np.where(allowed, key64, -np.inf).max(1)
    err, short = np.abs(key_got.astype(np.float64) - at), best - at
    assert allowed[rows, words_got].all()
    return float(np.nan_to_num(err, nan=np.inf).max()), float(short.max())


@pytest.fixture(scope='module')
def err_model_logits():
    g = torch.Generator().manual_seed(4096)
    return ((torch.rand((4096, 1000), generator=g) * 2 - 1) * 16).to(BF16).float().numpy()


@pytest.mark.parametrize('inv_t', [0.25, 1.0, 4.0])
def test_key_error_model_holds_for_the_fp32_restatement(err_model_logits, inv_t):
    x32 = err_model_logits
    assert KEY_ATOL(64.0) <= 1e-4
    a = float(np.abs(x32).max()) * inv_t
    atol = KEY_ATOL(a)
    key64 = rng.sample_keys(x32, inv_t, 77)
    k32 = _keys32(x32, inv_t, 77)
    every = float(np.abs(k32.astype(np.float64) - key64).max())
    words = k32.argmax(1)
    err, short = _check_rows(k32[np.arange(len(words)), words], words, key64, np.ones_like(key64, bool), atol)
    gap = np.sort(key64, axis=1)
    gap = gap[:, -1] - gap[:, -2]
    print('inv_t %.2f: KEY_ATOL %.3g; fp32 restatement: every key within %.3g, winners within %.3g, shortfall %.3g; '
          'smallest top-two gap %.3g, %.3f %% of rows under 2 KEY_ATOL' % (inv_t, atol, every, err, short, gap.min(),
                                                                           100.0 * (gap < 2 * atol).mean()))
    assert every <= atol and err <= atol and short <= 2 * atol


def test_per_row_check_sees_a_fault_the_global_check_passes(err_model_logits):
    """u rounded to fp32 in the upper half (no log1pf branch): E is off by up to 2^-25 / E relative, which matters exactly
    for the keys that win (small E).  Agreement of the words and the relative L2 error of the winning keys - a loose global
    check - pass; the per-row bound does not."""
    x32, inv_t = err_model_logits, 1.0
    atol = KEY_ATOL(float(np.abs(x32).max()) * inv_t)
    key64 = rng.sample_keys(x32, inv_t, 77)
    bad = _keys32(x32, inv_t, 77, fault=True)
    rows = np.arange(x32.shape[0])
    words = bad.argmax(1)
    got, ref = bad[rows, words].astype(np.float64), key64.max(1)
    agree = float((words == key64.argmax(1)).mean())
    rel = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    err, _ = _check_rows(bad[rows, words], words, key64, np.ones_like(key64, bool), atol)
    print('fault: words agree in %.2f %% of rows, relative L2 of the winning keys %.3g; worst row %.3g against KEY_ATOL %.3g'
          % (100 * agree, rel, err, atol))
    assert agree >= 0.99 and rel <= 1e-3                    # the loose global check (below every global bar of tests/util.py) passes
    assert err > atol                                       # the per-row check does not


def _oracle_backed(monkeypatch, c, sd, record=None):
    """m3p_amd.decoder's search loops with the oracle as the step function (the lines of tests/test_decoder.py); record
    collects every step's scores."""
    from m3p_amd import decoder

    def fwd(model, x, lengths, src_enc, src_len, positions, langs, cache):
        cache['slen'] = x.shape[0]
        return ref_cpu.decoder_crossfwd(sd, c['n_dec_layers'], c['n_heads'], x, lengths, src_enc, src_len, positions, langs)[-1:]

    def scores(model, h):
        s = ref_cpu.word_scores(sd, h)
        if record is not None:
            record.append(s.clone())
        return s

    monkeypatch.setattr(decoder, 'decoder_forward', fwd)
    monkeypatch.setattr(decoder, 'word_scores', scores)
    return SimpleNamespace(n_words=c['n_words'], pad_index=synth.PAD, eos_index=synth.EOS, dim=c['emb_dim'],
                           embeddings=SimpleNamespace(weight=torch.zeros(1)))


def _unfinished_before(gen):
    """[cur_len, bs] bool: was the sentence still open when position p was decoded?"""
    gen = np.asarray(gen)
    open_ = np.ones(gen.shape, bool)
    for p in range(2, gen.shape[0]):
        open_[p] = open_[p - 1] & (gen[p - 1] != synth.EOS)
    open_[0] = False
    return open_


def test_seeded_generate_on_the_oracle_step(monkeypatch):
    from m3p_amd import decoder
    tag = 'multi'
    c, P, sd, src_enc, src_len, x, lengths = synth.decoder_case(tag)
    record = []
    stub = _oracle_backed(monkeypatch, c, sd, record)
    bs, max_len = c['bs'], c['max_len']
    run = lambda **kw: decoder.generate(stub, src_enc, src_len, c['tgt_lang_id'], max_len=max_len, **kw)   # noqa: E731
    state = torch.random.get_rng_state()
    g1, l1 = run(sample_seed=3)
    g2, l2 = run(sample_seed=3)
    assert torch.equal(torch.random.get_rng_state(), state), 'the seeded path consumed torch\'s generator'
    assert torch.equal(g1, g2) and torch.equal(l1, l2) and g1.dtype == torch.int64
    g4, l4 = run(sample_seed=4)
    assert g4.shape != g1.shape or not torch.equal(g4, g1)
    # finished sentences are padded; <EOS> opens every sentence and closes it
    for gen, ln in ((g1, l1), (g4, l4)):
        assert int((gen == synth.EOS).sum()) == 2 * bs and (gen[0] == synth.EOS).all()
        for b in range(bs):
            n = int(ln[b])
            assert gen[n - 1, b] == synth.EOS and (gen[n:, b] == synth.PAD).all() and (gen[1:n - 1, b] != synth.EOS).all()
    # top_k = 1 is greedy, whatever the seed and the temperature
    greedy, greedy_len = run()
    for seed, T in ((3, None), (11, 0.5), (12, 3.0)):
        gk, lk = run(sample_seed=seed, sample_top_k=1, sample_temperature=T)
        assert torch.equal(gk, greedy) and torch.equal(lk, greedy_len), (seed, T)
    # the log-probabilities, against the scores the loop was handed
    for T, top_k in ((1.0, None), (0.8, None), (0.8, 4)):
        del record[:]
        gen, ln, lp = run(sample_seed=5, sample_temperature=T, sample_top_k=top_k, return_logprobs=True)
        assert lp.dtype == torch.float32 and lp.shape == gen.shape and len(record) == gen.shape[0] - 1
        open_ = _unfinished_before(gen)
        worst = 0.0
        for p in range(1, gen.shape[0]):
            s = record[p - 1].double() / T
            if top_k:
                kth = torch.topk(s, top_k, dim=1)[0][:, -1:]
                s = torch.where(s >= kth, s, torch.full_like(s, -math.inf))
            ref = (s.gather(1, gen[p].clamp(min=0)[:, None]).squeeze(1) - torch.logsumexp(s, dim=1))
            for b in range(bs):
                forced = p == max_len - 1 and gen[p, b] == synth.EOS and float(lp[p, b]) == 0.0
                if open_[p, b] and not forced:
                    assert math.isfinite(float(ref[b]))
                    worst = max(worst, abs(float(lp[p, b]) - float(ref[b])))
                else:
                    assert float(lp[p, b]) == 0.0, (p, b)
        assert (lp[0] == 0).all() and worst <= 1e-5, (T, top_k, worst)
        g_again, l_again = run(sample_seed=5, sample_temperature=T, sample_top_k=top_k)
        assert torch.equal(g_again, gen) and torch.equal(l_again, ln)
    # the modes that need a seed say so
    with pytest.raises(ValueError):
        run(sample_top_k=3)
    with pytest.raises(ValueError):
        run(sample_temperature=0.7, sample_top_k=3)
    with pytest.raises(ValueError):
        run(return_logprobs=True)


def test_unseeded_sampling_is_still_torch_multinomial(monkeypatch):
    """sample_temperature without a seed: the torch path on torch's generator, replayed draw for draw."""
    from m3p_amd import decoder
    c, P, sd, src_enc, src_len, x, lengths = synth.decoder_case('multi')
    record = []
    stub = _oracle_backed(monkeypatch, c, sd, record)
    torch.manual_seed(5)
    gen, ln = decoder.generate(stub, src_enc, src_len, c['tgt_lang_id'], max_len=c['max_len'], sample_temperature=0.7)
    after = torch.random.get_rng_state()
    torch.manual_seed(5)
    open_ = _unfinished_before(gen)
    for p in range(1, gen.shape[0]):
        words = torch.multinomial(torch.softmax(record[p - 1] / 0.7, dim=1), 1).squeeze(1)
        for b in range(c['bs']):
            forced = p == c['max_len'] - 1 and gen[p, b] == synth.EOS
            if open_[p, b] and not forced:
                assert gen[p, b] == words[b], (p, b)
    assert torch.equal(torch.random.get_rng_state(), after)


# ------------------------------------------------------------------------------------------------------------------ GPU
def _logits(n, V, ld, seed, amp=16.0):
    """bf16 [n, ld], |x| <= amp in the V real columns, NaN / +inf alternating behind them (as tests/test_vocab_select.py)."""
    g = torch.Generator().manual_seed(seed)
    x = ((torch.rand((n, V), generator=g) * 2 - 1) * amp).to(BF16)
    full = torch.empty((n, ld), dtype=BF16)
    full[:, :V] = x
    full[:, V::2] = float('nan')
    full[:, V + 1::2] = float('inf')
    return full


def _run(dev, V, T, seed, top_k):
    from m3p_amd import ops
    n = dev.shape[0]
    with poisoned_outputs():
        res = ops.vocab_sample(dev, V, T, seed, top_k)
    assert res is not None
    words, logprob, key = res
    torch.cuda.synchronize()
    assert words.shape == logprob.shape == key.shape == (n,)
    assert words.dtype == torch.int64 and logprob.dtype == torch.float32 and key.dtype == torch.float32
    return words, logprob, key


def _hold_to_twin(full, dev, V, T, seed, top_k, key64, what):
    """One launch against the twin: (a) - (d) of the contract for every row.  -> (words, worst (a), worst (d))."""
    x32 = full[:, :V].float().numpy()
    inv_t = rng.inv_temperature(T)
    a = float(np.abs(x32[np.isfinite(x32)]).max()) * inv_t
    atol = KEY_ATOL(a)
    words_t, logprob_t, key_t = _run(dev, V, T, seed, top_k)
    words, logprob, key = words_t.cpu().numpy(), logprob_t.cpu().numpy(), key_t.cpu().numpy()
    assert ((words >= 0) & (words < V)).all(), what                                          # (c)
    allowed = rng.sample_allowed(x32, top_k)
    rows = np.arange(x32.shape[0])
    assert allowed[rows, words].all(), what                                                  # (c): inside the twin's top-k set
    err, short = _check_rows(key, words, key64, allowed, atol)
    assert err <= atol, (what, err, atol)                                                    # (a)
    assert short <= 2 * atol, (what, short, atol)                                            # (b)
    y = np.where(allowed, x32.astype(np.float64) * inv_t, -np.inf)
    mx = y.max(1)
    lp64 = y[rows, words] - (mx + np.log(np.exp(y - mx[:, None]).sum(1)))
    lerr = float(np.nan_to_num(np.abs(logprob.astype(np.float64) - lp64), nan=np.inf).max())
    assert lerr <= lse_bar(a), (what, lerr, lse_bar(a))                                      # (d)
    return (words_t, logprob_t, key_t), err, lerr


@pytest.mark.gpu
@pytest.mark.parametrize('V,ld,n', [
    (1000, 1024, 3),                                # one partial chunk
    (2 * CHUNK + 2, 8448, 5),                       # whole chunks plus two columns
    (1000, 1024, 1),                                # a single row
    (250002, 250112, 2),                            # the full width
    (40, 40, 4096),                                 # many rows, tiny V
    (2059, 2304, 3),                                # a chunk's second half: one whole load, a 3-column tail, the rest past V
])
def test_vocab_sample_against_the_twin(V, ld, n):
    from m3p_amd import ops
    full = _logits(n, V, ld, seed=V + n)
    dev = full.cuda()
    x32 = full[:, :V].float().numpy()
    seed, other = rng.stream_seed(V, n, 1), rng.stream_seed(V, n, 2)
    worst_a = worst_d = 0.0
    for T in (4.0, 1.0, 0.25):                      # inv_t 0.25, 1, 4
        key64 = rng.sample_keys(x32, rng.inv_temperature(T), seed)
        for top_k in (0, 1, 5, 16):
            if top_k > V:
                continue
            what = 'V %d n %d inv_t %.2f top_k %d' % (V, n, 1 / T, top_k)
            got, err, lerr = _hold_to_twin(full, dev, V, T, seed, top_k, key64, what)
            worst_a, worst_d = max(worst_a, err), max(worst_d, lerr)
            again = _run(dev, V, T, seed, top_k)
            for g, h, name in zip(got, again, ('words', 'logprob', 'key')):
                assert_bits_equal(g, h, what + ': a second launch, ' + name)
            diff = _run(dev, V, T, other, top_k)
            assert top_k == 1 or not torch.equal(diff[2], got[2]), what + ': another seed, the same keys'
            if top_k == 1:
                greedy = ops.vocab_select(dev, V, None, 1, 1)[1].squeeze(1)
                assert torch.equal(got[0], greedy) and torch.equal(diff[0], greedy), what
    print('V %d ld %d n %d: max |key - key64| = %.3g, max |logprob - fp64| = %.3g' % (V, ld, n, worst_a, worst_d))


@pytest.mark.gpu
def test_vocab_sample_planted_cases():
    from m3p_amd import ops
    V, ld, n = 2 * CHUNK + 2, 8448, 5
    full = _logits(n, V, ld, seed=11, amp=8.0)
    seed, T = rng.stream_seed(11, 0, 3), 1.0
    atol = KEY_ATOL(48.0)
    base = rng.sample_keys(full[:, :V].float().numpy(), 1.0, seed)
    order = np.argsort(-base[0])
    assert base[0, order[1]] - base[0, order[2]] > 2 * atol and base[0, order[0]] - base[0, order[1]] > 2 * atol
    full[0, order[0]] = float('-inf')                   # row 0: the twin's winner removed - the runner-up it is
    full[1, 0] += 40.0                                  # rows 1 - 3: the winner forced into column 0, column V - 1
    full[2, V - 1] += 40.0                              # and the first column of the last chunk (others: key <= 8 + 17.4)
    full[3, 2 * CHUNK] += 40.0
    full[4, 7] = full[4, CHUNK + 9] = 12.0              # row 4: two equal top logits in two chunks
    dev = full.cuda()
    x32 = full[:, :V].float().numpy()
    key64 = rng.sample_keys(x32, 1.0, seed)
    got, _, _ = _hold_to_twin(full, dev, V, T, seed, 0, key64, 'planted')
    words = got[0].tolist()
    assert words[0] == order[1] and words[1:4] == [0, V - 1, 2 * CHUNK], words
    assert math.isfinite(float(got[1][0])) and math.isfinite(float(got[2][0]))
    for top_k in (1, 3, 16):
        got, _, _ = _hold_to_twin(full, dev, V, T, seed, top_k, key64, 'planted, top_k %d' % top_k)
        assert got[0].tolist()[1:4] == [0, V - 1, 2 * CHUNK] and got[0][0] != order[0]
    seen = set()
    for s in range(16):                                 # both equal logits are inside a top-2 set, and nothing else is
        ss = rng.stream_seed(s, 1, 3)
        got, _, _ = _hold_to_twin(full, dev, V, T, ss, 2, rng.sample_keys(x32, 1.0, ss), 'planted, top_k 2')
        seen.add(int(got[0][4]))
    assert seen == {7, CHUNK + 9}, seen
    # more than VS_MAX_K words: declined, and the plan says so
    assert ops.vocab_sample(dev, V, T, seed, top_k=17) is None
    assert not ops.vocab_sample_takes(n, V, ld, 17) and ops.vocab_sample_takes(n, V, ld, 16) and ops.vocab_sample_takes(n, V, ld, 0)


@pytest.mark.gpu
def test_vocab_sample_distribution_on_the_device():
    """The CPU chi-square case on the kernel, same bar; and word for word the twin's draw outside the band where the twin's
    own top-two gap is below 2 KEY_ATOL (expected: about 0.02 % of the rows)."""
    x16 = _dist_rows()
    x32 = x16.float().numpy()
    n, V = x32.shape
    seed = rng.stream_seed(1, 5, 0)
    words = _run(x16.cuda(), V, 1.0, seed, 0)[0].cpu().numpy()
    p = _softmax64(x32[0].astype(np.float64))
    stat, dof = _chi2(np.bincount(words, minlength=V), p)
    print('device: chi-square %.1f at %d degrees of freedom (bar %.1f)' % (stat, dof, _chi2_quantile(dof)))
    assert stat <= _chi2_quantile(dof)
    key64 = rng.sample_keys(x32, 1.0, seed)
    top2 = np.sort(key64, axis=1)[:, -2:]
    band = (top2[:, 1] - top2[:, 0]) < 2 * KEY_ATOL(float(np.abs(x32).max()))
    print('device: %d of %d rows inside the band, %d rows differ from the twin' % (band.sum(), n, (words != key64.argmax(1)).sum()))
    assert band.mean() <= 0.005
    assert np.array_equal(words[~band], key64.argmax(1)[~band])


def _hip_model(tag):
    from m3p_amd.model.transformer import TransformerModel
    c, P, sd, src_enc, src_len, x, lengths = synth.decoder_case(tag)
    torch.manual_seed(0)
    m = TransformerModel(P, is_encoder=False, with_output=True, is_crossModal=True).cuda()
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected
    m.eval()
    return m, c, src_enc.cuda(), src_len.cuda()


@pytest.mark.gpu
def test_seeded_generate_end_to_end(monkeypatch):
    from m3p_amd import decoder
    m, c, src_enc, src_len = _hip_model('multi')
    bs, max_len, T = c['bs'], c['max_len'], 0.8
    inv_t = rng.inv_temperature(T)
    record = []
    real = decoder.word_logits16

    def recording(model, tensor):
        logits, V = real(model, tensor)
        record.append((logits.clone(), V))
        return logits, V

    monkeypatch.setattr(decoder, 'word_logits16', recording)
    gen_kw = dict(max_len=max_len)

    def run(**kw):
        del record[:]
        with torch.no_grad():
            return m.generate(src_enc, src_len, c['tgt_lang_id'], **gen_kw, **kw)

    def gaps_and_checks(gen, lp, seed, top_k):
        """(b) and (d) for every step and open row against the recorded logits -> the first step with a gap below 2 KEY_ATOL."""
        gen_h, open_ = gen.cpu().numpy(), _unfinished_before(gen.cpu())
        first_close = None
        for p in range(1, gen_h.shape[0]):
            logits, V = record[p - 1]
            x32 = logits[:, :V].float().cpu().numpy()
            a = float(np.abs(x32).max()) * inv_t
            key64 = rng.sample_keys(x32, inv_t, rng.stream_seed(seed, p, decoder.SAMPLE_SITE))
            allowed = rng.sample_allowed(x32, top_k)
            best = np.sort(np.where(allowed, key64, -np.inf), axis=1)[:, -2:]
            y = np.where(allowed, x32.astype(np.float64) * inv_t, -np.inf)
            lse = np.log(np.exp(y - y.max(1)[:, None]).sum(1)) + y.max(1)
            for b in range(bs):
                forced = p == max_len - 1 and gen_h[p, b] == synth.EOS and (lp is None or float(lp[p, b]) == 0.0)
                if not open_[p, b] or forced:
                    assert gen_h[p, b] in ((synth.PAD, synth.EOS) if forced else (synth.PAD,))
                    assert lp is None or float(lp[p, b]) == 0.0, (p, b)       # (a drawn <PAD> word is not a pad position)
                    continue
                w = int(gen_h[p, b])
                assert allowed[b, w] and key64[b, w] >= best[b, 1] - 2 * KEY_ATOL(a), (p, b, w)              # (b)
                if lp is not None:
                    assert abs(float(lp[p, b]) - (y[b, w] - lse[b])) <= lse_bar(a), (p, b)                   # (d)
                if best[b, 1] - best[b, 0] < 2 * KEY_ATOL(a) and first_close is None:
                    first_close = p
        return first_close

    cuda_state = torch.cuda.get_rng_state()
    gen, ln, lp = run(sample_temperature=T, sample_seed=5, return_logprobs=True)
    assert lp.dtype == torch.float32 and lp.shape == gen.shape and (lp[0] == 0).all()
    assert len(record) == gen.shape[0] - 1 and int((gen == synth.EOS).sum()) == 2 * bs
    gaps_and_checks(gen, lp, 5, 0)
    gen2, ln2, lp2 = run(sample_temperature=T, sample_seed=5, return_logprobs=True)
    assert torch.equal(gen, gen2) and torch.equal(ln, ln2)
    assert_bits_equal(lp, lp2, 'log-probabilities of a second run')
    assert torch.equal(torch.cuda.get_rng_state(), cuda_state), 'the seeded path consumed torch\'s CUDA generator'
    assert not torch.equal(run(sample_temperature=T, sample_seed=6)[0], gen) or gen.shape[0] <= 2
    # top_k = 1 is greedy, token for token
    greedy, greedy_len = run()
    gk, lk = run(sample_temperature=T, sample_seed=5, sample_top_k=1)
    assert torch.equal(gk, greedy) and torch.equal(lk, greedy_len)
    # a truncated draw, and the twin route on the device logits: identical until a row's gap falls below 2 KEY_ATOL
    for top_k in (4, 0):
        kw = dict(sample_temperature=T, sample_seed=5, sample_top_k=top_k or None)
        gen_d, ln_d, lp_d = run(return_logprobs=True, **kw)
        first_close = gaps_and_checks(gen_d, lp_d, 5, top_k)
        with monkeypatch.context() as mp:
            mp.setattr(decoder, 'VOCAB_SELECT_MAX_K', 0)
            called = []
            mp.setattr(decoder.ops, 'vocab_sample', lambda *a, **k: called.append(a))
            gen_t, ln_t, lp_t = run(return_logprobs=True, **kw)
        assert not called, 'VOCAB_SELECT_MAX_K = 0 must take the twin'
        stop = min(gen_d.shape[0], gen_t.shape[0]) if first_close is None else first_close
        assert torch.equal(gen_d[:stop], gen_t[:stop]), (top_k, first_close)
        if first_close is None:
            assert torch.equal(gen_d, gen_t) and torch.equal(ln_d, ln_t)
