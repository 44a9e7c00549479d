"""Decoding constraints of the search loops: min_len, repetition_penalty, no_repeat_ngram, banned_words (csrc/constrain.hip:
m3p_logits_constrain; m3p_amd/decoder.py: constrain_scores_, generate / generate_beam; m3p_amd/ops.py: logits_constrain).

The contract (include/m3p_hip.h): at the step that decodes position cur_len, row r has the history H = generated[1:cur_len, r],
L = cur_len - 1 words, the <EOS> at position 0 NOT among them.  In this order: (1) every distinct word w of H inside [0, V) gets
x[w] <- bf16_rne(fl32(x[w] * (x[w] > 0 ? inv_theta : theta))), once however often it occurs; (2) for every j in [0, L - n] with
H[j + i] == H[L - n + 1 + i] for all i in [0, n - 2] the word H[j + n - 1] gets -inf; (3) <EOS> gets -inf while cur_len <=
min_len; (4) every banned id gets -inf.  Everything else keeps its bits.

Three statements of that rule are held to each other bit for bit: a brute-force restatement written here (Python loops over
rows, positions and words; its own bf16 rounding), the torch twin decoder.constrain_scores_, and the kernel.  No tolerance is
involved anywhere but in the log-probabilities of the sampled runs, which keep the bars of tests/test_vocab_sample.py."""
import math

import numpy as np
import pytest
import torch

from m3p_amd import decoder, rng, synth
from tests.test_decoder import G
from tests.test_vocab_sample import _hip_model, _logits, _oracle_backed, _unfinished_before, lse_bar
from tests.util import assert_bits_equal, poisoned_outputs

BF16 = torch.bfloat16
EOS, PAD = synth.EOS, synth.PAD
NEG_INF = float('-inf')
ALPHABET = (5, 9, 11, 20, 33)          # the history words of the CPU cases (none of them <EOS> or <PAD>)
FAULTS = ('penalty_per_occurrence', 'bos_counted', 'j_runs_to_L_minus_n_plus_1', 'ban_off_by_one', 'penalty_after_ban')


# ------------------------------------------------------------------------------------------------------ the brute force
def _bf16_rne(f):
    """fl32 -> the nearest bf16 (ties to even), as an fp32 number; by its bits, not through torch."""
    u = int(np.float32(f).view(np.uint32))
    if (u & 0x7FFFFFFF) >= 0x7F800000:
        return np.float32(f)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return np.uint32(u & 0xFFFFFFFF).view(np.float32)


def _brute(x, V, gen, cur_len, theta, inv_theta, ngram, eos, banned, fault=None):
    """The contract, word by word, on a copy of x fp32 [n, >= V] -> (result, facts); `fault` plants one of FAULTS.  facts: per
    row the words penalised, the words banned, and how often the most frequent history word occurs."""
    out = np.array(x, dtype=np.float32, copy=True)
    gen = np.asarray(gen)
    n = out.shape[0]
    th, inv = np.float32(theta), np.float32(inv_theta)
    facts = dict(penalised=[], banned=[], most=[])
    for r in range(n):
        H = [int(w) for w in gen[(0 if fault == 'bos_counted' else 1):cur_len, r]]
        Ln = len(H)
        row0 = out[r].copy()
        pen, ban = [], []
        if theta != 1.0 or inv_theta != 1.0:
            seen = set()
            for w in H:
                if not 0 <= w < V or (w in seen and fault != 'penalty_per_occurrence'):
                    continue
                seen.add(w)
                v = out[r, w]
                out[r, w] = _bf16_rne(np.float32(v * (inv if v > 0 else th)))
            pen = sorted(seen)
        if ngram >= 1 and Ln >= ngram:
            last = Ln - ngram + (1 if fault == 'j_runs_to_L_minus_n_plus_1' else 0)
            for j in range(0, last + 1):
                if all(H[j + i] == H[Ln - ngram + 1 + i] for i in range(ngram - 1)):
                    at = j + ngram - 1 - (1 if fault == 'ban_off_by_one' else 0)
                    # (the planted j = L - n + 1 reads one word past the history: position cur_len of the row)
                    w = H[at] if 0 <= at < Ln else int(gen[cur_len, r])
                    if 0 <= w < V:
                        ban.append(w)
        if eos >= 0:
            ban.append(eos)
        for w in (banned if banned is not None else ()):
            if 0 <= int(w) < V:
                ban.append(int(w))
        for w in ban:
            out[r, w] = -np.inf
        if fault == 'penalty_after_ban':                     # the penalty, computed from the untouched logits, lands last
            for w in pen:
                v = row0[w]
                out[r, w] = _bf16_rne(np.float32(v * (inv if v > 0 else th)))
        facts['penalised'].append(set(pen))
        facts['banned'].append(set(ban))
        facts['most'].append(max([H.count(w) for w in set(H)] or [0]))
    return out, facts


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.int32), np.asarray(b, np.float32).view(np.int32))


# ---------------------------------------------------------------------------------------------------------- CPU: the twin
V_CPU, LD_CPU, N_CPU = 50, 56, 6


def _cpu_case(name):
    """-> dict(x fp32 [n, ld] (bf16 numbers, a sentinel behind V), gen int64 [42, n], cur_len, pair, ngram, eos, banned, claims)."""
    rs = np.random.RandomState(sum(map(ord, name)))
    x = torch.from_numpy(((rs.rand(N_CPU, LD_CPU) * 2 - 1) * 6).astype(np.float32)).to(BF16).float()
    x[:, V_CPU:] = 768.0
    gen = np.full((42, N_CPU), PAD, dtype=np.int64)
    gen[0] = EOS
    gen[1:41] = np.asarray(ALPHABET)[rs.randint(0, len(ALPHABET), size=(40, N_CPU))]
    c = dict(x=x, gen=gen, eos=-1, banned=None, ngram=0, pair=(1.0, 1.0), cur_len=41)
    if name == 'long_trigram':         # theta > 1; row 0 ends in a word seen nowhere else: no trigram of it can repeat
        gen[40, 0] = 17
        gen[7, 1], gen[12, 2] = -1, V_CPU + 3                # history words outside [0, V): skipped
        x[1, ALPHABET[0]], x[2, ALPHABET[1]], x[3, ALPHABET[2]] = 0.0, -0.0, NEG_INF
        c.update(pair=decoder.penalty_pair(1.3), ngram=3, claims={'thrice', 'penalised_and_banned', 'row_without_ban'})
    elif name == 'long_bigram_lists':  # theta < 1, <EOS> and a ban list: one listed word is a history word, one lies past V
        c.update(pair=decoder.penalty_pair(0.5), ngram=2, eos=EOS, banned=[ALPHABET[3], 41, V_CPU + 2],
                 claims={'thrice', 'penalised_and_banned'})
    elif name == 'unigram':
        c.update(pair=decoder.penalty_pair(1.3), ngram=1, claims={'thrice', 'penalised_and_banned'})
    elif name == 'short_L_below_n':    # L = 2, n = 4
        c.update(pair=decoder.penalty_pair(1.3), ngram=4, cur_len=3, claims={'L<n', 'row_without_ban'})
    elif name == 'short_L_is_n_minus_1':
        gen[1:3, 0] = ALPHABET[0]
        c.update(pair=decoder.penalty_pair(1.3), ngram=3, cur_len=3, claims={'L==n-1', 'row_without_ban'})
    elif name == 'short_L_is_n':       # one window, j = 0: row 0 repeats one word, row 1 does not match
        gen[1:4, 0] = ALPHABET[0]
        gen[1:4, 1] = ALPHABET[:3]
        c.update(pair=decoder.penalty_pair(1.3), ngram=3, cur_len=4, claims={'L==n', 'penalised_and_banned', 'row_without_ban'})
    elif name == 'first_step':         # L = 0: only <EOS> and the list
        c.update(pair=decoder.penalty_pair(1.3), ngram=2, cur_len=1, eos=EOS, banned=[7], claims={'L<n'})
    else:
        raise KeyError(name)
    return c


CPU_CASES = ('long_trigram', 'long_bigram_lists', 'unigram', 'short_L_below_n', 'short_L_is_n_minus_1', 'short_L_is_n', 'first_step')


def _claims_hold(c, facts):
    """From the brute force alone: does the case contain what it claims?"""
    Ln, n = c['cur_len'] - 1, c['ngram']
    have = set()
    if max(facts['most']) >= 3:
        have.add('thrice')
    if any(p & b for p, b in zip(facts['penalised'], facts['banned'])):
        have.add('penalised_and_banned')
    if any(not b for b in facts['banned']):
        have.add('row_without_ban')
    if Ln < n:
        have.add('L<n')
    if Ln == n - 1:
        have.add('L==n-1')
    if Ln == n:
        have.add('L==n')
    assert c['claims'] <= have, (c['claims'] - have)


def _twin(c, dtype):
    s = c['x'].to(dtype).clone()
    banned = None if c['banned'] is None else torch.tensor(c['banned'], dtype=torch.long)
    got = decoder.constrain_scores_(s, V_CPU, torch.from_numpy(c['gen']), c['cur_len'], c['pair'][0], c['pair'][1], c['ngram'],
                                    c['eos'], banned)
    assert got is s and s.dtype == dtype
    return s.float().numpy()


@pytest.mark.parametrize('name', CPU_CASES)
def test_twin_against_brute_force(name):
    c = _cpu_case(name)
    ref, facts = _brute(c['x'].numpy(), V_CPU, c['gen'], c['cur_len'], c['pair'][0], c['pair'][1], c['ngram'], c['eos'], c['banned'])
    _claims_hold(c, facts)
    assert _same_bits(ref[:, V_CPU:], c['x'].numpy()[:, V_CPU:])
    for dtype in (torch.float32, BF16):
        assert _same_bits(_twin(c, dtype), ref), (name, dtype)
    # fp32 scores that are no bf16 numbers (the oracle's): the penalised values alone are rounded
    c['x'] = c['x'] * 1.0009765625 + 0.000123
    c['x'][:, V_CPU:] = 768.0
    ref, _ = _brute(c['x'].numpy(), V_CPU, c['gen'], c['cur_len'], c['pair'][0], c['pair'][1], c['ngram'], c['eos'], c['banned'])
    assert _same_bits(_twin(c, torch.float32), ref), name
    # all four off: not a bit moves
    off = decoder.constrain_scores_(c['x'].clone(), V_CPU, torch.from_numpy(c['gen']), c['cur_len'])
    assert _same_bits(off.numpy(), c['x'].numpy())


@pytest.mark.parametrize('fault,name', [
    ('penalty_per_occurrence', 'long_trigram'), ('bos_counted', 'long_trigram'), ('j_runs_to_L_minus_n_plus_1', 'long_trigram'),
    ('ban_off_by_one', 'long_trigram'), ('penalty_after_ban', 'long_bigram_lists'), ('bos_counted', 'short_L_is_n_minus_1'),
    ('j_runs_to_L_minus_n_plus_1', 'long_bigram_lists'), ('ban_off_by_one', 'long_bigram_lists')])
def test_comparison_sees_each_planted_fault(fault, name):
    """The comparison of test_twin_against_brute_force, with one fault planted in the brute force, fails: a penalty per
    occurrence, <BOS> counted as history, the match loop running to j = L - n + 1 (the suffix matching itself), the ban one
    position early, the penalty written behind the bans."""
    assert fault in FAULTS
    c = _cpu_case(name)
    args = (c['x'].numpy(), V_CPU, c['gen'], c['cur_len'], c['pair'][0], c['pair'][1], c['ngram'], c['eos'], c['banned'])
    good, _ = _brute(*args)
    bad, _ = _brute(*args, fault=fault)
    got = _twin(c, torch.float32)
    assert _same_bits(got, good) and not _same_bits(got, bad), (fault, name)


def test_every_fault_is_shown():
    params = [m for m in test_comparison_sees_each_planted_fault.pytestmark if m.name == 'parametrize'][0].args[1]
    assert {f for f, _ in params} == set(FAULTS)


def test_penalty_pair_and_bf16_rounding():
    assert decoder.penalty_pair(None) == (1.0, 1.0) and decoder.penalty_pair(1.0) == (1.0, 1.0)
    th, inv = decoder.penalty_pair(1.3)
    assert th == float(np.float32(1.3)) and inv == float(np.float32(1.0) / np.float32(1.3))
    for bad in (0.0, -1.0, float('inf'), float('nan'), 1e-46):
        with pytest.raises(ValueError):
            decoder.penalty_pair(bad)
    # the brute force's rounding is torch's
    rs = np.random.RandomState(3)
    v = np.concatenate([(rs.randn(4096) * 8).astype(np.float32), np.array([0.0, -0.0, -np.inf, 1.00390625, 1.01171875], np.float32)])
    mine = np.array([_bf16_rne(f) for f in v], np.float32)
    assert _same_bits(mine, torch.from_numpy(v).to(BF16).float().numpy())


# ------------------------------------------------------------------------------------------- CPU: the loops on the oracle step
def _sentences(gen, lengths):
    gen, lengths = np.asarray(gen), np.asarray(lengths)
    return [[int(w) for w in gen[1:lengths[b], b]] for b in range(gen.shape[1])]          # (the words and the closing <EOS>)


def _repeats(words, n):
    grams = [tuple(words[i:i + n]) for i in range(len(words) - n + 1)]
    return len(grams) - len(set(grams))


def _loops(monkeypatch, tag, record=None):
    c, P, sd, src_enc, src_len, x, lengths = synth.decoder_case(tag)
    stub = _oracle_backed(monkeypatch, c, sd, record)
    beam_size = c['beam_size'] or 2
    greedy = lambda **kw: decoder.generate(stub, src_enc, src_len, c['tgt_lang_id'], max_len=c['max_len'], **kw)     # noqa: E731
    beam = lambda **kw: decoder.generate_beam(stub, src_enc, src_len, c['tgt_lang_id'], beam_size, 1.0, False,      # noqa: E731
                                              max_len=c['max_len'], **kw)
    return c, greedy, beam


@pytest.mark.parametrize('tag', ['mono', 'multi', 'wide'])
def test_constrained_loops_on_the_oracle_step(tag, monkeypatch):
    c, greedy, beam = _loops(monkeypatch, tag)
    OFF = dict(min_len=0, repetition_penalty=None, no_repeat_ngram=0, banned_words=None)
    for loop, name in ((greedy, 'greedy'), (beam, 'beam')):
        base = loop()
        if name == 'greedy':                                 # today's output: the reference's golden vectors
            assert np.array_equal(base[0].numpy(), G[tag + '.greedy']) and np.array_equal(base[1].numpy(), G[tag + '.greedy_len'])
        elif c['beam_size']:
            key = tag + '.beam_lp1.0_es0'
            assert np.array_equal(base[0].numpy(), G[key]) and np.array_equal(base[1].numpy(), G[key + '_len'])
        for off in (OFF, dict(repetition_penalty=1.0, banned_words=[])):
            got = loop(**off)
            assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), (name, off)
        plain = _sentences(*base)
        assert all(_repeats(s, 1) > 0 for s in plain), 'the fixtures repeat themselves'
        for n in (1, 2, 3):
            got = loop(no_repeat_ngram=n)
            sents = _sentences(*got)
            assert all(_repeats(s, n) == 0 for s in sents), (name, n, sents)
            assert sents != plain, (name, n)
            assert all(s[-1] == EOS and EOS not in s[:-1] for s in sents)
        got = loop(min_len=10)
        assert int(base[1].min()) - 2 < 10 <= int(got[1].min()) - 2, (name, base[1].tolist(), got[1].tolist())
        words = sorted({w for s in plain for w in s} - {EOS, PAD})
        got = loop(banned_words=words)
        assert not ({w for s in _sentences(*got) for w in s} & set(words)), name
        both = loop(banned_words=words, no_repeat_ngram=2, min_len=10, repetition_penalty=1.3)
        sents = _sentences(*both)
        assert all(_repeats(s, 2) == 0 and len(s) - 1 >= 10 and not (set(s) & set(words)) for s in sents), (name, sents)


@pytest.mark.parametrize('tag', ['mono', 'multi', 'wide'])
def test_repetition_penalty_on_the_oracle_step(tag, monkeypatch):
    record = []
    c, greedy, beam = _loops(monkeypatch, tag, record)
    bs, max_len, V = c['bs'], c['max_len'], c['n_words']
    th, inv = decoder.penalty_pair(1.3)
    base = greedy()
    del record[:]
    gen, ln = greedy(repetition_penalty=1.3)
    assert gen.shape != base[0].shape or not torch.equal(gen, base[0])
    open_ = _unfinished_before(gen)
    moved = 0
    for pos in range(1, gen.shape[0]):
        raw = record[pos - 1]
        s = decoder.constrain_scores_(raw.clone(), V, gen, pos, th, inv)
        moved += int((s != raw).sum())
        for b in range(bs):
            if open_[pos, b] and not (pos == max_len - 1):
                assert int(gen[pos, b]) == int(s[b].argmax()), (pos, b)
    assert moved > 0
    # seeded sampling: replayable, and its log-probabilities are those of the constrained rows
    T = 0.8
    kw = dict(sample_seed=5, sample_temperature=T, repetition_penalty=1.3, no_repeat_ngram=2, return_logprobs=True)
    state = torch.random.get_rng_state()
    del record[:]
    gen, ln, lp = greedy(**kw)
    assert len(record) == gen.shape[0] - 1
    open_ = _unfinished_before(gen)
    worst, banned_mass = 0.0, 0
    for pos in range(1, gen.shape[0]):
        s = decoder.constrain_scores_(record[pos - 1].clone(), V, gen, pos, th, inv, 2).double() / T
        banned_mass += int(torch.isinf(s).sum())
        ref = s.gather(1, gen[pos].clamp(min=0)[:, None]).squeeze(1) - torch.logsumexp(s, dim=1)
        for b in range(bs):
            forced = pos == max_len - 1 and gen[pos, b] == EOS and float(lp[pos, b]) == 0.0
            if open_[pos, b] and not forced:
                assert math.isfinite(float(ref[b])), (pos, b)                          # a banned word was never drawn
                worst = max(worst, abs(float(lp[pos, b]) - float(ref[b])))
            else:
                assert float(lp[pos, b]) == 0.0, (pos, b)
    assert worst <= 1e-5 and banned_mass > 0, (worst, banned_mass)
    assert all(_repeats(s, 2) == 0 for s in _sentences(gen, ln))
    again = greedy(**kw)
    assert all(torch.equal(u, v) for u, v in zip(again, (gen, ln, lp)))
    assert torch.equal(torch.random.get_rng_state(), state), 'the seeded path consumed torch\'s generator'
    # unseeded sampling and the nucleus take the constraints too
    torch.manual_seed(3)
    g_m, l_m = greedy(sample_temperature=0.7, no_repeat_ngram=1, min_len=5)
    assert all(_repeats(s, 1) == 0 and len(s) - 1 >= 5 for s in _sentences(g_m, l_m))
    g_p, l_p = greedy(sample_seed=5, sample_top_p=0.9, no_repeat_ngram=1, min_len=5)
    assert all(_repeats(s, 1) == 0 and len(s) - 1 >= 5 for s in _sentences(g_p, l_p))


def test_bad_constraints_raise(monkeypatch):
    c, greedy, beam = _loops(monkeypatch, 'multi')
    max_len, V = c['max_len'], c['n_words']
    for loop in (greedy, beam):
        for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.3), dict(repetition_penalty=float('inf')),
                    dict(repetition_penalty=float('nan')), dict(no_repeat_ngram=-1), dict(min_len=-1), dict(min_len=max_len - 1),
                    dict(banned_words=[V]), dict(banned_words=[-1]), dict(banned_words=[7, EOS])):
            with pytest.raises(ValueError):
                loop(**bad)
        loop(min_len=max_len - 2, banned_words=[V - 1, 0])   # the largest legal values


# ------------------------------------------------------------------------------------------------------------------ GPU
def _history(rs, n, V, ld, hist_len, alphabet):
    """generated int64 [hist_len + 2, n] inside a wider tensor (row pitch n + 2): <EOS>, the history, one <PAD> row."""
    back = torch.full((hist_len + 2, n + 2), PAD, dtype=torch.long)
    gen = back[:, :n]
    gen[0] = EOS
    if hist_len:
        words = np.asarray(alphabet)[rs.randint(0, len(alphabet), size=(hist_len, n))] if alphabet is not None else \
            np.stack([rs.permutation(V)[:hist_len] for _ in range(n)], axis=1)
        gen[1:hist_len + 1] = torch.from_numpy(words)
        if hist_len >= 3:                                    # ids outside [0, V): below 0, and inside the pitch behind V
            gen[2, 0], gen[hist_len, n - 1] = -3, V + (ld - V) // 2
    return gen


@pytest.mark.gpu
@pytest.mark.parametrize('V,ld,n', [(1000, 1024, 1), (4099, 4352, 6)])
def test_kernel_against_the_twin_bit_for_bit(V, ld, n):
    from m3p_amd import ops
    rs = np.random.RandomState(V + n)
    seven = (5, 9, 11, 20, 33, V - 1, 640)
    base = _logits(n, V, ld, seed=V + n)                    # NaN / +inf alternate behind V: the sentinel
    base[:, 5], base[:, 9], base[:, 11] = 0.0, -0.0, NEG_INF
    base[:, 20], base[:, 33] = 3.140625, -2.71875
    list3 = torch.tensor([20, 77, V - 1], dtype=torch.long)
    seen = set()
    launches = 0
    for hist_len in (0, 1, 2, 3, 255, 256, 257, 700):
        for alphabet in (seven, None):
            gen = _history(rs, n, V, ld, hist_len, alphabet)
            gen_d = torch.empty((hist_len + 2, n + 2), dtype=torch.long, device='cuda')
            gen_d[:, :n] = gen
            gen_d = gen_d[:, :n]
            cur_len = hist_len + 1
            hist = gen[1:cur_len]
            inside = (hist >= 0) & (hist < V)
            cols = torch.where(inside, hist, torch.full_like(hist, V)).t().contiguous()
            in_hist = torch.zeros((n, V + 1), dtype=torch.bool)                        # the rows' history words inside [0, V)
            in_hist.scatter_(1, cols, True)
            counts = torch.zeros((n, V + 1), dtype=torch.long)
            counts.scatter_add_(1, cols, torch.ones((n, hist_len), dtype=torch.long))
            if hist_len and int(counts[:, :V].max()) >= 3:
                seen.add('thrice')
            for ngram in (0, 1, 2, 3, 4):
                for theta in (0.5, 1.3):
                    th, inv = decoder.penalty_pair(theta)
                    for eos in (-1, EOS):
                        for banned in (None, list3):
                            what = 'V %d n %d L %d %s n-gram %d theta %g eos %d list %s' % (
                                V, n, hist_len, 'dense' if alphabet else 'sparse', ngram, theta, eos, banned is not None)
                            ref = decoder.constrain_scores_(base.clone(), V, gen, cur_len, th, inv, ngram, eos, banned)
                            # what this combination contains, from the twin alone
                            newly = (ref[:, :V] == NEG_INF) & (base[:, :V] != NEG_INF)
                            if bool((~newly.any(1)).any()):
                                seen.add('row_without_ban')
                            if bool((newly & in_hist[:, :V] & (base[:, :V] != 0)).any()):
                                seen.add('penalised_and_banned')
                            if ngram and hist_len < ngram:
                                seen.add('L<n')
                            if ngram and hist_len == ngram - 1:
                                seen.add('L==n-1')
                            if ngram and hist_len == ngram:
                                seen.add('L==n')
                            dev = base.cuda()
                            with poisoned_outputs():
                                got = ops.logits_constrain(dev, V, gen_d, cur_len, th, inv, ngram, eos,
                                                           None if banned is None else banned.cuda())
                            assert got is dev, what
                            assert_bits_equal(dev.cpu(), ref, what)
                            launches += 1
    assert seen == {'thrice', 'row_without_ban', 'penalised_and_banned', 'L<n', 'L==n-1', 'L==n'}, seen
    print('V %d ld %d n %d: %d launches equal to the twin over all %d x %d elements' % (V, ld, n, launches, n, ld))


@pytest.mark.gpu
def test_declined_shape_returns_none_and_the_loop_takes_the_twin(monkeypatch):
    from m3p_amd import ops
    V, ld, n = 1000, 1024, 2
    base = _logits(n, V, ld, seed=9)
    dev = base.cuda()
    gen = torch.full((1027, n), 5, dtype=torch.long, device='cuda')
    th, inv = decoder.penalty_pair(1.3)
    assert ops.logits_constrain(dev, V, gen, 1026, th, inv, 2) is None                 # 1025 history words
    assert_bits_equal(dev.cpu(), base, 'a declined call touched the logits')
    assert ops.logits_constrain(dev, V, gen, 1025, th, inv, 2) is dev
    assert not ops.logits_constrain_takes(n, V, ld, 1025) and ops.logits_constrain_takes(n, V, ld, 1024, 16, 4096)
    assert not ops.logits_constrain_takes(n, V, ld, 10, 17) and not ops.logits_constrain_takes(n, V, ld, 10, 2, 4097)
    # inside the loop: an n-gram order above the kernel's limit is declined by the plan; the twin edits the logits in front of
    # the selection kernel, and the result is that of the torch route
    m, c, src_enc, src_len = _hip_model('multi')
    kw = dict(max_len=c['max_len'], no_repeat_ngram=17, repetition_penalty=1.3, min_len=6)
    calls, selects = [], []
    real_c, real_s = ops.logits_constrain, ops.vocab_select
    monkeypatch.setattr(ops, 'logits_constrain', lambda *a, **k: calls.append(a[3]) or real_c(*a, **k))
    monkeypatch.setattr(ops, 'vocab_select', lambda *a, **k: selects.append(1) or real_s(*a, **k))
    with torch.no_grad():
        gen_d, len_d = m.generate(src_enc, src_len, c['tgt_lang_id'], **kw)
        plain = m.generate(src_enc, src_len, c['tgt_lang_id'], max_len=c['max_len'])
    assert not calls and selects
    assert int(len_d.min()) - 2 >= 6 and (gen_d.shape != plain[0].shape or not torch.equal(gen_d, plain[0]))
    monkeypatch.setattr(decoder, 'VOCAB_SELECT_MAX_K', 0)
    del selects[:]
    with torch.no_grad():
        gen_t, len_t = m.generate(src_enc, src_len, c['tgt_lang_id'], **kw)
    assert not selects and torch.equal(gen_t, gen_d) and torch.equal(len_t, len_d)


@pytest.mark.gpu
@pytest.mark.parametrize('tag', ['multi', 'wide'])
def test_constrained_generate_end_to_end(tag, monkeypatch):
    """Greedy, beam search, seeded sampling and seeded nucleus sampling with constraints on: the device route (the kernel in
    front of the selection kernels) against the torch route (decoder.VOCAB_SELECT_MAX_K = 0: the twin on word_scores) - tokens
    and lengths torch.equal, the sampled words' log-probabilities within lse_bar.  One ops.logits_constrain call per step with
    constraints on; none with all of them off, and then the outputs are bit for bit those of a run without the keywords."""
    from m3p_amd import ops
    m, c, src_enc, src_len = _hip_model(tag)
    max_len, T, theta = c['max_len'], 0.8, 1.3
    with torch.no_grad():
        plain = m.generate(src_enc, src_len, c['tgt_lang_id'], max_len=max_len)
    first_words = sorted(set(plain[0][1].tolist()) - {EOS, PAD})
    cons = dict(no_repeat_ngram=2, repetition_penalty=theta, min_len=6, banned_words=first_words)
    OFF = dict(min_len=0, repetition_penalty=None, no_repeat_ngram=0, banned_words=None)
    calls, amax = [], [0.0]
    real_c, real_l = ops.logits_constrain, decoder.word_logits16
    monkeypatch.setattr(ops, 'logits_constrain', lambda *a, **k: calls.append(a[3]) or real_c(*a, **k))

    def logits16(model, tensor):
        logits, V = real_l(model, tensor)
        amax[0] = max(amax[0], float(logits[:, :V].float().abs().max()))
        return logits, V
    monkeypatch.setattr(decoder, 'word_logits16', logits16)
    modes = {
        'greedy': lambda **kw: m.generate(src_enc, src_len, c['tgt_lang_id'], max_len=max_len, **kw),
        'beam': lambda **kw: m.generate_beam(src_enc, src_len, c['tgt_lang_id'], c['beam_size'], 1.0, False, max_len=max_len, **kw),
        'seeded': lambda **kw: m.generate(src_enc, src_len, c['tgt_lang_id'], max_len=max_len, sample_seed=5, sample_temperature=T,
                                          return_logprobs=True, **kw),
        'nucleus': lambda **kw: m.generate(src_enc, src_len, c['tgt_lang_id'], max_len=max_len, sample_seed=5, sample_temperature=T,
                                           sample_top_p=0.9, return_logprobs=True, **kw),
    }
    for name, run in modes.items():
        with torch.no_grad():
            del calls[:]
            base = run()
            off = run(**OFF)
            assert not calls, (name, 'a constraint launch with every constraint off')
            for u, v in zip(base, off):
                assert_bits_equal(u, v, '%s: all four off' % name)
            got = run(**cons)
            steps = got[0].shape[0] - 1 if name != 'beam' else len(calls)
            assert calls == list(range(1, steps + 1)) and steps >= 6, (name, calls)       # one call per step, at cur_len = 1, 2, ...
            sents = [[int(w) for w in got[0][1:int(got[1][b]), b]] for b in range(got[0].shape[1])]
            for s in sents:
                grams = [tuple(s[i:i + 2]) for i in range(len(s) - 1)]
                assert len(grams) == len(set(grams)) and len(s) - 1 >= 6 and not (set(s) & set(first_words)), (name, s)
            assert got[0].shape != base[0].shape or not torch.equal(got[0], base[0]), name
            with monkeypatch.context() as mp:
                mp.setattr(decoder, 'VOCAB_SELECT_MAX_K', 0)
                del calls[:]
                ref = run(**cons)
                assert not calls, (name, 'VOCAB_SELECT_MAX_K = 0 must take the twin')
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), (name, got[0].t().tolist(), ref[0].t().tolist())
        if len(got) == 3:
            bar = lse_bar(amax[0] * theta * rng.inv_temperature(T))
            err = float((got[2] - ref[2]).abs().max())
            print('%s %s: log-probabilities of the two routes differ by at most %.3g (bar %.3g)' % (tag, name, err, bar))
            assert bool(torch.isfinite(got[2]).all()) and err <= bar, (name, err, bar)
