"""decoder.beam_advance_host - the hypothesis bookkeeping of a beam-search step as one function over plain arrays - against the
loop it replaces, kept here word for word over the untouched decoder.BeamHypotheses class, on candidate streams made without
a model.  After EVERY step: the next beams (score bits, words, rows), the done flags and every sentence's list of finished
hypotheses as (score, arrival, tokens).  Seeded random streams over beam x length_penalty x early_stopping, and hand-made ones:
<EOS> at rank 0, <EOS> at every second rank, equal fp32 sums at equal length (arrival decides, the strict > does not evict), a
sentence that finishes at step 2 while its neighbours run on, the cur_len + 1 == max_len step.  Then the n_best /
return_scores argument checks of generate_beam.  tests/test_beam_advance.py runs the same streams through the kernel."""
import numpy as np
import pytest
import torch

from m3p_amd import decoder

EOS, PAD = 1, 2


# --------------------------------------------------------------------------------------------------------- candidate streams
def candidates(rs, beam_scores, bs, beam, V, eos_ranks=None, equal=None):
    """One step's candidates, (scores fp32 [bs, 2 beam] descending, flat_idx int64 [bs, 2 beam]): per sentence 2 * beam DISTINCT
    (beam, word) entries - so at most one <EOS> per beam, as a real selection gives - with <EOS> entries four times as likely
    as any other.  eos_ranks(s) -> the ranks that hold an <EOS> (None: random); equal(s) -> one value for every rank (None:
    a descending random walk below the sentence's best beam score)."""
    k = 2 * beam
    sc = np.empty((bs, k), dtype=np.float32)
    idx = np.empty((bs, k), dtype=np.int64)
    flat = np.arange(beam * V)
    is_eos = flat % V == EOS
    for s in range(bs):
        ranks = None if eos_ranks is None else eos_ranks(s)
        if ranks is None:
            w = np.where(is_eos, 4.0, 1.0)
            idx[s] = rs.choice(flat, size=k, replace=False, p=w / w.sum())
        else:
            ranks = sorted(ranks)
            assert len(ranks) <= beam
            idx[s] = rs.choice(flat[~is_eos], size=k, replace=False)
            idx[s, ranks] = rs.permutation(beam)[:len(ranks)] * V + EOS
        top = float(beam_scores[s * beam:(s + 1) * beam].max())
        value = None if equal is None else equal(s)
        if value is None:
            sc[s] = np.sort((top - rs.exponential(1.0, size=k)).astype(np.float32))[::-1]
        else:
            sc[s] = np.float32(value)
    return sc, idx


class Case:
    def __init__(self, name, beam, length_penalty, early_stopping, bs=3, V=11, max_len=6, seed=0, eos_ranks=None, equal=None):
        self.name, self.beam, self.lp, self.es = name, beam, length_penalty, early_stopping
        self.bs, self.V, self.max_len, self.seed = bs, V, max_len, seed
        self.eos_ranks, self.equal = eos_ranks, equal              # (cur_len, sentence) -> ranks / value, or None

    def __repr__(self):
        return self.name


def random_cases(beams=(1, 2, 3, 16), max_len=6):
    return [Case('random-beam%d-lp%g-es%d-len%d' % (beam, lp, es, max_len), beam, lp, es, max_len=max_len,
                 seed=1000 * beam + int(10 * lp) + es)
            for beam in beams for lp in (0, 0.6, 1, 2) for es in (False, True)]


def hand_made_cases():
    out = []
    for beam in (2, 3):
        for es in (False, True):
            tag = 'beam%d-es%d' % (beam, es)
            out.append(Case('eos-at-rank-0-' + tag, beam, 1.0, es, seed=11, eos_ranks=lambda cur, s: [0] if cur >= 2 else []))
            out.append(Case('eos-at-every-second-rank-' + tag, beam, 0.6, es, seed=12,
                            eos_ranks=lambda cur, s, beam=beam: list(range(0, 2 * beam, 2)) if cur >= 2 else []))
            # equal sums: with length_penalty 0 one <EOS> at step 2 and `beam` at step 3, all of one value, are one more than
            # the list holds; and at equal length the last step, where all 2 * beam candidates are offered, brings twice as many
            out.append(Case('equal-sums-' + tag, beam, 0.0, es, seed=13, equal=lambda cur, s: -2.5,
                            eos_ranks=lambda cur, s, beam=beam: [0] if cur == 2 else list(range(beam)) if cur == 3 else []))
            out.append(Case('equal-sums-last-step-' + tag, beam, 1.0, es, seed=14, max_len=4,
                            equal=lambda cur, s: -1.25 if cur == 3 else None, eos_ranks=lambda cur, s: []))
            # sentence 1 fills its list at step 2 (sums of -0.5) and is done from step 3 on, where its best candidate has -50;
            # sentences 0 and 2 see no <EOS> before the last step
            out.append(Case('one-sentence-finishes-at-step-2-' + tag, beam, 1.0, es, seed=15,
                            equal=lambda cur, s: None if s != 1 or cur < 2 else -0.5 if cur == 2 else -50.0,
                            eos_ranks=lambda cur, s, beam=beam: list(range(beam)) if (s == 1 and cur == 2) else []))
    out.append(Case('last-step-only', 3, 1.0, False, max_len=2, seed=16))
    return out


# ------------------------------------------------------------------------------------------------------ the two book-keepers
class ClassLoop:
    """The per-step loop of generate_beam as it stood before beam_advance_host, over decoder.BeamHypotheses."""

    def __init__(self, c):
        self.c = c
        self.hyps = [decoder.BeamHypotheses(c.beam, c.max_len, c.lp, c.es) for _ in range(c.bs)]
        self.done = [False] * c.bs

    def step(self, next_scores, next_words, generated, cur_len):
        c, hyps, done = self.c, self.hyps, self.done
        bs, beam_size, n_words, max_len = c.bs, c.beam, c.V, c.max_len
        next_scores_h, next_words_h = torch.from_numpy(next_scores).tolist(), torch.from_numpy(next_words).tolist()
        next_batch_beam = []
        for sent in range(bs):
            done[sent] = done[sent] or hyps[sent].is_done(max(next_scores_h[sent]))
            if done[sent]:
                next_batch_beam.extend([(0, PAD, 0)] * beam_size)
                continue
            next_sent_beam = []
            for idx, value in zip(next_words_h[sent], next_scores_h[sent]):
                beam_id, word_id = idx // n_words, idx % n_words
                if word_id == EOS or cur_len + 1 == max_len:
                    hyps[sent].add(generated[:cur_len, sent * beam_size + beam_id].copy(), value)
                else:
                    next_sent_beam.append((value, word_id, sent * beam_size + beam_id))
                if len(next_sent_beam) == beam_size:
                    break
            assert len(next_sent_beam) == (0 if cur_len + 1 == max_len else beam_size)
            if len(next_sent_beam) == 0:
                next_sent_beam = [(0, PAD, 0)] * beam_size
            next_batch_beam.extend(next_sent_beam)
        return (np.array([v[0] for v in next_batch_beam], dtype=np.float32), np.array([v[1] for v in next_batch_beam], dtype=np.int64),
                np.array([v[2] for v in next_batch_beam], dtype=np.int64))

    def lists(self):
        return [sorted((float(sc), arr, tok.tolist()) for sc, arr, tok in hp._heap) for hp in self.hyps]

    def dones(self):
        return [bool(d) for d in self.done]


def state_lists(state):
    """A hypothesis state (NumPy) as ClassLoop.lists gives it: per sentence [(score, arrival, tokens)], sorted."""
    out = []
    for s in range(state['hyp_count'].shape[0]):
        out.append(sorted((float(state['hyp_score'][s, j]), int(state['hyp_arrival'][s, j]),
                           state['hyp_tok'][s, j, :int(state['hyp_len'][s, j])].tolist()) for j in range(int(state['hyp_count'][s]))))
    return out


class Twin:
    def __init__(self, c):
        self.c = c
        self.state = decoder.beam_state_host(c.bs, c.beam, c.max_len, PAD)
        self.norm, self.norm_max = decoder.beam_norms(c.max_len, c.lp)

    def step(self, next_scores, next_words, generated, cur_len):
        c = self.c
        return decoder.beam_advance_host(next_scores, next_words, generated, self.state, cur_len, c.max_len, EOS, PAD, c.V, c.beam,
                                         c.es, self.norm, self.norm_max)

    def lists(self):
        return state_lists(self.state)

    def dones(self):
        return [bool(d) for d in self.state['done']]


def drive(c, first, second, after_step=None):
    """Run one candidate stream through two book-keepers and compare them after every step.  -> the steps run."""
    rs = np.random.RandomState(c.seed)
    n = c.bs * c.beam
    generated = np.full((c.max_len, n), PAD, dtype=np.int64)
    generated[0] = EOS
    beam_scores = np.zeros((c.bs, c.beam), dtype=np.float32)
    beam_scores[:, 1:] = -1e9
    beam_scores = beam_scores.reshape(-1)
    steps = 0
    for cur_len in range(1, c.max_len):
        sc, idx = candidates(rs, beam_scores, c.bs, c.beam, c.V,
                             None if c.eos_ranks is None else (lambda s: c.eos_ranks(cur_len, s)),
                             None if c.equal is None else (lambda s: c.equal(cur_len, s)))
        a = first.step(sc, idx, generated, cur_len)
        b = second.step(sc, idx, generated, cur_len)
        where = (c.name, 'step', cur_len)
        assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)), where + ('beam_scores',)
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), where + ('beam_words / beam_idx',)
        assert first.dones() == second.dones(), where + ('done', first.dones(), second.dones())
        assert first.lists() == second.lists(), where + ('lists',)
        beam_scores, words, rows = a
        nxt = generated[:, rows]
        nxt[cur_len] = words
        if after_step is not None:
            after_step(cur_len, sc, idx, generated, nxt, a)
        generated = nxt
        steps += 1
        if all(first.dones()):
            break
    return steps


# ----------------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize('c', random_cases(), ids=repr)
def test_random_streams_equal_the_class_loop(c):
    twin = Twin(c)
    drive(c, ClassLoop(c), twin)
    assert not twin.state['status'].any()


@pytest.mark.parametrize('c', hand_made_cases(), ids=repr)
def test_hand_made_streams_equal_the_class_loop(c):
    twin = Twin(c)
    steps = drive(c, ClassLoop(c), twin)
    st = twin.state
    assert not st['status'].any()
    if c.name.startswith('one-sentence-finishes-at-step-2'):
        assert steps == c.max_len - 1
        assert int(st['hyp_len'][1].max()) == 2 and int(st['hyp_count'][1]) == c.beam           # frozen since step 2 ...
        assert int(st['hyp_len'][0].max()) == c.max_len - 1                                     # ... while the neighbours ran on
    if c.name.startswith('equal-sums'):
        # the list holds the FIRST arrivals: nothing of an equal score evicted them
        for s in range(c.bs):
            assert len(set(st['hyp_score'][s].tolist())) == 1
            assert sorted(st['hyp_arrival'][s].tolist()) == list(range(c.beam))
        assert int(st['arrivals'].min()) > c.beam


def test_the_streams_cover_what_they_are_for():
    """Fixture sanity over the random cases: some list evicts an entry, and some sentence is done before the last step without
    early stopping.  (A full list that refuses an offer is what the equal-sums cases assert.)"""
    evicted = done_early = 0
    for c in random_cases():
        twin = Twin(c)
        before = {}

        def watch(cur_len, sc, idx, generated, nxt, out, twin=twin, before=before, c=c):
            nonlocal evicted, done_early
            st = twin.state
            for s in range(c.bs):
                arr = sorted(st['hyp_arrival'][s, :int(st['hyp_count'][s])].tolist())
                evicted += len(before.get(s, [])) == c.beam and arr != before[s]
                before[s] = arr
            done_early += (not c.es) and cur_len + 1 < c.max_len and bool(st['done'].any())
        drive(c, ClassLoop(c), twin, watch)
    assert evicted and done_early, (evicted, done_early)


def test_too_few_continuations_set_status():
    """More <EOS> candidates than a real selection can give (one beam's <EOS> twice): fewer than `beam` continuations."""
    beam, V, max_len = 2, 11, 6
    st = decoder.beam_state_host(1, beam, max_len, PAD)
    norm, norm_max = decoder.beam_norms(max_len, 1.0)
    gen = np.full((max_len, beam), PAD, dtype=np.int64)
    gen[0] = EOS
    sc = np.array([[-1, -2, -3, -4]], dtype=np.float32)
    idx = np.array([[EOS, V + EOS, EOS, 5]], dtype=np.int64)
    out = decoder.beam_advance_host(sc, idx, gen, st, 1, max_len, EOS, PAD, V, beam, False, norm, norm_max)
    assert st['status'].tolist() == [1]
    assert out[0].tolist() == [-4.0, 0.0] and out[1].tolist() == [5, PAD] and out[2].tolist() == [0, 0]
    assert int(st['hyp_count'][0]) == 2 and int(st['arrivals'][0]) == 3


def test_result_orders_by_score_then_arrival():
    st = decoder.beam_state_host(1, 3, 5, PAD)
    st['hyp_count'][0] = 3
    st['hyp_score'][0] = [-1.0, -0.5, -1.0]
    st['hyp_arrival'][0] = [4, 2, 1]
    st['hyp_len'][0] = [2, 3, 1]
    st['hyp_tok'][0, 0, :2] = [EOS, 7]
    st['hyp_tok'][0, 1, :3] = [EOS, 8, 9]
    st['hyp_tok'][0, 2, :1] = [EOS]
    dec, tl, sc = decoder._beam_result(st, 3, True, EOS, PAD, torch.device('cpu'))
    assert dec.shape == (4, 1, 3) and dec.dtype == torch.int64 and sc.dtype == torch.float64 and tl.shape == (1, 3)
    assert dec[:, 0, 0].tolist() == [EOS, 8, 9, EOS] and dec[:, 0, 1].tolist() == [EOS, EOS, PAD, PAD]
    assert dec[:, 0, 2].tolist() == [EOS, 7, EOS, PAD]
    assert tl.tolist() == [[4, 2, 3]] and sc.tolist() == [[-0.5, -1.0, -1.0]]
    dec1, tl1 = decoder._beam_result(st, 1, False, EOS, PAD, torch.device('cpu'))
    assert dec1.shape == (4, 1) and torch.equal(dec1, dec[:, :, 0]) and tl1.tolist() == [4]
    st['status'][0] = 1
    from m3p_amd import lib as L
    with pytest.raises(L.M3PError):
        decoder._beam_result(st, 1, False, EOS, PAD, torch.device('cpu'))


@pytest.mark.parametrize('n_best', [0, -1, 4, 2.0, True, None])
def test_n_best_outside_its_range_raises(n_best):
    from types import SimpleNamespace
    model = SimpleNamespace(n_words=11, embeddings=SimpleNamespace(weight=torch.zeros(1)), eos_index=EOS, pad_index=PAD)
    with pytest.raises(ValueError):
        decoder.generate_beam(model, torch.zeros(2, 3, 4), torch.tensor([3, 3]), None, 3, 1.0, False, max_len=5, n_best=n_best)


def test_generate_beam_keywords_and_defaults():
    import inspect
    from m3p_amd.model.transformer import TransformerModel
    for fn in (decoder.generate_beam, TransformerModel.generate_beam):
        p = inspect.signature(fn).parameters
        assert p['n_best'].default == 1 and p['return_scores'].default is False
    assert decoder.BEAM_HYPS_ON_DEVICE in (True, False)
