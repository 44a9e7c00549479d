"""Prompted decoding on the host: ``generate`` / ``generate_beam`` with ``prefix`` / ``prefix_len`` (m3p_amd/decoder.py), the
loops driven by the oracle's step function (full recomputation, as tests/test_decoder.py::_oracle_backed does it) on the
models of m3p_amd.synth.decoder_case.  The reference is a prompted greedy loop written here on ref_cpu.decoder_crossfwd +
ref_cpu.word_scores, recomputed from scratch at every step; agreement is exact."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from m3p_amd import synth
from oracle import ref_cpu

EOS, PAD = synth.EOS, synth.PAD


def _oracle_backed(monkeypatch, c, sd):
    """m3p_amd.decoder's search loops with the oracle as the step function (with or without a source encoding)."""
    from m3p_amd import decoder

    def fwd(model, x, lengths, src_enc, src_len, positions, langs, cache):
        cache['slen'] = x.shape[0]
        return ref_cpu.decoder_crossfwd(sd, c['n_dec_layers'], c['n_heads'], x, lengths, src_enc, src_len, positions, langs)[-1:]

    monkeypatch.setattr(decoder, 'decoder_forward', fwd)
    monkeypatch.setattr(decoder, 'word_scores', lambda model, h: ref_cpu.word_scores(sd, h))
    return SimpleNamespace(n_words=c['n_words'], pad_index=PAD, eos_index=EOS, dim=c['emb_dim'],
                           embeddings=SimpleNamespace(weight=torch.zeros(1)))


def _prompts(c, lens, seed=5):
    """prefix (P, bs) of words in [3, n_words) and prefix_len = lens; entries behind a sentence's length are pad."""
    rs = np.random.RandomState(seed)
    P = max(lens)
    prefix = torch.from_numpy(rs.randint(3, c['n_words'], size=(P, len(lens)))).long()
    for b, n in enumerate(lens):
        prefix[n:, b] = PAD
    return prefix, torch.tensor(lens, dtype=torch.long)


def _ngram_ban(scores, hist, n):
    """-inf for every word that would complete an n-gram the history (a list of words) already holds."""
    L = len(hist)
    if n < 1 or L < n:
        return
    tail = hist[L - n + 1:]
    for j in range(L - n + 1):
        if hist[j:j + n - 1] == tail:
            scores[hist[j + n - 1]] = float('-inf')


def _prompted_greedy(sd, c, src_enc, src_len, prefix, plen, max_len, ngram=0):
    """The reference: every prompt is written into `generated` up front; at each step the batch is recomputed from scratch
    over generated[:cur_len] and a row whose prompt reaches position cur_len keeps the word that already stands there.
    -> (generated, gen_len, margins): margins[t - 1, b] is the gap between the two best scores at the step that decodes
    position t (inf for a finished sentence and for a forced word; rows before the first step are inf too)."""
    bs = prefix.shape[1]
    gen = torch.full((max_len, bs), PAD, dtype=torch.long)
    gen[0] = EOS
    for b in range(bs):
        gen[1:1 + int(plen[b]), b] = prefix[:int(plen[b]), b]
    cur = 1 + int(plen.min())
    gen_len = torch.full((bs,), cur, dtype=torch.long)
    unfinished = torch.ones(bs, dtype=torch.long)
    margins = torch.full((max_len - 1, bs), float('inf'))
    while cur < max_len:
        langs = None if c['tgt_lang_id'] is None else torch.full((cur, bs), int(c['tgt_lang_id']), dtype=torch.long)
        h = ref_cpu.decoder_crossfwd(sd, c['n_dec_layers'], c['n_heads'], gen[:cur], gen_len, src_enc, src_len, langs=langs)
        scores = ref_cpu.word_scores(sd, h[-1]).clone()
        for b in range(bs):
            _ngram_ban(scores[b], gen[1:cur, b].tolist(), ngram)
        nxt = scores.argmax(dim=1)
        top2 = scores.topk(2, dim=1)[0]
        for b in range(bs):
            if 1 + int(plen[b]) > cur:
                nxt[b] = gen[cur, b]
            elif int(unfinished[b]):
                margins[cur - 1, b] = top2[b, 0] - top2[b, 1]
        gen[cur] = nxt * unfinished + PAD * (1 - unfinished)
        gen_len += unfinished
        unfinished = unfinished * nxt.ne(EOS).long()
        cur += 1
        if int(unfinished.max()) == 0:
            break
    if cur == max_len:
        gen[-1].masked_fill_(unfinished.bool(), EOS)
    return gen[:cur], gen_len, margins[:cur - 1]


LENS = {'mono': [0, 3, 6, 1, 6], 'multi': [2, 0, 5, 5]}          # ragged, 0 and P among them


@pytest.mark.parametrize('with_src', [True, False])
@pytest.mark.parametrize('tag', sorted(LENS))
def test_prompted_greedy_equals_the_reference_loop(tag, with_src, monkeypatch):
    from m3p_amd import decoder
    c, P, sd, src_enc, src_len, x, lengths = synth.decoder_case(tag)
    if not with_src:
        src_enc = src_len = None
    stub = _oracle_backed(monkeypatch, c, sd)
    prefix, plen = _prompts(c, LENS[tag])
    gen, gen_len = decoder.generate(stub, src_enc, src_len, c['tgt_lang_id'], max_len=c['max_len'], prefix=prefix, prefix_len=plen)
    ref, ref_len, _ = _prompted_greedy(sd, c, src_enc, src_len, prefix, plen, c['max_len'])
    assert torch.equal(gen, ref) and torch.equal(gen_len, ref_len)
    for b, n in enumerate(LENS[tag]):
        assert gen[0, b] == EOS and torch.equal(gen[1:1 + n, b], prefix[:n, b])
        assert int((gen[:, b] == EOS).sum()) == 2 and gen[int(gen_len[b]) - 1, b] == EOS
        assert int(gen_len[b]) >= n + 2


def test_a_zero_length_prefix_without_a_source_gives_the_batch_size(monkeypatch):
    """Unprompted generation from the language model: the (0, bs) prefix only says how many sentences to decode."""
    from m3p_amd import decoder
    c, P, sd, _, _, x, lengths = synth.decoder_case('mono')
    stub = _oracle_backed(monkeypatch, c, sd)
    prefix, plen = torch.zeros((0, 3), dtype=torch.long), torch.zeros(3, dtype=torch.long)
    gen, gen_len = decoder.generate(stub, None, None, None, max_len=c['max_len'], prefix=prefix, prefix_len=plen)
    ref, ref_len, _ = _prompted_greedy(sd, c, None, None, prefix, plen, c['max_len'])
    assert gen.shape[1] == 3 and torch.equal(gen, ref) and torch.equal(gen_len, ref_len)


def test_argument_errors(monkeypatch):
    from m3p_amd import decoder
    c, P, sd, src_enc, src_len, x, lengths = synth.decoder_case('multi')
    stub = _oracle_backed(monkeypatch, c, sd)
    prefix, plen = _prompts(c, [2, 0, 5, 5])
    gen = lambda **kw: decoder.generate(stub, src_enc, src_len, c['tgt_lang_id'], max_len=c['max_len'], **kw)      # noqa: E731
    beam = lambda **kw: decoder.generate_beam(stub, src_enc, src_len, c['tgt_lang_id'], 3, 1.0, False,             # noqa: E731
                                              max_len=c['max_len'], **kw)
    for call in (gen, beam):
        bad = prefix.clone()
        bad[1, 2] = EOS
        with pytest.raises(ValueError, match='EOS'):
            call(prefix=bad, prefix_len=torch.full((4,), 5))
        bad[1, 2] = c['n_words']
        with pytest.raises(ValueError):
            call(prefix=bad, prefix_len=torch.full((4,), 5))
        long_prefix, long_len = _prompts(c, [c['max_len'] - 1] * 4)          # 1 + 13 > max_len - 1 = 13
        with pytest.raises(ValueError, match='too long'):
            call(prefix=long_prefix, prefix_len=long_len)
        full_prefix, full_len = _prompts(c, [c['max_len'] - 2] * 4)          # the longest allowed: only the forced <EOS> follows
        out = call(prefix=full_prefix, prefix_len=full_len)
        assert int(out[1].max()) == c['max_len'] and bool((out[0][1:-1].reshape(c['max_len'] - 2, -1)[:, 0] == full_prefix[:, 0]).all())
        with pytest.raises(ValueError):
            call(prefix=prefix, prefix_len=torch.tensor([2, 0, 6, 5]))      # beyond P
    # a word behind a sentence's length may be anything
    ok = prefix.clone()
    ok[4, 0] = EOS
    gen(prefix=ok, prefix_len=plen)
    with pytest.raises(ValueError, match='equal'):
        beam(prefix=prefix, prefix_len=plen)
    with pytest.raises(ValueError, match='needs a prefix'):
        decoder.generate(stub, None, None, c['tgt_lang_id'], max_len=c['max_len'])
    with pytest.raises(ValueError, match='needs a prefix'):
        decoder.generate_beam(stub, None, None, c['tgt_lang_id'], 3, 1.0, False, max_len=c['max_len'])


@pytest.mark.parametrize('tag', ['mono', 'multi'])
def test_a_zero_length_prefix_with_a_source_changes_nothing(tag, monkeypatch):
    from m3p_amd import decoder
    c, P, sd, src_enc, src_len, x, lengths = synth.decoder_case(tag)
    stub = _oracle_backed(monkeypatch, c, sd)
    bs = c['bs']
    empty = dict(prefix=torch.zeros((0, bs), dtype=torch.long), prefix_len=torch.zeros(bs, dtype=torch.long))
    for kw in (dict(), dict(sample_seed=9, sample_temperature=0.8, sample_top_k=5, return_logprobs=True)):
        a = decoder.generate(stub, src_enc, src_len, c['tgt_lang_id'], max_len=c['max_len'], **kw)
        b = decoder.generate(stub, src_enc, src_len, c['tgt_lang_id'], max_len=c['max_len'], **kw, **empty)
        assert len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))
    if c['beam_size']:
        a = decoder.generate_beam(stub, src_enc, src_len, c['tgt_lang_id'], c['beam_size'], 1.0, False, max_len=c['max_len'],
                                  n_best=2, return_scores=True)
        b = decoder.generate_beam(stub, src_enc, src_len, c['tgt_lang_id'], c['beam_size'], 1.0, False, max_len=c['max_len'],
                                  n_best=2, return_scores=True, **empty)
        assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_log_probabilities_are_zero_at_forced_positions(monkeypatch):
    from m3p_amd import decoder
    c, P, sd, src_enc, src_len, x, lengths = synth.decoder_case('mono')
    stub = _oracle_backed(monkeypatch, c, sd)
    lens = LENS['mono']
    prefix, plen = _prompts(c, lens)
    gen, gen_len, lp = decoder.generate(stub, src_enc, src_len, None, max_len=c['max_len'], sample_seed=3, sample_temperature=0.9,
                                        return_logprobs=True, prefix=prefix, prefix_len=plen)
    assert lp.shape == gen.shape
    drawn = 0
    for b, n in enumerate(lens):
        assert torch.equal(gen[1:1 + n, b], prefix[:n, b])
        assert bool((lp[:1 + n, b] == 0).all())
        own = lp[1 + n:int(gen_len[b]) - 1, b]               # the words the sentence drew (its last <EOS> may have been forced)
        assert bool((own < 0).all()), (b, own)
        drawn += own.numel()
        assert bool((lp[int(gen_len[b]) - 1:, b] <= 0).all()) and bool((lp[int(gen_len[b]):, b] == 0).all())
    assert drawn > 0
    # the same seed without the prompts draws from the same streams: a sentence with an empty prompt next to longer ones is
    # still the batch's row 0 at every step
    again = decoder.generate(stub, src_enc, src_len, None, max_len=c['max_len'], sample_seed=3, sample_temperature=0.9,
                             return_logprobs=True, prefix=prefix, prefix_len=plen)
    assert all(torch.equal(u, v) for u, v in zip(again, (gen, gen_len, lp)))


def test_no_repeat_ngram_sees_the_prefix(monkeypatch):
    """A word `b` with a huge output bias is what every unconstrained step picks.  Behind the prompt a b a, no_repeat_ngram = 2
    must ban b - the bigram a b stands in the PROMPT - and the loop must equal the reference with the same ban."""
    from m3p_amd import decoder
    c, P, sd, src_enc, src_len, x, lengths = synth.decoder_case('mono')
    a, b = 17, 23
    sd = dict(sd)
    sd['pred_layer.proj.bias'] = sd['pred_layer.proj.bias'].clone()
    sd['pred_layer.proj.bias'][b] += 100.0
    stub = _oracle_backed(monkeypatch, c, sd)
    bs = c['bs']
    prefix = torch.tensor([a, b, a], dtype=torch.long)[:, None].expand(3, bs).contiguous()
    plen = torch.full((bs,), 3, dtype=torch.long)
    free, _ = decoder.generate(stub, src_enc, src_len, None, max_len=c['max_len'], prefix=prefix, prefix_len=plen)
    assert bool((free[4] == b).all())
    gen, gen_len = decoder.generate(stub, src_enc, src_len, None, max_len=c['max_len'], prefix=prefix, prefix_len=plen, no_repeat_ngram=2)
    assert bool((gen[4] != b).all())
    ref, ref_len, _ = _prompted_greedy(sd, c, src_enc, src_len, prefix, plen, c['max_len'], ngram=2)
    assert torch.equal(gen, ref) and torch.equal(gen_len, ref_len)
    for s in range(bs):                                                  # no bigram twice, prompt included
        words = gen[1:int(gen_len[s]) - 1, s].tolist()
        grams = list(zip(words, words[1:]))
        assert len(grams) == len(set(grams)), (s, words)
    # min_len counts prefix words: with min_len = 4 the first free position (4) may not end the sentence, the next one may
    eos_sd = dict(sd)
    eos_sd['pred_layer.proj.bias'] = sd['pred_layer.proj.bias'].clone()
    eos_sd['pred_layer.proj.bias'][EOS] += 200.0
    stub = _oracle_backed(monkeypatch, c, eos_sd)
    gen, gen_len = decoder.generate(stub, src_enc, src_len, None, max_len=c['max_len'], prefix=prefix, prefix_len=plen, min_len=4)
    assert bool((gen[4] == b).all()) and bool((gen[5] == EOS).all()) and bool((gen_len == 6).all())


def _teacher_forced_score(sd64, c, src_enc, src_len_b, tokens, n_forced, length_penalty):
    """Sum of the fp64 log-probabilities of tokens[1 + n_forced:] given what precedes them, over (len - 1) ** penalty."""
    T = tokens.numel()
    x = tokens[:T - 1, None]
    langs = None if c['tgt_lang_id'] is None else torch.full((T - 1, 1), int(c['tgt_lang_id']), dtype=torch.long)
    h = ref_cpu.decoder_crossfwd(sd64, c['n_dec_layers'], c['n_heads'], x, torch.tensor([T - 1]), src_enc, src_len_b, langs=langs)
    logp = torch.log_softmax(ref_cpu.word_scores(sd64, h[:, 0]), dim=-1)             # row p scores position p + 1
    total = sum(float(logp[p - 1, int(tokens[p])]) for p in range(1 + n_forced, T))
    return total / float(T - 1) ** length_penalty


@pytest.mark.parametrize('with_src', [True, False])
@pytest.mark.parametrize('tag', ['multi', 'wide'])
def test_prompted_beam_search(tag, with_src, monkeypatch):
    from m3p_amd import decoder
    c, P, sd, src_enc, src_len, x, lengths = synth.decoder_case(tag)
    if not with_src:
        src_enc = src_len = None
    stub = _oracle_backed(monkeypatch, c, sd)
    bs, beam, n_forced, max_len, lp = c['bs'], c['beam_size'], 3, 24, 0.8
    prefix, plen = _prompts(c, [n_forced] * bs)
    dec, tl, scores = decoder.generate_beam(stub, src_enc, src_len, c['tgt_lang_id'], beam, lp, False, max_len=max_len, n_best=beam,
                                            return_scores=True, prefix=prefix, prefix_len=plen)
    assert dec.shape[1:] == (bs, beam) and tl.shape == (bs, beam) and scores.dtype == torch.float64
    # (the recomputation below needs hypotheses that ended on a word they chose: the last step replaces its word by <EOS>)
    assert int(tl.max()) < max_len
    sd64 = {k: v.double() for k, v in sd.items()}
    for s in range(bs):
        for j in range(beam):
            n = int(tl[s, j])
            hyp = dec[:n, s, j]
            assert hyp[0] == EOS and hyp[n - 1] == EOS and int((hyp == EOS).sum()) == 2 and n >= n_forced + 2
            assert torch.equal(hyp[1:1 + n_forced], prefix[:, s]), (s, j, hyp.tolist())
            ref = _teacher_forced_score(sd64, c, None if src_enc is None else src_enc[s:s + 1].double(),
                                        None if src_len is None else src_len[s:s + 1], hyp, n_forced, lp)
            assert abs(float(scores[s, j]) - ref) < 1e-5, (s, j, float(scores[s, j]), ref)
        assert bool((scores[s, :-1] >= scores[s, 1:]).all())
    # one beam is prompted greedy decoding
    dec1, tl1 = decoder.generate_beam(stub, src_enc, src_len, c['tgt_lang_id'], 1, lp, False, max_len=max_len, prefix=prefix,
                                      prefix_len=plen)
    gen, gen_len = decoder.generate(stub, src_enc, src_len, c['tgt_lang_id'], max_len=max_len, prefix=prefix, prefix_len=plen)
    assert torch.equal(tl1, gen_len)
    for s in range(bs):
        assert torch.equal(dec1[:int(tl1[s]), s], gen[:int(gen_len[s]), s])
