"""Prompted decoding on the device: the prefill call of ``decoder_forward`` (several new positions over a cache: the tiled
prefix kernel from decoder.PREFILL_TILED_MIN_T on, the rows kernel below it and with the route switched off), and
``generate`` / ``generate_beam`` with ``prefix`` / ``prefix_len`` on a 2-layer, 128-d, V = 1000 model without an <EOS> ramp.

The reference is the prompted greedy loop of tests/test_generate_prefix_cpu.py on the fp32 oracle, computed once per set of
prompt lengths.  Tokens are compared by the near-tie rule of tests/test_decoder.py (tol = 0.02 on the oracle's own top-2
margin; a host test checks that the fixture holds sentences without one).  Without the ramp no sentence ends before
max_len, which is chosen a few free steps behind the longest prompt."""
import functools

import numpy as np
import pytest
import torch

from m3p_amd import rng, synth
from oracle import ref_cpu
from tests.test_decoder import _agree_until_near_tie
from tests.test_generate_prefix_cpu import _prompted_greedy, _prompts
from tests.test_vocab_sample import KEY_ATOL
from tests.util import GLOBAL_GEMM, rel_l2

EOS, PAD = synth.EOS, synth.PAD
C = dict(emb_dim=128, n_heads=4, n_dec_layers=2, n_words=1000, tgt_lang_id=None, bs=3, S=12, seed=83, prompt_seed=86)
EQUAL, RAGGED = (70, 70, 70), (5, 70, 130)
MAX_LEN = {EQUAL: 80, RAGGED: 140}
ROUTES = ['tiled', 'rows']


@functools.lru_cache(maxsize=None)
def _weights():
    P = synth.model_params(C['emb_dim'], C['n_heads'], 1, C['n_words'], n_dec_layers=C['n_dec_layers'])
    sd = synth.golden_state_dict(synth.decoder_param_shapes(P), seed=C['seed'], scale=0.05)
    rs = np.random.RandomState(C['seed'] + 1)
    src_enc = torch.from_numpy(rs.standard_normal((C['bs'], C['S'], C['emb_dim'])).astype(np.float32))
    src_len = torch.tensor([C['S'], 7, 10])
    return P, sd, src_enc, src_len


@functools.lru_cache(maxsize=None)
def _model():
    from m3p_amd.model.transformer import TransformerModel
    P, sd, src_enc, src_len = _weights()
    torch.manual_seed(0)
    m = TransformerModel(P, is_encoder=False, with_output=True, is_crossModal=True).cuda()
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected
    m.eval()
    return m, src_enc.cuda(), src_len.cuda()


@functools.lru_cache(maxsize=None)
def _reference(lens, with_src=True):
    """(prefix, prefix_len, generated, gen_len, margins) of the CPU loop - computed once and left unchanged."""
    P, sd, src_enc, src_len = _weights()
    prefix, plen = _prompts(C, list(lens), seed=C['prompt_seed'])
    if not with_src:
        src_enc = src_len = None
    return (prefix, plen) + _prompted_greedy(sd, C, src_enc, src_len, prefix, plen, MAX_LEN[lens])


def _route(monkeypatch, route):
    """Switches the tiled prefill off for 'rows'; -> the list every ops.attn_prefix_fwd call's (Tq, pos0) is appended to."""
    from m3p_amd import decoder, ops
    assert decoder.PREFILL_TILED_MIN_T == 0 or 8 <= decoder.PREFILL_TILED_MIN_T <= 64
    if route == 'rows':
        monkeypatch.setattr(decoder, 'PREFILL_TILED_MIN_T', 0)
    calls, real = [], ops.attn_prefix_fwd

    def spy(q, kv, B, Tq, H, dh, pos0, out=None):
        res = real(q, kv, B, Tq, H, dh, pos0, out=out)
        assert res is not None
        calls.append((Tq, pos0))
        return res
    monkeypatch.setattr(ops, 'attn_prefix_fwd', spy)
    return calls


def test_the_fixture_has_a_sentence_without_a_near_tie():
    """(no device needed) For each set of prompt lengths at least one sentence's free steps all have a top-2 margin >= 0.02."""
    for lens in (EQUAL, RAGGED):
        for with_src in (True, False):
            prefix, plen, gen, gen_len, margins = _reference(lens, with_src)
            assert gen.shape[0] == MAX_LEN[lens]
            exact = [b for b in range(C['bs']) if float(margins[:, b].min()) >= 0.02]
            assert exact, (lens, with_src, margins.min(0)[0].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('with_src', [True, False], ids=['seq2seq', 'lm'])
def test_prefill_call_vs_reference_and_step_by_step_cache(with_src, route, monkeypatch):
    from m3p_amd import decoder
    m, src_enc, src_len = _model()
    P, sd, src_enc_h, src_len_h = _weights()
    if not with_src:
        src_enc = src_len = src_enc_h = src_len_h = None
    T, bs, d = 71, C['bs'], C['emb_dim']
    prefix, plen, _, _, _ = _reference(EQUAL)
    x = torch.cat([torch.full((1, bs), EOS, dtype=torch.long), prefix[:70]]).cuda()
    lengths = torch.full((bs,), T, dtype=torch.long).cuda()
    calls = _route(monkeypatch, route)
    with torch.no_grad():
        cache = {'slen': 0, 'max_len': 80, 'tiled_prefill': True}
        full = decoder.decoder_forward(m, x, lengths, src_enc, src_len, cache=cache)
        assert calls == ([(T, 0)] * C['n_dec_layers'] if route == 'tiled' else [])
        steps = {'slen': 0, 'max_len': 80, 'tiled_prefill': True}
        pieces = [decoder.decoder_forward(m, x[:t], lengths.clamp(max=t), src_enc, src_len, cache=steps) for t in range(1, T + 1)]
    assert full.shape == (T, bs, d) and cache['slen'] == steps['slen'] == T
    ref = ref_cpu.decoder_crossfwd(sd, C['n_dec_layers'], C['n_heads'], x.cpu(), lengths.cpu(), src_enc_h, src_len_h)
    inc = torch.cat(pieces, 0)
    figures = dict(full=rel_l2(full.float().cpu(), ref), inc=rel_l2(inc.float().cpu(), ref), both=rel_l2(inc.float(), full.float()))
    print(route, figures)
    assert figures['full'] < 2e-2 and figures['inc'] < 2e-2 and figures['both'] < 5e-3, figures
    for i in range(C['n_dec_layers']):
        a, b = cache[('self', i)][:, :T].float(), steps[('self', i)][:, :T].float()
        assert bool(torch.isfinite(a).all()) and rel_l2(a, b) < GLOBAL_GEMM, (i, rel_l2(a, b))
        if with_src:
            assert rel_l2(cache[('cross', i)].float(), steps[('cross', i)].float()) < GLOBAL_GEMM


def _check_greedy(gen, gen_len, lens, with_src=True):
    prefix, plen, ref, ref_len, margins = _reference(lens, with_src)
    g, gl = gen.cpu().numpy(), gen_len.cpu().numpy()
    assert g.shape[1] == C['bs'] and (g[0] == EOS).all() and ((g == EOS).sum(0) == 2).all()
    for b, n in enumerate(lens):
        assert np.array_equal(g[1:1 + n, b], prefix[:n, b].numpy()), 'the prompt of sentence %d is not reproduced' % b
        assert g[gl[b] - 1, b] == EOS and (g[gl[b]:, b] == PAD).all() and gl[b] >= n + 2
    _agree_until_near_tie(g, ref.numpy(), margins.numpy(), tol=0.02)
    exact = [b for b in range(C['bs']) if float(margins[:, b].min()) >= 0.02]
    assert exact
    for b in exact:
        assert gl[b] == int(ref_len[b]) and np.array_equal(g[:gl[b], b], ref[:int(ref_len[b]), b].numpy())


@pytest.mark.gpu
@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('lens', [EQUAL, RAGGED], ids=['equal', 'ragged'])
def test_prompted_greedy_vs_the_cpu_loop(lens, route, monkeypatch):
    from m3p_amd import decoder
    m, src_enc, src_len = _model()
    prefix, plen = _reference(lens)[:2]
    calls = _route(monkeypatch, route)
    first = 1 + min(lens)
    tiled = route == 'tiled' and first >= decoder.PREFILL_TILED_MIN_T
    for select in (True, False):                       # ops.vocab_select, then the torch route
        del calls[:]
        if not select:
            monkeypatch.setattr(decoder, 'VOCAB_SELECT_MAX_K', 0)
        with torch.no_grad():
            gen, gen_len = m.generate(src_enc, src_len, None, max_len=MAX_LEN[lens], prefix=prefix.cuda(), prefix_len=plen.cuda())
        assert calls == ([(first, 0)] * C['n_dec_layers'] if tiled else []), calls
        _check_greedy(gen, gen_len, lens)


@pytest.mark.gpu
@pytest.mark.parametrize('route', ROUTES)
def test_prompted_greedy_without_a_source(route, monkeypatch):
    m, _, _ = _model()
    prefix, plen = _reference(EQUAL, False)[:2]
    _route(monkeypatch, route)
    with torch.no_grad():
        gen, gen_len = m.generate(None, None, None, max_len=MAX_LEN[EQUAL], prefix=prefix.cuda(), prefix_len=plen.cuda())
    _check_greedy(gen, gen_len, EQUAL, with_src=False)


@pytest.mark.gpu
@pytest.mark.parametrize('route', ROUTES)
def test_seeded_prompted_sampling_device_and_twin_routes(route, monkeypatch):
    """The rule of tests/test_vocab_sample.py: the device draw and the NumPy twin on the same logits give the same tokens
    until a free, open row's gap between its two largest keys falls below 2 KEY_ATOL; log-probabilities are 0 at the prompt."""
    from m3p_amd import decoder
    m, src_enc, src_len = _model()
    lens, seed, T = RAGGED, 5, 0.8
    prefix, plen = _reference(lens)[:2]
    _route(monkeypatch, route)
    inv_t = rng.inv_temperature(T)
    record, real = [], decoder.word_logits16

    def recording(model, tensor):
        logits, V = real(model, tensor)
        record.append((logits.clone(), V))
        return logits, V
    monkeypatch.setattr(decoder, 'word_logits16', recording)

    def run():
        del record[:]
        with torch.no_grad():
            return m.generate(src_enc, src_len, None, max_len=MAX_LEN[lens], sample_temperature=T, sample_seed=seed,
                              return_logprobs=True, prefix=prefix.cuda(), prefix_len=plen.cuda())

    gen_d, len_d, lp_d = run()
    first, first_close = 1 + min(lens), None
    g = gen_d.cpu().numpy()
    open_ = np.ones(g.shape, dtype=bool)                       # open_[p, b]: sentence b was unfinished before position p
    for p in range(2, g.shape[0]):
        open_[p] = open_[p - 1] & (g[p - 1] != EOS)
    for p in range(first, g.shape[0]):
        logits, V = record[p - first]
        x32 = logits[:, :V].float().cpu().numpy()
        a = float(np.abs(x32).max()) * inv_t
        key64 = rng.sample_keys(x32, inv_t, rng.stream_seed(seed, p, decoder.SAMPLE_SITE))
        best = np.sort(key64, axis=1)[:, -2:]
        for b, n in enumerate(lens):
            if p <= n:
                assert g[p, b] == int(prefix[p - 1, b]) and float(lp_d[p, b]) == 0.0
            elif open_[p, b] and best[b, 1] - best[b, 0] < 2 * KEY_ATOL(a) and first_close is None:
                first_close = p
    assert bool((lp_d[0] == 0).all()) and int((gen_d == EOS).sum()) == 2 * C['bs']
    with monkeypatch.context() as mp:
        mp.setattr(decoder, 'VOCAB_SELECT_MAX_K', 0)
        called = []
        mp.setattr(decoder.ops, 'vocab_sample', lambda *a, **k: called.append(a))
        gen_t, len_t, lp_t = run()
    assert not called, 'VOCAB_SELECT_MAX_K = 0 must take the twin'
    stop = min(gen_d.shape[0], gen_t.shape[0]) if first_close is None else first_close
    assert torch.equal(gen_d[:stop], gen_t[:stop]), first_close
    if first_close is None:
        assert torch.equal(gen_d, gen_t) and torch.equal(len_d, len_t)
        assert float((lp_d - lp_t).abs().max()) <= 1e-3
    for b, n in enumerate(lens):
        assert bool((lp_t[:1 + n, b] == 0).all()) and bool((lp_d[:1 + n, b] == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('hyps_dev', [False, True], ids=['host-hyps', 'device-hyps'])
@pytest.mark.parametrize('beam', [4, 12])
def test_prompted_beam_search_torch_and_select_routes(beam, hyps_dev, route, monkeypatch):
    """The same n-best lists from the torch route (VOCAB_SELECT_MAX_K = 0) and the select route (beam 4: ops.vocab_select,
    beam 12: ops.vocab_select_wide), with the hypothesis bookkeeping on the host or on the device.  Tokens and lengths are
    equal.  The scores are fp64 quotients of fp32 sums of the same words' log-probabilities, but the two routes read them off
    hidden states of different kernels (the torch route prefills on the tiled kernel and gathers its caches, the select
    route reads through the owner table on the rows kernel): a bf16 logit of magnitude <= 4 moves by at most two ulps
    (2 * 2^-8 * 4) per generated word, at most 9 words behind the 70-word prompt, over a length of at least 72.
    C['prompt_seed'] is one at which no two candidates sit that close at the beam's cut-off: where they do, the routes keep
    different hypotheses - torch.topk leaves ties open (tests/test_beam_wide.py counts such sentences and asserts nothing)."""
    from m3p_amd import decoder, ops
    m, src_enc, src_len = _model()
    prefix, plen = _reference(EQUAL)[:2]
    calls = _route(monkeypatch, route)
    monkeypatch.setattr(decoder, 'BEAM_HYPS_ON_DEVICE', hyps_dev)
    advances, real = [], ops.beam_advance
    monkeypatch.setattr(ops, 'beam_advance', lambda *a, **kw: advances.append(1) or real(*a, **kw))
    kw = dict(max_len=MAX_LEN[EQUAL], n_best=beam, return_scores=True, prefix=prefix.cuda(), prefix_len=plen.cuda())
    with torch.no_grad():
        dec_s, tl_s, sc_s = m.generate_beam(src_enc, src_len, None, beam, 1.0, False, **kw)
    assert not calls, 'the select route reads its caches through the owner table: the rows kernel'
    assert bool(advances) == hyps_dev
    monkeypatch.setattr(decoder, 'VOCAB_SELECT_MAX_K', 0)
    del advances[:]
    with torch.no_grad():
        dec_t, tl_t, sc_t = m.generate_beam(src_enc, src_len, None, beam, 1.0, False, **kw)
    assert not advances
    assert calls == ([(71, 0)] * C['n_dec_layers'] if route == 'tiled' and decoder.PREFILL_TILED_MIN_T <= 71 else []), calls
    assert dec_s.shape[1:] == (C['bs'], beam) and sc_s.dtype == torch.float64
    assert torch.equal(tl_s, tl_t) and torch.equal(dec_s, dec_t)
    assert float((sc_s - sc_t).abs().max()) <= 9 * 2 * 2.0 ** -8 * 4 / 72
    dec, tl = dec_s.cpu(), tl_s.cpu()
    for s in range(C['bs']):
        for j in range(beam):
            n = int(tl[s, j])
            assert torch.equal(dec[1:71, s, j], prefix[:70, s]) and dec[0, s, j] == EOS and dec[n - 1, s, j] == EOS
            assert int((dec[:, s, j] == EOS).sum()) == 2 and n >= 72
    assert bool((sc_s[:, :-1] >= sc_s[:, 1:]).all())
