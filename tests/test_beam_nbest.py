"""generate_beam(n_best=k, return_scores=True) end to end, and the hypothesis bookkeeping on the device inside the loop
(decoder.BEAM_HYPS_ON_DEVICE: ops.beam_advance, csrc/beam.hip) against the host bookkeeping behind the same selection, on the
models of synth.decoder_case.

- device against host bookkeeping, for both (length_penalty, early_stopping) pairs of tests/test_beam_wide.py, at the case's
  own beam and at beam 9, with and without decoding constraints: decoded, tgt_len, the full n_best = beam_size lists and the
  fp64 scores are equal exactly; the default call is [..., 0] of the n-best call;
- the golden hypotheses, by the criterion of tests/test_beam_cache.py;
- with device bookkeeping the loop reads the host once per call (decoder._host_read) and never calls Tensor.tolist, and the
  result does not depend on when the host notices that every sentence is done;
- VOCAB_SELECT_MAX_K = 0 and beam 33 take the torch loop and serve n_best too."""
import numpy as np
import pytest
import torch

from m3p_amd import synth
from tests.test_beam_wide import PAIRS
from tests.test_decoder import G, _hip_model

CONSTRAINTS = dict(no_repeat_ngram=2, min_len=3, banned_words=[5, 6])


def _call(m, c, src_enc, src_len, beam, lp, es, **kw):
    with torch.no_grad():
        return m.generate_beam(src_enc, src_len, c['tgt_lang_id'], beam, lp, es, max_len=c['max_len'], **kw)


def _count_calls(monkeypatch, module, name, calls=None):
    calls = [] if calls is None else calls
    real = getattr(module, name)

    def spy(*a, **kw):
        calls.append(name)
        return real(*a, **kw)
    monkeypatch.setattr(module, name, spy)
    return calls


def _check_lists(dec, tl, sc, bs, beam):
    """Shapes, dtypes and the order of an n_best = beam result."""
    assert dec.dtype == torch.int64 and dec.dim() == 3 and dec.shape[1:] == (bs, beam) and tl.shape == (bs, beam)
    assert sc.dtype == torch.float64 and sc.shape == (bs, beam)
    assert dec.shape[0] == int(tl.max())
    dec, tl, sc = dec.cpu(), tl.cpu(), sc.cpu()
    assert bool((sc[:, :-1] >= sc[:, 1:]).all()), 'the lists are not in descending order of score'
    for s in range(bs):
        for j in range(beam):
            n = int(tl[s, j])
            col = dec[:, s, j]
            assert int(col[0]) == synth.EOS and int(col[n - 1]) == synth.EOS and int((col == synth.EOS).sum()) == 2
            assert bool((col[n:] == synth.PAD).all()) and not bool((col[:n] == synth.PAD).any())


def _check_default(default, full):
    """The default call is hypothesis 0 of the n-best call (which may be padded further: another hypothesis is longer)."""
    (dec0, tl0), (dec, tl, sc) = default, full
    n = dec0.shape[0]
    assert dec0.dim() == 2 and tl0.dim() == 1 and torch.equal(tl0, tl[:, 0])
    assert torch.equal(dec0, dec[:n, :, 0]) and bool((dec[n:, :, 0] == synth.PAD).all())


@pytest.mark.gpu
@pytest.mark.parametrize('constrained', [False, True], ids=['plain', 'constrained'])
@pytest.mark.parametrize('tag,beam', [('multi', 3), ('multi', 9), ('wide', 4), ('wide', 9)])
def test_device_bookkeeping_equals_host_bookkeeping(tag, beam, constrained, monkeypatch):
    from m3p_amd import decoder, ops
    m, c, sd, src_enc, src_len, _, _ = _hip_model(tag)
    assert beam in (c['beam_size'], 9)
    kw = dict(CONSTRAINTS) if constrained else {}
    launches = _count_calls(monkeypatch, ops, 'beam_advance')
    for lp, es in PAIRS:
        monkeypatch.setattr(decoder, 'BEAM_HYPS_ON_DEVICE', True)
        dev_full = _call(m, c, src_enc, src_len, beam, lp, es, n_best=beam, return_scores=True, **kw)
        dev_default = _call(m, c, src_enc, src_len, beam, lp, es, **kw)
        dev_one = _call(m, c, src_enc, src_len, beam, lp, es, return_scores=True, **kw)
        n_dev = len(launches)
        assert n_dev >= 3, 'the device bookkeeping did not run'
        monkeypatch.setattr(decoder, 'BEAM_HYPS_ON_DEVICE', False)
        host_full = _call(m, c, src_enc, src_len, beam, lp, es, n_best=beam, return_scores=True, **kw)
        host_default = _call(m, c, src_enc, src_len, beam, lp, es, **kw)
        assert len(launches) == n_dev, 'BEAM_HYPS_ON_DEVICE = False must keep the bookkeeping on the host'
        del launches[:]
        _check_lists(*host_full, bs=c['bs'], beam=beam)
        for name, a, b in zip(('decoded', 'tgt_len', 'scores'), dev_full, host_full):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (tag, beam, lp, es, name)
        assert len(dev_default) == 2 and len(host_default) == 2
        for a, b in zip(dev_default, host_default):
            assert torch.equal(a, b), (tag, beam, lp, es, 'default call')
        _check_default(dev_default, dev_full)
        _check_default(host_default, host_full)
        assert len(dev_one) == 3 and torch.equal(dev_one[0], dev_default[0]) and torch.equal(dev_one[1], dev_default[1])
        assert dev_one[2].shape == (c['bs'],) and torch.equal(dev_one[2], dev_full[2][:, 0])


@pytest.mark.gpu
@pytest.mark.parametrize('tag', ['multi', 'wide'])
def test_device_bookkeeping_meets_the_golden_hypotheses(tag, monkeypatch):
    from m3p_amd import decoder, ops
    m, c, sd, src_enc, src_len, _, _ = _hip_model(tag)
    monkeypatch.setattr(decoder, 'BEAM_HYPS_ON_DEVICE', True)
    launches = _count_calls(monkeypatch, ops, 'beam_advance')
    n_equal = n_total = 0
    for lp, es in PAIRS:
        dec, tl = _call(m, c, src_enc, src_len, c['beam_size'], lp, es)
        key = '%s.beam_lp%.1f_es%d' % (tag, lp, es)
        ref, ref_len = G[key], G[key + '_len']
        dec, tl = dec.cpu().numpy(), tl.cpu().numpy()
        assert dec.shape[1] == ref.shape[1] and ((dec == synth.EOS).sum(0) == 2).all() and (dec[0] == synth.EOS).all()
        for b in range(ref.shape[1]):
            n_total += 1
            n_equal += int(tl[b] == ref_len[b] and np.array_equal(dec[:tl[b], b], ref[:ref_len[b], b]))
    assert launches and n_equal >= n_total - 1, (n_equal, n_total)


@pytest.mark.gpu
@pytest.mark.parametrize('tag,beam', [('multi', 3), ('wide', 9)])
def test_device_bookkeeping_reads_the_host_once(tag, beam, monkeypatch):
    from m3p_amd import decoder
    m, c, sd, src_enc, src_len, _, _ = _hip_model(tag)
    reads = _count_calls(monkeypatch, decoder, '_host_read')
    lists = _count_calls(monkeypatch, torch.Tensor, 'tolist')
    monkeypatch.setattr(decoder, 'BEAM_HYPS_ON_DEVICE', True)
    for lp, es in PAIRS:
        del reads[:], lists[:]
        _call(m, c, src_enc, src_len, beam, lp, es, n_best=beam, return_scores=True)
        assert len(reads) == 1 and not lists, (len(reads), len(lists))
    # the host bookkeeping reads once per step, through the same helper
    monkeypatch.setattr(decoder, 'BEAM_HYPS_ON_DEVICE', False)
    del reads[:]
    _call(m, c, src_enc, src_len, beam, 1.0, False)
    assert 2 <= len(reads) <= c['max_len'] - 1


@pytest.mark.gpu
def test_result_does_not_depend_on_when_the_host_notices(monkeypatch):
    """A host that never sees a `done` copy arrive decodes to max_len; one that waits for every copy stops at the first step
    after the last sentence finished.  Done sentences are frozen: the same lists either way."""
    from m3p_amd import decoder, ops
    m, c, sd, src_enc, src_len, _, _ = _hip_model('multi')
    beam = c['beam_size']
    monkeypatch.setattr(decoder, 'BEAM_HYPS_ON_DEVICE', True)
    launches = _count_calls(monkeypatch, ops, 'beam_advance')
    out, steps = {}, {}
    for name, query in (('never', lambda self: False), ('at once', lambda self: (self.synchronize(), True)[1])):
        with monkeypatch.context() as mp:
            mp.setattr(torch.cuda.Event, 'query', query)
            del launches[:]
            out[name] = _call(m, c, src_enc, src_len, beam, 0.6, True, n_best=beam, return_scores=True)
            steps[name] = len(launches)
    print('steps: %s' % steps)
    assert steps['never'] == c['max_len'] - 1 and steps['at once'] < steps['never'], steps
    for a, b in zip(out['never'], out['at once']):
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize('route', ['VOCAB_SELECT_MAX_K = 0', 'beam 33'])
def test_the_torch_loop_serves_n_best(route, monkeypatch):
    from m3p_amd import decoder, ops
    m, c, sd, src_enc, src_len, _, _ = _hip_model('multi')
    monkeypatch.setattr(decoder, 'BEAM_HYPS_ON_DEVICE', True)
    beam = c['beam_size']
    if route == 'beam 33':
        beam = 33
    else:
        monkeypatch.setattr(decoder, 'VOCAB_SELECT_MAX_K', 0)
    calls = []
    for name in ('beam_advance', 'vocab_select', 'vocab_select_wide'):
        _count_calls(monkeypatch, ops, name, calls)
    k = min(beam, 5)
    full = _call(m, c, src_enc, src_len, beam, 1.0, False, n_best=k, return_scores=True)
    default = _call(m, c, src_enc, src_len, beam, 1.0, False)
    assert not calls, 'the torch loop must not call %s' % sorted(set(calls))
    _check_lists(*full, bs=c['bs'], beam=k)
    _check_default(default, full)
    with pytest.raises(ValueError):
        _call(m, c, src_enc, src_len, beam, 1.0, False, n_best=beam + 1)
