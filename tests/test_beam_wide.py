"""Beam search beyond 8 beams, end to end (m3p_amd/decoder.py: generate_beam over ops.vocab_select_wide, the caches in place
behind cache['owner'], the source once per sentence), on the models of synth.decoder_case.

- narrow beams forced through the wide entry (BEAM_SELECT_WIDE_MIN_K = 1) give the narrow route's tokens and lengths exactly
  and meet the reference's golden hypotheses by the criterion of tests/test_beam_cache.py;
- beams of 9 and 16 agree with the same loop run over a host twin of the selection - the total order T of
  tests/test_vocab_select.py (ref_select) on the bf16 logits, with the lse of ops.vocab_select(logits, V, None, 1, 1), which the
  contract makes bit-equal to the wide entry's - in tokens, lengths and every step's (score bits, flat_idx);
- with decoding constraints in front; VOCAB_SELECT_MAX_K = 0 and beam_size = 33 stay on the torch path.
Token equality with the torch path is printed, not asserted: torch.topk leaves ties open and its fp32 log_softmax differs from
the kernel's lse in the last bits (DESIGN.md 4 measured this for the narrow route)."""
import numpy as np
import pytest
import torch

from m3p_amd import synth
from tests.test_decoder import G, _hip_model
from tests.test_vocab_select import ref_select

PAIRS = ((1.0, False), (0.6, True))


def _spy_select(monkeypatch, name, log):
    """Record (beam, k, score bits, flat_idx) of every call of ops.<name>."""
    from m3p_amd import ops
    real = getattr(ops, name)

    def spy(logits, V, beam_scores, beam, k):
        res = real(logits, V, beam_scores, beam, k)
        log.append((name, beam, k, res[0].cpu().view(torch.int32).clone(), res[1].cpu().clone()))
        return res
    monkeypatch.setattr(ops, name, spy)


def _twin_select(log):
    """ops.vocab_select_wide on the host: the narrow entry's lse (bit-equal by the contract), then T by ref_select."""
    from m3p_amd import ops
    narrow = ops.vocab_select               # (the real one, whatever a test patches afterwards)

    def twin(logits, V, beam_scores, beam, k):
        lse = narrow(logits, V, None, 1, 1)[2]
        n = logits.shape[0]
        bsc = np.zeros(n, np.float32) if beam_scores is None else beam_scores.cpu().numpy()
        sc, idx = ref_select(logits[:, :V].float().cpu().numpy(), lse.cpu().numpy(), bsc, beam, k)
        sc, idx = torch.from_numpy(sc), torch.from_numpy(idx)
        log.append(('twin', beam, k, sc.view(torch.int32).clone(), idx.clone()))
        return sc.to(logits.device), idx.to(logits.device), lse
    return twin


def _beam(m, c, src_enc, src_len, beam, lp, es, **kw):
    with torch.no_grad():
        dec, tl = m.generate_beam(src_enc, src_len, c['tgt_lang_id'], beam, lp, es, max_len=c['max_len'], **kw)
    dec, tl = dec.cpu(), tl.cpu()
    assert dec.shape[1] == c['bs'] and bool(((dec == synth.EOS).sum(0) == 2).all()) and bool((dec[0] == synth.EOS).all())
    return dec, tl


def _spy_loop(monkeypatch, owners, sources):
    """Record every beam_idx handed to advance_owner and the row count of every src_enc handed to decoder_forward."""
    from m3p_amd import decoder
    real_owner, real_fwd = decoder.advance_owner, decoder.decoder_forward

    def owner_spy(owner, beam_idx, next_pos):
        owners.append(beam_idx.tolist())
        return real_owner(owner, beam_idx, next_pos)

    def fwd_spy(model, x, lengths, src_enc=None, *a, **kw):
        sources.append(int(src_enc.shape[0]))
        return real_fwd(model, x, lengths, src_enc, *a, **kw)
    monkeypatch.setattr(decoder, 'advance_owner', owner_spy)
    monkeypatch.setattr(decoder, 'decoder_forward', fwd_spy)


# ------------------------------------------------------------------------------------- narrow beams through the wide entry
@pytest.mark.gpu
@pytest.mark.parametrize('tag', ['multi', 'wide'])
def test_narrow_beams_through_the_wide_entry_equal_the_narrow_route(tag, monkeypatch):
    from m3p_amd import decoder
    m, c, sd, src_enc, src_len, _, _ = _hip_model(tag)
    beam = c['beam_size']
    assert 2 * beam < decoder.BEAM_SELECT_WIDE_MIN_K
    log = []
    _spy_select(monkeypatch, 'vocab_select', log)
    _spy_select(monkeypatch, 'vocab_select_wide', log)
    narrow = {p: _beam(m, c, src_enc, src_len, beam, *p) for p in PAIRS}
    assert log and all(e[0] == 'vocab_select' for e in log)
    narrow_log = list(log)
    del log[:]
    monkeypatch.setattr(decoder, 'BEAM_SELECT_WIDE_MIN_K', 1)
    n_equal = n_total = 0
    for p in PAIRS:
        dec, tl = _beam(m, c, src_enc, src_len, beam, *p)
        assert torch.equal(tl, narrow[p][1]) and torch.equal(dec, narrow[p][0]), (tag, p)
        key = '%s.beam_lp%.1f_es%d' % ((tag,) + p)
        ref, ref_len = G[key], G[key + '_len']
        dec, tl = dec.numpy(), tl.numpy()
        for b in range(ref.shape[1]):
            n_total += 1
            n_equal += int(tl[b] == ref_len[b] and np.array_equal(dec[:tl[b], b], ref[:ref_len[b], b]))
    assert n_equal >= n_total - 1, (n_equal, n_total)
    assert log and all(e[0] == 'vocab_select_wide' and e[1:3] == (beam, 2 * beam) for e in log)
    # step by step the two entries returned the same bits
    assert len(log) == len(narrow_log)
    for a, b in zip(log, narrow_log):
        assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])


# -------------------------------------------------------------------------------------------------------------- wide beams
def _reorders(owners, bs, beam):
    """Does some beam_idx map a sentence's rows to something other than themselves, beam 0 alone (the first step) or row 0 (a
    finished sentence)?"""
    for v in owners:
        for s in range(bs):
            rows = v[s * beam:(s + 1) * beam]
            if rows not in (list(range(s * beam, (s + 1) * beam)), [s * beam] * beam, [0] * beam):
                return True
    return False


def _against_the_twin(tag, beam, monkeypatch, pairs=PAIRS, **kw):
    from m3p_amd import decoder, ops
    m, c, sd, src_enc, src_len, _, _ = _hip_model(tag)
    assert decoder.BEAM_SELECT_WIDE_MIN_K <= 2 * beam <= decoder.BEAM_SELECT_WIDE_MAX_K
    owners, sources = [], []
    _spy_loop(monkeypatch, owners, sources)
    dev_log, twin_log, narrow_log = [], [], []
    twin = _twin_select(twin_log)
    _spy_select(monkeypatch, 'vocab_select', narrow_log)
    with monkeypatch.context() as mp:
        _spy_select(mp, 'vocab_select_wide', dev_log)
        got = {p: _beam(m, c, src_enc, src_len, beam, *p, **kw) for p in pairs}
    assert dev_log and all(e[1:3] == (beam, 2 * beam) for e in dev_log) and not narrow_log
    assert sources and all(s == c['bs'] for s in sources), 'src_enc must reach decoder_forward unexpanded'
    n = c['bs'] * beam
    assert _reorders(owners, c['bs'], beam), 'no step behind the first re-ordered the beams of a live sentence'
    with monkeypatch.context() as mp:
        mp.setattr(ops, 'vocab_select_wide', twin)
        exp = {p: _beam(m, c, src_enc, src_len, beam, *p, **kw) for p in pairs}
    assert len(twin_log) == len(dev_log)
    for t, (a, b) in enumerate(zip(dev_log, twin_log)):
        assert torch.equal(a[4], b[4]), (tag, beam, 'flat_idx of select call', t)
        assert torch.equal(a[3], b[3]), (tag, beam, 'score bits of select call', t)
    for p in pairs:
        assert torch.equal(got[p][1], exp[p][1]) and torch.equal(got[p][0], exp[p][0]), (tag, beam, p)
    # the torch path: counted, not asserted
    n_calls = len(dev_log) + len(twin_log)
    monkeypatch.setattr(decoder, 'VOCAB_SELECT_MAX_K', 0)
    same = 0
    for p in pairs:
        dec0, tl0 = _beam(m, c, src_enc, src_len, beam, *p, **kw)
        same += sum(int(int(tl0[b]) == int(got[p][1][b]) and torch.equal(dec0[:int(tl0[b]), b], got[p][0][:int(tl0[b]), b]))
                    for b in range(c['bs']))
    print('%s beam %d %s: %d of %d sentences equal the torch path' % (tag, beam, kw or '', same, len(pairs) * c['bs']))
    assert len(dev_log) + len(twin_log) == n_calls and sources[-1] == n, 'VOCAB_SELECT_MAX_K = 0 must take the torch path'


@pytest.mark.gpu
@pytest.mark.parametrize('tag,beam', [('multi', 9), ('wide', 16)])
def test_wide_beams_agree_with_the_host_twin(tag, beam, monkeypatch):
    _against_the_twin(tag, beam, monkeypatch)


@pytest.mark.gpu
def test_wide_beams_with_constraints_agree_with_the_host_twin(monkeypatch):
    _against_the_twin('multi', 9, monkeypatch, pairs=PAIRS[:1], no_repeat_ngram=2, min_len=3, banned_words=[5, 6])


# ------------------------------------------------------------------------------------------------------------ other routes
@pytest.mark.gpu
def test_beam_33_stays_on_the_torch_path(monkeypatch):
    from m3p_amd import decoder
    m, c, sd, src_enc, src_len, _, _ = _hip_model('multi')
    log = []
    _spy_select(monkeypatch, 'vocab_select', log)
    _spy_select(monkeypatch, 'vocab_select_wide', log)
    dec, tl = _beam(m, c, src_enc, src_len, 33, 1.0, False)
    assert not log
    monkeypatch.setattr(decoder, 'VOCAB_SELECT_MAX_K', 0)
    dec0, tl0 = _beam(m, c, src_enc, src_len, 33, 1.0, False)
    assert not log and torch.equal(tl, tl0) and torch.equal(dec, dec0)
