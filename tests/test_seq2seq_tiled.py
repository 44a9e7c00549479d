"""The teacher-forced decoder pass of the seq2seq steps on the tiled attention kernels: functional.DecoderFn and the
cache-less scoring pass of decoder.decoder_forward dispatch the attention over the source encoding to csrc/attn_tiled.hip
by functional.cross_attn_tiled (and the self-attention to its causal kernels from CAUSAL_TILED_MIN_T on), and fall back to
the rows kernels of csrc/decode.hip.

GPU: the translation and captioning steps against the reference's goldens with the rules forced either way; a case large
enough for every loop of the kernels to run (T = 70, S = 130, ragged, NaN in the source rows past their length) against
the oracle + autograd; the two choices against each other under dropout; a declining launcher; the scoring pass.  CPU: the
rule as a pure function, its constants read back from the committed measurement.  Run with -s to see each figure before
it is asserted."""
import os
import re

import numpy as np
import pytest
import torch

from m3p_amd import synth
from oracle import ref_cpu
from tests.util import rel_l2

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_RTOL, LOSS_TOL, GRAD_RTOL = 1e-2, 5e-3, 5e-2        # tests/test_clm.py
TILED, ROWS = 0, 10 ** 9                                # what the rules' constants are forced to


def _force(monkeypatch, value):
    from m3p_amd import functional as Fn
    for name in ('CAUSAL_TILED_MIN_T', 'CROSS_TILED_MIN_TQ', 'CROSS_TILED_MIN_S'):
        monkeypatch.setattr(Fn, name, value)


def _launches(monkeypatch):
    """Counts the attention launchers a pass takes (a declined launch - None - is not one); the rows launchers are split by
    their causal argument: self-attention / attention over the source."""
    from m3p_amd import ops
    seen = dict(cross_fwd=0, cross_bwd=0, causal_fwd=0, causal_bwd=0, rows_self_fwd=0, rows_self_bwd=0, rows_src_fwd=0,
                rows_src_bwd=0, query_fwd=0)
    for name in ('attn_cross_fwd', 'attn_cross_bwd', 'attn_causal_fwd', 'attn_causal_bwd', 'attn_rows_fwd', 'attn_rows_bwd',
                 'attn_query_fwd'):
        def spy(*a, _real=getattr(ops, name), _name=name[5:], **kw):
            out = _real(*a, **kw)
            key = _name.replace('rows_', 'rows_self_' if kw.get('causal') else 'rows_src_') if _name.startswith('rows') else _name
            seen[key] += out is not None
            return out
        monkeypatch.setattr(ops, name, spy)
    return seen


def _expect(seen, n_layers, tiled, backward=True):
    nb = n_layers if backward else 0
    want = dict(cross_fwd=n_layers, cross_bwd=nb, causal_fwd=n_layers, causal_bwd=nb) if tiled else dict(
        rows_src_fwd=n_layers, rows_src_bwd=nb, rows_self_fwd=n_layers, rows_self_bwd=nb)
    assert seen == {k: want.get(k, 0) for k in seen}, seen


def _model(P, sd):
    from m3p_amd.model.transformer import TransformerModel
    torch.manual_seed(0)
    m = TransformerModel(P, is_encoder=True, with_output=True, is_crossModal=True).cuda()
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and not [k for k in missing if k.startswith(('encoder_attn', 'layer_norm15', 'cross_lang'))]
    return m


# ------------------------------------------------------------------------------------------------ the reference's goldens
@gpu
@pytest.mark.parametrize('force,tiled', [(TILED, True), (ROWS, False)])
def test_mt_step_vs_reference_on_either_kernels(monkeypatch, force, tiled):
    """tests/test_decoder.py::test_mt_step_forward_backward_vs_reference with the dispatch forced, at its bars."""
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'mt_step.npz'))
    P, sd, x1, len1, x2, len2 = synth.mt_case()
    _force(monkeypatch, force)
    seen = _launches(monkeypatch)
    m = _model(P, sd).train()
    m.arena().zero_grad()
    pred_mask, y = synth.mt_targets(x2, len2)
    enc1 = m('crossfwd', stream_='text', x=x1.cuda(), lengths=len1.cuda(), langs=x1.clone().fill_(0).cuda(), causal=False).transpose(0, 1)
    dec2 = m('crossfwd', stream_='text', x=x2.cuda(), lengths=len2.cuda(), langs=x2.clone().fill_(1).cuda(), causal=True,
             src_enc=enc1, src_len=len1.cuda())
    _, loss = m('predict', tensor=dec2, pred_mask=pred_mask.cuda(), y=y.cuda(), get_scores=False)
    loss.backward()
    torch.cuda.synchronize()
    _expect(seen, P.n_layers, tiled)
    own = dict(m.named_parameters())
    errs = {k[5:]: rel_l2(own[k[5:]].grad.float(), g[k]) for k in g.files if k.startswith('grad.') and np.abs(g[k]).max() >= 1e-7}
    worst = max(errs, key=errs.get)
    e_dec = rel_l2(dec2.float(), g['dec2'])
    print('mt_step (%s): dec2 %.3e, loss %.5f (reference %.5f), worst gradient %s %.3e' % (
        'tiled' if tiled else 'rows', e_dec, float(loss.detach()), float(g['loss']), worst, errs[worst]))
    assert e_dec < 1.5e-2
    assert abs(float(loss.detach()) - float(g['loss'])) < 5e-3
    bad = [(k, e) for k, e in errs.items() if e > 4e-2]
    assert len(errs) >= 30 and not bad, bad


@gpu
@pytest.mark.parametrize('force,tiled', [(TILED, True), (ROWS, False)])
def test_ic_step_vs_reference_on_either_kernels(monkeypatch, force, tiled):
    """tests/test_decoder.py::test_ic_step_vs_reference (ragged image lengths) with the dispatch forced, at its bars."""
    from m3p_amd.trainer import XTrainer
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'ic_step.npz'))
    P, sd, x_img, loc, img_len, x2, len2 = synth.ic_case()
    for k, v in synth.trainer_params(batch_size=6, langs=['en', 'zh'], ft_lgs=[]).items():
        setattr(P, k, v)
    _force(monkeypatch, force)
    m = _model(P, sd).train()
    m.arena().zero_grad()
    tr = XTrainer(m, {}, P)
    names = [k[5:] for k in g.files if k.startswith('grad.')]
    grads = {}
    opt = tr.optimizers['model']
    inner = opt.step

    def step(closure=None):          # look at the gradients the optimizer is about to consume
        torch.cuda.synchronize()
        named = dict(m.named_parameters())
        for k in names:
            grads[k] = named[k].grad.float().cpu().clone()
        return inner(closure)
    opt.step = step
    R = x_img.shape[0]
    x1_mask = (torch.arange(R)[None, :] < img_len[:, None]).long()
    seen = _launches(monkeypatch)
    loss = tr.ic_step_on_batch(x2, len2, x_img.transpose(0, 1).contiguous(), x1_mask, loc.transpose(0, 1).contiguous(), 'coco', 'img', 1.0)
    torch.cuda.synchronize()
    _expect(seen, P.n_layers, tiled)
    errs = {k: rel_l2(v, g['grad.' + k]) for k, v in grads.items()}
    worst = max(errs, key=errs.get)
    print('ic_step (%s): loss %.5f (reference %.5f), worst gradient %s %.3e' % (
        'tiled' if tiled else 'rows', float(loss), float(g['loss']), worst, errs[worst]))
    assert abs(float(loss) - float(g['loss'])) < 5e-3
    bad = [(k, e) for k, e in errs.items() if e > 4e-2]
    assert grads and not bad, bad
    assert opt.grad_norm() < 5


# ------------------------------------------------------------------------------------------------ a case whose loops run
T_BIG, S_BIG, B_BIG = 70, 130, 3


def _big_case(dropout=0.0):
    """The two-layer model of synth.mt_case (d = 128, H = 4) on 3 targets of up to 70 symbols (one of 2) over source
    encodings of up to 130 rows (one of 1): two query blocks, three key tiles, both ragged."""
    P, sd, *_ = synth.mt_case()
    P.dropout = P.attention_dropout = dropout
    rs = np.random.RandomState(91)
    x = torch.from_numpy(rs.randint(3, P.n_words - 1, size=(T_BIG, B_BIG))).long()
    lengths = torch.tensor([T_BIG, 2, 40])
    x[0] = synth.EOS
    for b in range(B_BIG):
        x[int(lengths[b]) - 1, b] = synth.EOS
        x[int(lengths[b]):, b] = synth.PAD
    src = torch.from_numpy(rs.standard_normal((B_BIG, S_BIG, P.emb_dim)).astype(np.float32))
    src_len = torch.tensor([S_BIG, 1, 65])
    pred_mask, y = synth.mt_targets(x, lengths)
    return P, sd, x, lengths, x.clone().fill_(1), src, src_len, pred_mask, y


def _past(src_len):
    return torch.arange(S_BIG)[None, :] >= src_len[:, None]


@pytest.fixture(scope='module')
def oracle_big():
    """The oracle's output, loss and gradients (parameters and source encoding) of the dropout-free pass, once."""
    P, sd, x, lengths, langs, src, src_len, pred_mask, y = _big_case()
    ref = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    src = src.clone().requires_grad_(True)
    out = ref_cpu.decoder_crossfwd(ref, P.n_layers, P.n_heads, x, lengths, src, src_len, langs=langs)
    _, loss = ref_cpu.predict_mlm(ref, out, pred_mask, y)
    loss.backward()
    return out.detach(), float(loss), {k: v.grad for k, v in ref.items() if v.grad is not None}, src.grad


def _run_big(m, dropout=0.0):
    """Forward + loss + backward of the pass on the model -> output, loss, parameter gradients, gradient reaching src_enc.
    Source rows past src_len hold NaN."""
    P, sd, x, lengths, langs, src, src_len, pred_mask, y = _big_case(dropout)
    src = src.masked_fill(_past(src_len)[:, :, None], float('nan')).cuda().requires_grad_(True)
    m.arena().zero_grad()
    out = m('crossfwd', stream_='text', x=x.cuda(), lengths=lengths.cuda(), langs=langs.cuda(), causal=True, src_enc=src,
            src_len=src_len.cuda())
    _, loss = m('predict', tensor=out, pred_mask=pred_mask.cuda(), y=y.cuda(), get_scores=False)
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.float().cpu().clone() for k, p in m.named_parameters() if p.grad is not None}
    return out.detach().float().cpu(), float(loss.detach()), grads, src.grad.float().cpu()


def _grad_errors(got, want, diff=False):
    """rel-L2 per parameter; attentions.*.k_lin.bias (a true gradient of zero) absolute against the q_lin.bias scale, as
    tests/test_clm.py."""
    qb = float(want['attentions.0.q_lin.bias'].norm())
    errs = {}
    for k in got:
        if k not in want:
            continue
        if '.k_lin.bias' in k:
            errs[k] = float((got[k] - want[k]).norm() if diff else got[k].norm()) / qb
        else:
            errs[k] = rel_l2(got[k], want[k])
    return errs


@gpu
@pytest.mark.parametrize('force,tiled', [(TILED, True), (ROWS, False)])
def test_decoder_pass_over_a_source_vs_oracle(oracle_big, monkeypatch, force, tiled):
    want_out, want_loss, want_grads, want_dsrc = oracle_big
    P, sd, x, lengths, langs, src, src_len, pred_mask, y = _big_case()
    _force(monkeypatch, force)
    seen = _launches(monkeypatch)
    m = _model(P, sd).train()
    out, loss, grads, dsrc = _run_big(m)
    _expect(seen, P.n_layers, tiled)
    errs = _grad_errors(grads, want_grads)
    assert len(errs) >= 40 and 'encoder_attn.1.k_lin.weight' in errs and 'encoder_attn.0.v_lin.bias' in errs
    worst = max(errs, key=errs.get)
    e_out, e_src = rel_l2(out, want_out), rel_l2(dsrc, want_dsrc)
    print('decoder pass over a source (%s): output %.3e, loss %.5f (oracle %.5f), d src_enc %.3e, worst gradient %s %.3e' % (
        'tiled' if tiled else 'rows', e_out, loss, want_loss, e_src, worst, errs[worst]))
    assert e_out <= OUT_RTOL
    assert abs(loss - want_loss) <= LOSS_TOL
    bad = [(k, e) for k, e in errs.items() if e > GRAD_RTOL]
    assert not bad, bad
    assert bool(torch.isfinite(dsrc).all()) and e_src <= GRAD_RTOL
    assert float(dsrc[_past(src_len)].abs().max()) == 0, 'source rows past src_len received a gradient'


@gpu
def test_tiled_and_rows_passes_agree_under_dropout(monkeypatch):
    """Two models from one state dict and the same forward counter draw the same dropout masks at every site - the tiled
    and the rows kernels index one stream - so the two passes differ by rounding only."""
    res = {}
    for tag, force in (('tiled', TILED), ('rows', ROWS)):
        P, sd, *_ = _big_case(dropout=0.1)
        _force(monkeypatch, force)
        m = _model(P, sd).train()
        assert m._fwd_counter == res.get('counter', m._fwd_counter)
        res['counter'] = m._fwd_counter
        res[tag] = _run_big(m, dropout=0.1)
    (o_t, l_t, g_t, s_t), (o_r, l_r, g_r, s_r) = res['tiled'], res['rows']
    assert set(g_t) == set(g_r) and len(g_t) >= 40
    errs = _grad_errors(g_t, g_r, diff=True)
    worst = max(errs, key=errs.get)
    print('dropout 0.1: output %.3e, loss tiled %.5f rows %.5f, d src_enc %.3e, worst gradient %s %.3e' % (
        rel_l2(o_t, o_r), l_t, l_r, rel_l2(s_t, s_r), worst, errs[worst]))
    assert rel_l2(o_t, o_r) <= OUT_RTOL
    assert abs(l_t - l_r) <= LOSS_TOL
    bad = [(k, e) for k, e in errs.items() if e > GRAD_RTOL]
    assert not bad, bad
    assert rel_l2(s_t, s_r) <= GRAD_RTOL


@gpu
def test_decoder_fn_takes_the_rows_kernels_when_the_cross_launcher_declines(monkeypatch):
    from m3p_amd import ops
    P, sd, *_ = _big_case()
    _force(monkeypatch, TILED)
    monkeypatch.setattr(ops, 'attn_cross_fwd', lambda *a, **kw: None)         # what the launcher answers for S = 1025 or dh = 48
    seen = _launches(monkeypatch)
    m = _model(P, sd).train()
    _run_big(m)
    n = P.n_layers
    assert seen == dict(cross_fwd=0, cross_bwd=0, causal_fwd=n, causal_bwd=n, rows_self_fwd=0, rows_self_bwd=0, rows_src_fwd=n,
                        rows_src_bwd=n, query_fwd=0), seen


# ------------------------------------------------------------------------------------------------ the scoring pass
@gpu
def test_scoring_pass_takes_the_tiled_forwards_and_decoding_does_not(oracle_big, monkeypatch):
    want_out = oracle_big[0]
    P, sd, x, lengths, langs, src, src_len, pred_mask, y = _big_case()
    _force(monkeypatch, TILED)
    seen = _launches(monkeypatch)
    m = _model(P, sd).eval()
    src_nan = src.masked_fill(_past(src_len)[:, :, None], float('nan')).cuda()
    n = P.n_layers
    zero = {k: 0 for k in seen}
    with torch.no_grad():
        out = m('crossfwd', stream_='text', x=x.cuda(), lengths=lengths.cuda(), langs=langs.cuda(), causal=True, src_enc=src_nan,
                src_len=src_len.cuda())
        torch.cuda.synchronize()
        assert seen == dict(zero, cross_fwd=n, causal_fwd=n), seen
        err = rel_l2(out.float().cpu(), want_out)
        print('scoring pass on the tiled forwards: output %.3e' % err)
        assert err <= OUT_RTOL
        # with a cache: the decoding kernels only
        seen.update(zero)
        cache = {'slen': 0}
        inc = m('crossfwd', stream_='text', x=x.cuda(), lengths=lengths.cuda(), langs=langs.cuda(), causal=True, src_enc=src_nan,
                src_len=src_len.cuda(), cache=cache)
        torch.cuda.synchronize()
        assert seen == dict(zero, query_fwd=2 * n), seen
        assert rel_l2(inc.float().cpu(), want_out) <= OUT_RTOL
        # one step of generate(): the same
        seen.update(zero)
        gen, gen_len = m.generate(src_nan, src_len.cuda(), 1, max_len=3)
        torch.cuda.synchronize()
        assert seen['query_fwd'] > 0 and seen == dict(zero, query_fwd=seen['query_fwd']), seen


# ------------------------------------------------------------------------------------------------ CPU: the rule
def test_cross_dispatch_rule_is_the_measured_one():
    """The rule as a pure function of (Tq, S): rows below its constants, tiled at the two step shapes of the measurement - and
    the constants are the ones profiles/attn_cross_vs_rows.txt states (nothing else pins them)."""
    from m3p_amd import functional as Fn
    text = open(os.path.join(ROOT, 'profiles', 'attn_cross_vs_rows.txt')).read()
    stated = {k: int(v) for k, v in re.findall(r'^(CROSS_TILED_MIN_TQ|CROSS_TILED_MIN_S) = (\d+)$', text, re.M)}
    assert set(stated) == {'CROSS_TILED_MIN_TQ', 'CROSS_TILED_MIN_S'}, stated
    for k, v in stated.items():
        assert getattr(Fn, k) == v, (k, getattr(Fn, k), v)
    tq, s = Fn.CROSS_TILED_MIN_TQ, Fn.CROSS_TILED_MIN_S
    assert Fn.cross_attn_tiled(tq, s) is True
    assert Fn.cross_attn_tiled(tq - 1, 1024) is False and Fn.cross_attn_tiled(512, s - 1) is False
    assert Fn.cross_attn_tiled(256, 256) is True and Fn.cross_attn_tiled(32, 100) is True
    # the measured grid supports it: every (Tq, S) line at or above the constants shows three tiled wins
    rows = re.findall(r'^cross +B +\d+ +Tq +(\d+) +S +(\d+) .*ratio +([\d.]+) +([\d.]+) +([\d.]+)$', text, re.M)
    assert len(rows) == 16, len(rows)
    for q_, s_, *ratios in rows:
        if Fn.cross_attn_tiled(int(q_), int(s_)):
            assert min(float(r) for r in ratios) > 1.0, (q_, s_, ratios)
