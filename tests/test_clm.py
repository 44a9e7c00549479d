"""The causal language-model objective: Trainer.clm_step / clm_step_on_batch (xtrainer.py:694-732), evaluate_clm
(xevaluator.py:329-387) and its place in run_all_evals (:133, :185-190).

CPU: the statistics keys, the prediction mask and targets against a literal restatement of xtrainer.py:710-715, and the
evaluation loop driven by the oracle-backed stub of tests/test_eval_lm.py.  GPU: the step on a two-layer synthetic
multilingual model against oracle.ref_cpu.decoder_crossfwd(src_enc=None) + predict_mlm + autograd at the SURVEY section 8c
bars, once on the tiled causal-attention kernels and once on the rows kernels; the two under dropout against each other;
twelve steps on a stream; evaluate_clm against the oracle; a forced one-rank data-parallel world against the plain step.
Run with -s to see each figure before it is asserted."""
import math
import os
import socket
import traceback
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from m3p_amd import synth
from oracle import ref_cpu
from tests.test_eval_lm import OracleModel
from tests.util import rel_l2

gpu = pytest.mark.gpu
OUT_RTOL, LOSS_TOL, GRAD_RTOL = 1e-2, 5e-3, 5e-2
MARGIN = 0.02           # oracle top-2 margin under which bf16 scores may land on the other word (tests/test_decoder.py)


# ------------------------------------------------------------------------------------------------ CPU: trainer surface
def test_stat_names_hold_the_clm_keys():
    from m3p_amd.trainer import _stat_names
    names = _stat_names(SimpleNamespace(langs=['en', 'zh'], clm_steps=[('en', None), ('en', 'zh')]))
    assert 'CLM-en' in names and 'CLM-en-zh' in names and 'CLM-zh' not in names
    assert not [n for n in _stat_names(SimpleNamespace(langs=['en'], clm_steps=[])) if n.startswith('CLM')]
    assert not [n for n in _stat_names(SimpleNamespace(langs=['en'])) if n.startswith('CLM')]


def _ragged_batch():
    _, _, _, _, x2, len2 = synth.mt_case()
    return x2, len2


def _stream_batch():
    rs = np.random.RandomState(3)
    x = torch.from_numpy(rs.randint(2, 1000, size=(16, 4))).long()
    return x, torch.full((4,), 16, dtype=torch.long)


@pytest.mark.parametrize('context_size', [0, 3])
@pytest.mark.parametrize('batch', ['ragged', 'stream'])
def test_clm_step_builds_the_reference_targets(batch, context_size):
    from m3p_amd.trainer import Trainer
    x, lengths = _ragged_batch() if batch == 'ragged' else _stream_batch()
    langs = x.clone().fill_(1)
    P = SimpleNamespace(context_size=context_size, fp16=False)
    asked, got = [], {}

    def generate_batch(lang1, lang2, name):
        asked.append((lang1, lang2, name))
        return x, lengths, None, langs, (None, None)

    def on_batch(x_, lengths_, pred_mask, y, lang, lambda_coeff, langs=None, positions=None, stat=None):
        got.update(x=x_, lengths=lengths_, pred_mask=pred_mask, y=y, lang=lang, lam=lambda_coeff, langs=langs, positions=positions, stat=stat)
        return 'loss'

    fake = SimpleNamespace(params=P, generate_batch=generate_batch, round_batch=lambda *a: a + (None,), clm_step_on_batch=on_batch)
    assert Trainer.clm_step(fake, 'zh', None, 0.5) == 'loss'
    assert asked == [('zh', None, 'causal')]
    # xtrainer.py:710-715, literally
    alen = torch.arange(lengths.max(), dtype=torch.long, device=lengths.device)
    pred_mask = alen[:, None] < lengths[None] - 1
    if context_size > 0:
        pred_mask[:context_size] = 0
    y = x[1:].masked_select(pred_mask[:-1])
    assert pred_mask.sum().item() == y.size(0)
    assert torch.equal(got['pred_mask'], pred_mask) and torch.equal(got['y'], y) and got['pred_mask'].dtype == torch.bool
    assert got['x'] is x and got['lengths'] is lengths and got['langs'] is langs and got['positions'] is None
    assert (got['lang'], got['lam'], got['stat']) == ('zh', 0.5, None)
    assert int(pred_mask.sum()) == int((lengths - 1).sum()) - (context_size * x.shape[1] if context_size else 0)
    # a pair records under its own key; a zero coefficient does nothing
    Trainer.clm_step(fake, 'en', 'zh', 1.0)
    assert got['stat'] == 'CLM-en-zh' and asked[-1] == ('en', 'zh', 'causal')
    n = len(asked)
    assert Trainer.clm_step(fake, 'en', None, 0) is None and len(asked) == n


# ------------------------------------------------------------------------------------------------ CPU: the evaluator on the oracle
class ClmOracle(OracleModel):
    """The stub of tests/test_eval_lm.py; the causal pass of evaluate_clm has no source encoding."""

    def __call__(self, mode, **kw):
        if mode == 'crossfwd' and kw['causal']:
            kw.setdefault('src_enc', None)
            kw.setdefault('src_len', None)
        return OracleModel.__call__(self, mode, **kw)


@pytest.fixture
def cpu_batches(monkeypatch):
    from m3p_amd import evaluation as E
    monkeypatch.setattr(E, 'to_cuda', lambda *a: list(a))
    return E


def _close(a, b):
    return abs(a - b) <= 1e-6 * abs(b)


def _langs_case():
    from m3p_amd.datasets import StreamDataset
    cfg, P, sd, _, _ = synth.text_langs_case()
    P.langs = ['en', 'zh']
    sent, pos, _ = synth.token_stream()
    ds = StreamDataset(sent, pos, SimpleNamespace(bptt=16, batch_size=4, eos_index=synth.EOS, lang2id=P.lang2id))
    return P, sd, list(ds.get_iterator(shuffle=False))[:3]


def _targets(x, lengths):
    alen = torch.arange(int(lengths.max()), dtype=torch.long)
    pred_mask = alen[:, None] < lengths[None] - 1
    return pred_mask, x[1:].masked_select(pred_mask[:-1])


def test_evaluate_clm_on_the_oracle(cpu_batches):
    E = cpu_batches
    P, sd, batches = _langs_case()
    stub = ClmOracle(P, sd)
    scores = E.evaluate_clm(stub, P, iter(batches), OrderedDict(), 'valid', 'zh', None)
    assert list(scores) == ['valid_zh_clm_ppl', 'valid_zh_clm_acc']
    ppl, acc, n = stub.restated()
    assert _close(scores['valid_zh_clm_ppl'], ppl) and _close(scores['valid_zh_clm_acc'], acc) and stub.training
    assert n == sum(int((lengths - 1).sum()) for _, lengths in batches)
    assert stub.modes == ['crossfwd/text/causal', 'predict_stats'] * len(batches)       # causal=True is the default
    # the batches restated: the stream, its language's id on every token, next-word targets, no masking
    for (x, lengths), (got, y_got) in zip(batches, stub.calls):
        pred_mask, y = _targets(x, lengths)
        out = ref_cpu.decoder_crossfwd(sd, P.n_layers, P.n_heads, x, lengths, langs=x.clone().fill_(1))
        want, _ = ref_cpu.predict_mlm(sd, out, pred_mask, y)
        assert torch.equal(y, y_got) and float((got - want).abs().max()) < 1e-5
    # causal=False: the reference's live line, the bidirectional stream - another (lower) perplexity
    stub2 = ClmOracle(P, sd)
    live = E.evaluate_clm(stub2, P, iter(batches), OrderedDict(), 'valid', 'zh', None, causal=False)
    assert stub2.modes == ['crossfwd/text', 'predict_stats'] * len(batches)
    x, lengths = batches[0]
    pred_mask, y = _targets(x, lengths)
    out = ref_cpu.crossfwd_text(sd, P.n_layers, P.n_heads, x, lengths, langs=x.clone().fill_(1))
    assert float((stub2.calls[0][0] - ref_cpu.predict_mlm(sd, out, pred_mask, y)[0]).abs().max()) < 1e-5
    assert not _close(live['valid_zh_clm_ppl'], scores['valid_zh_clm_ppl'])
    # pairs: joined with reset positions, per-token language ids, the pair's keys
    _, _, x1, len1, x2, len2 = synth.mt_case()
    stub3 = ClmOracle(P, sd)
    pair = E.evaluate_clm(stub3, P, iter([((x1, len1), (x2, len2))]), OrderedDict(), 'valid', 'en', 'zh')
    assert list(pair) == ['valid_en-zh_clm_ppl', 'valid_en-zh_clm_acc']
    from m3p_amd.utils import concat_batches
    x, lengths, positions, langs = concat_batches(x1, len1, 0, x2, len2, 1, P.pad_index, P.eos_index, reset_positions=True)
    pred_mask, y = _targets(x, lengths)
    out = ref_cpu.decoder_crossfwd(sd, P.n_layers, P.n_heads, x, lengths, positions=positions, langs=langs)
    assert float((stub3.calls[0][0] - ref_cpu.predict_mlm(sd, out, pred_mask, y)[0]).abs().max()) < 1e-5
    # like the reference, a data set without a word divides by zero: no sentinel (empty= is evaluate_mlm's alone)
    with pytest.raises(ZeroDivisionError):
        E.evaluate_clm(ClmOracle(P, sd), P, iter([]), {}, 'valid', 'zh', None)
    # a monolingual model gets no language ids
    cfg = synth.CONFIGS['cfg1']
    P1 = synth.model_params(cfg['emb_dim'], cfg['n_heads'], cfg['n_layers'], cfg['n_words'])
    P1.langs = ['en']
    seen = {}

    class NoLangs(ClmOracle):
        def __call__(self, mode, **kw):
            if mode == 'crossfwd':
                seen['langs'] = kw['langs']
            return ClmOracle.__call__(self, mode, **kw)
    E.evaluate_clm(NoLangs(P1, dict(sd)), P1, iter(batches[:1]), {}, 'valid', 'en', None)
    assert seen['langs'] is None


def test_run_all_evals_scores_the_clm_steps(cpu_batches):
    E = cpu_batches
    P, sd, batches = _langs_case()
    _, _, x1, len1, x2, len2 = synth.mt_case()
    for k, v in dict(is_master=True, mlm_steps=[('zh', None)], word_pred=0.15, mass_steps=[], mt_steps=[], bt_steps=[], text_steps=[],
                     is_ntg=False, is_generation=False, cross_modal_steps=[], is_understanding=False, cross_rel_steps=[]).items():
        setattr(P, k, v)
    asked = []

    def get_iterator(data_set, lang1, lang2):
        asked.append((data_set, lang1, lang2))
        return iter(batches[:2]) if lang2 is None else iter([((x1, len1), (x2, len2))])
    # without clm_steps (absent, or empty): exactly today's scores
    today = E.run_all_evals(ClmOracle(P, sd), P, get_iterator, 3)
    assert list(today) == ['epoch', 'valid_zh_mlm_ppl', 'valid_zh_mlm_acc', 'valid_mlm_ppl', 'valid_mlm_acc']
    P.clm_steps = []
    assert E.run_all_evals(ClmOracle(P, sd), P, get_iterator, 3) == today
    del asked[:]
    P.clm_steps = [('en', None), ('zh', None), ('en', 'zh')]
    stub = ClmOracle(P, sd)
    scores = E.run_all_evals(stub, P, get_iterator, 3)
    per_set = ['valid_en_clm', 'valid_zh_clm', 'valid_en-zh_clm', 'valid_zh_mlm', 'valid_clm', 'valid_mlm']
    assert list(scores) == ['epoch'] + [k + s for k in per_set for s in ('_ppl', '_acc')]
    assert asked[:3] == [('valid', 'en', None), ('valid', 'zh', None), ('valid', 'en', 'zh')]
    # the averages run over the monolingual entries only (xevaluator.py:185-190)
    for s in ('_ppl', '_acc'):
        assert _close(scores['valid_clm' + s], np.mean([scores['valid_en_clm' + s], scores['valid_zh_clm' + s]]))
    assert scores['valid_en_clm_ppl'] != scores['valid_zh_clm_ppl']                 # (the language id differs)
    assert {k: v for k, v in scores.items() if 'clm' not in k} == today and stub.training
    assert stub.modes.count('crossfwd/text/causal') == 5
    # pairs alone: per-pair scores, no average
    P.clm_steps = [('en', 'zh')]
    only = E.run_all_evals(ClmOracle(P, sd), P, get_iterator, 3)
    assert 'valid_clm_ppl' not in only and 'valid_en-zh_clm_ppl' in only


# ------------------------------------------------------------------------------------------------ GPU
T_STEP, B_STEP = 80, 6


def _step_case(dropout=0.0, **over):
    """The two-layer multilingual model of synth.mt_case (d = 128, H = 4, V = 1000) and a ragged batch of 6 sentences, the
    longest 80 symbols, one of 2."""
    P, sd, *_ = synth.mt_case()
    P.dropout = P.attention_dropout = dropout
    for k, v in synth.trainer_params(batch_size=B_STEP, langs=['en', 'zh'], clm_steps=[('zh', None)], context_size=0, **over).items():
        setattr(P, k, v)
    rs = np.random.RandomState(81)
    x = torch.from_numpy(rs.randint(3, P.n_words - 1, size=(T_STEP, B_STEP))).long()
    lengths = torch.tensor([T_STEP, 2, 65, 64, 33, 17])
    x[0] = synth.EOS
    for b in range(B_STEP):
        x[int(lengths[b]) - 1, b] = synth.EOS
        x[int(lengths[b]):, b] = synth.PAD
    pred_mask, y = _targets(x, lengths)
    return P, sd, x, lengths, x.clone().fill_(1), pred_mask, y


def _model(P, sd):
    from m3p_amd.model.transformer import TransformerModel
    torch.manual_seed(0)
    m = TransformerModel(P, is_encoder=True, with_output=True, is_crossModal=True).cuda()
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected
    return m


def _grads_at_step(m, opt, names):
    """Gradients the optimizer is about to consume, captured by wrapping its step()."""
    got = {}
    inner = opt.step

    def step(closure=None):
        torch.cuda.synchronize()
        named = dict(m.named_parameters())
        for k in names:
            if named[k].grad is not None:           # (a parameter the step does not reach - the heads of other objectives - has none)
                got[k] = named[k].grad.float().cpu().clone()
        return inner(closure)
    opt.step = step
    return got


def _launches(monkeypatch):
    """Counts the self-attention launchers DecoderFn takes."""
    from m3p_amd import ops
    seen = dict(tiled_fwd=0, tiled_bwd=0, rows_fwd=0, rows_bwd=0)
    for name, key in (('attn_causal_fwd', 'tiled_fwd'), ('attn_causal_bwd', 'tiled_bwd'), ('attn_rows_fwd', 'rows_fwd'),
                      ('attn_rows_bwd', 'rows_bwd')):
        def spy(*a, _real=getattr(ops, name), _key=key, **kw):
            out = _real(*a, **kw)
            seen[_key] += out is not None
            return out
        monkeypatch.setattr(ops, name, spy)
    return seen


@pytest.fixture(scope='module')
def oracle_step():
    """The oracle's output, loss and gradients of the dropout-free step, once for both kernel choices."""
    P, sd, x, lengths, langs, pred_mask, y = _step_case()
    ref = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    out = ref_cpu.decoder_crossfwd(ref, P.n_layers, P.n_heads, x, lengths, None, None, langs=langs)
    _, loss = ref_cpu.predict_mlm(ref, out, pred_mask, y)
    loss.backward()
    return out.detach(), float(loss), {k: v.grad for k, v in ref.items() if v.grad is not None}


@gpu
@pytest.mark.parametrize('min_t,tiled', [(0, True), (10 ** 9, False)])
def test_clm_step_on_batch_vs_oracle(oracle_step, monkeypatch, min_t, tiled):
    from m3p_amd import functional as Fn
    from m3p_amd.trainer import XTrainer
    want_out, want_loss, want_grads = oracle_step
    P, sd, x, lengths, langs, pred_mask, y = _step_case()
    monkeypatch.setattr(Fn, 'CAUSAL_TILED_MIN_T', min_t)
    seen = _launches(monkeypatch)
    m = _model(P, sd).train()
    out = m('crossfwd', stream_='text', x=x.cuda(), lengths=lengths.cuda(), langs=langs.cuda(), causal=True)
    err_out = rel_l2(out.float(), want_out)
    assert seen['tiled_fwd' if tiled else 'rows_fwd'] == P.n_layers and seen['rows_fwd' if tiled else 'tiled_fwd'] == 0
    tr = XTrainer(m, {}, P)
    names = [k for k, _ in m.named_parameters() if k in want_grads]
    assert len(names) >= 30 and 'cross_lang_embeddings.weight' in names and 'attentions.1.k_lin.weight' in names
    grads = _grads_at_step(m, tr.optimizers['model'], names)
    loss = tr.clm_step_on_batch(x, lengths, pred_mask, y, 'zh', 1.0, langs=langs)
    torch.cuda.synchronize()
    assert seen['tiled_bwd' if tiled else 'rows_bwd'] == P.n_layers and seen['rows_bwd' if tiled else 'tiled_bwd'] == 0
    qb = float(want_grads['attentions.0.q_lin.bias'].norm())
    errs = {k: (float(grads[k].norm()) / qb if '.k_lin.bias' in k else rel_l2(grads[k], want_grads[k])) for k in names}
    worst = max(errs, key=errs.get)
    print('clm step (%s): output %.3e, loss %.5f (oracle %.5f), worst gradient %s %.3e' % (
        'tiled' if tiled else 'rows', err_out, float(loss), want_loss, worst, errs[worst]))
    assert err_out <= OUT_RTOL
    assert abs(float(loss) - want_loss) <= LOSS_TOL
    # (attentions.*.k_lin.bias has a true gradient of zero: absolute against the q_lin.bias scale, as tests/test_model_parity.py)
    bad = [(k, e) for k, e in errs.items() if e > GRAD_RTOL]
    assert not bad, bad
    assert len(tr.stats['CLM-zh']) == 1 and tr.stats['processed_s'] == B_STEP and tr.n_sentences == B_STEP
    assert int(torch.stack(tr._pending_w).sum()) == int(pred_mask.sum()) == int((lengths - 1).sum())


@gpu
def test_decoder_fn_takes_the_rows_kernels_when_the_launcher_declines(monkeypatch):
    from m3p_amd import functional as Fn, ops
    P, sd, x, lengths, langs, pred_mask, y = _step_case()
    monkeypatch.setattr(Fn, 'CAUSAL_TILED_MIN_T', 0)
    monkeypatch.setattr(ops, 'attn_causal_fwd', lambda *a, **kw: None)        # what the launcher answers for T = 513 or dh = 48
    seen = _launches(monkeypatch)
    m = _model(P, sd).train()
    out = m('crossfwd', stream_='text', x=x.cuda(), lengths=lengths.cuda(), langs=langs.cuda(), causal=True)
    out.float().sum().backward()
    torch.cuda.synchronize()
    assert seen == dict(tiled_fwd=0, tiled_bwd=0, rows_fwd=P.n_layers, rows_bwd=P.n_layers)


@gpu
def test_tiled_and_rows_steps_agree_under_dropout(monkeypatch):
    """Two models from one state dict and the same forward counter draw the same dropout masks at every site - the tiled
    and the rows kernels index one stream - so the two steps differ by rounding only."""
    from m3p_amd import functional as Fn
    from m3p_amd.trainer import XTrainer
    res = {}
    for tag, min_t in (('tiled', 0), ('rows', 10 ** 9)):
        P, sd, x, lengths, langs, pred_mask, y = _step_case(dropout=0.1)
        monkeypatch.setattr(Fn, 'CAUSAL_TILED_MIN_T', min_t)
        m = _model(P, sd).train()
        assert m._fwd_counter == res.get('counter', m._fwd_counter)
        res['counter'] = m._fwd_counter
        tr = XTrainer(m, {}, P)
        names = [k for k, p in m.named_parameters() if p.requires_grad]
        grads = _grads_at_step(m, tr.optimizers['model'], names)
        loss = tr.clm_step_on_batch(x, lengths, pred_mask, y, 'zh', 1.0, langs=langs)
        res[tag] = (float(loss), {k: g for k, g in grads.items() if float(g.abs().max()) > 0})
    (l_t, g_t), (l_r, g_r) = res['tiled'], res['rows']
    assert set(g_t) == set(g_r) and len(g_t) >= 30
    qb = float(g_r['attentions.0.q_lin.bias'].norm())
    errs = {k: (float((g_t[k] - g_r[k]).norm()) / qb if '.k_lin.bias' in k else rel_l2(g_t[k], g_r[k])) for k in g_t}
    worst = max(errs, key=errs.get)
    print('dropout 0.1: loss tiled %.5f rows %.5f, worst gradient %s %.3e' % (l_t, l_r, worst, errs[worst]))
    assert abs(l_t - l_r) <= LOSS_TOL
    bad = [(k, e) for k, e in errs.items() if e > GRAD_RTOL]
    assert not bad, bad


@gpu
def test_twelve_clm_steps_on_a_stream():
    from m3p_amd.datasets import StreamDataset
    from m3p_amd.trainer import XTrainer
    P, sd, *_ = synth.mt_case()
    P.dropout = P.attention_dropout = 0.1
    # (lr 2e-3 without warm-up: twelve steps must move the frequent end-of-sentence symbol visibly)
    for k, v in synth.trainer_params(batch_size=2, langs=['en', 'zh'], clm_steps=[('en', None)], context_size=0, bptt=64,
                                     optimizer='adam,lr=0.002').items():
        setattr(P, k, v)
    sent, pos, _ = synth.token_stream(seed=43, n_sent=320)
    ds = StreamDataset(sent, pos, SimpleNamespace(bptt=64, batch_size=2, eos_index=synth.EOS, lang2id=P.lang2id))
    assert ds.n_batches >= 12
    m = _model(P, sd)
    tr = XTrainer(m, {'mono_stream': {'en': {'train': ds}}}, P)
    np.random.seed(5); torch.manual_seed(5)
    for _ in range(12):
        tr.clm_step('en', None, 1.0)
    losses = [float(v) for v in tr.stats['CLM-en']]
    print('clm stream losses', ' '.join('%.4f' % v for v in losses))
    assert len(losses) == 12 and all(math.isfinite(v) for v in losses)
    assert abs(losses[0] - math.log(P.n_words)) <= 0.05 * math.log(P.n_words)
    assert np.mean(losses[-3:]) < np.mean(losses[:3])
    # xtrainer.py:729-732: batch_size sentences, one per lane, every position but a lane's last predicted
    assert tr.n_sentences == 12 * 2 and tr.stats['processed_s'] == 12 * 2
    assert tr.stats['processed_w'] + int(torch.stack(tr._pending_w).sum()) == 12 * 2 * 63


@gpu
def test_evaluate_clm_against_the_oracle(monkeypatch):
    from m3p_amd import evaluation as E, ops
    P, sd, batches = _langs_case()
    # the oracle alone: scores, targets, and how many rows sit under the near-tie margin (a condition of the fixture)
    scores, ys = [], []
    for x, lengths in batches:
        pred_mask, y = _targets(x, lengths)
        out = ref_cpu.decoder_crossfwd(sd, P.n_layers, P.n_heads, x, lengths, langs=x.clone().fill_(1))
        scores.append(ref_cpu.predict_mlm(sd, out, pred_mask, y)[0])
        ys.append(y)
    scores, ys = torch.cat(scores), torch.cat(ys)
    top2 = scores.topk(2, dim=1)[0]
    sure = (top2[:, 0] - top2[:, 1]) >= MARGIN
    n = ys.numel()
    assert int((~sure).sum()) < 0.05 * n, 'the fixture puts too many rows under the near-tie margin'
    want_loss = float(torch.nn.functional.cross_entropy(scores, ys, reduction='mean'))
    want_hit = scores.max(1)[1] == ys
    seen, real = [], ops.ce_eval

    def spy(logits, V, target):
        out = real(logits, V, target)
        seen.append((out[1].long() == target).cpu())
        return out
    monkeypatch.setattr(ops, 'ce_eval', spy)
    m = _model(P, sd).train()
    got = E.evaluate_clm(m, P, iter(batches), OrderedDict(), 'valid', 'zh', None, causal=True)
    assert list(got) == ['valid_zh_clm_ppl', 'valid_zh_clm_acc'] and m.training
    got_hit = torch.cat(seen)
    got_loss = math.log(got['valid_zh_clm_ppl'])
    print('evaluate_clm: xe / n %.5f (oracle %.5f), hits %d (oracle %d) of %d, %d rows under the margin' % (
        got_loss, want_loss, int(got_hit.sum()), int(want_hit.sum()), n, int((~sure).sum())))
    assert abs(got_loss - want_loss) <= LOSS_TOL * abs(want_loss)
    assert got_hit.numel() == n and abs(got['valid_zh_clm_acc'] - 100. * int(got_hit.sum()) / n) < 1e-9
    assert torch.equal(got_hit[sure], want_hit[sure])
    # the reference's live line scores another pass
    live = E.evaluate_clm(m, P, iter(batches), OrderedDict(), 'valid', 'zh', None, causal=False)
    assert live['valid_zh_clm_ppl'] != got['valid_zh_clm_ppl']


# ---- a forced one-rank data-parallel world (M3P_DP_FORCE=1) against the plain step, in a fresh child process
def _free_port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close()
    return p


def _one_step(multi_gpu):
    from m3p_amd.trainer import XTrainer
    P, sd, x, lengths, langs, pred_mask, y = _step_case(multi_gpu=multi_gpu, is_master=True)
    m = _model(P, sd)
    tr = XTrainer(m, {}, P)
    loss = float(tr.clm_step_on_batch(x, lengths, pred_mask, y, 'zh', 1.0, langs=langs))
    torch.cuda.synchronize()
    return tr, m, loss


def _dp_worker(port, q):
    import torch.distributed as dist
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK='0', WORLD_SIZE='1', HSA_ENABLE_IPC_MODE_LEGACY='0',
                          M3P_DP_FORCE='1')
        torch.cuda.set_device(0)
        dist.init_process_group('nccl', rank=0, world_size=1)
        tr, m, loss = _one_step(True)
        wrapped = not tr.model.single
        tr.model.materialize_master()
        q.put(('ok', loss, m.arena().master.float().cpu().numpy(), wrapped))      # (numpy: a tensor's handle dies with the process)
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        q.put(('err', traceback.format_exc(), None, False))
        raise


@gpu
def test_clm_step_in_a_one_rank_world_matches_the_plain_step():
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    proc = ctx.Process(target=_dp_worker, args=(_free_port(), q))
    proc.start()
    status, loss_dp, master_dp, wrapped = q.get(timeout=600)
    proc.join(timeout=120)
    assert status == 'ok', loss_dp
    assert wrapped, 'M3P_DP_FORCE=1 did not put the one-rank world on the data-parallel path'
    tr, m, loss = _one_step(False)
    lr = tr.optimizers['model'].get_lr_for_step(0)
    diff = float((torch.from_numpy(master_dp) - m.arena().master.float().cpu()).abs().max())
    print('one-rank world: loss %.6f against %.6f, parameters differ by at most %.3e (lr %.3e)' % (loss_dp, loss, diff, lr))
    # the bars of tests/test_distributed_gpu.py's one-rank case: Adam moves every weight by <= ~lr per step
    assert abs(loss_dp - loss) <= LOSS_TOL
    assert diff <= 2.5 * lr
