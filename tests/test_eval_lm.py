"""Valid-set perplexity and accuracy of the language-model objectives (m3p_amd/evaluation.py: evaluate_mlm / _mt / _ic / _mt_ic /
_mass / _ntg, run_all_evals) - the CPU side.

* ``eval_mask_out`` / ``eval_mask_sent`` against tests/golden/eval_lm.npz, recorded from the reference evaluator's own
  ``mask_out`` / ``mask_sent`` (DESIGN.md names the seeds and shapes).
* The evaluation loops driven by an oracle-backed stub model (the way tests/test_decoder.py drives the search loops): the stub
  answers crossfwd / jointfwd / predict_stats with oracle.ref_cpu and keeps every batch's word scores, on which the test restates
  the reference's arithmetic - sum of ``mean loss * len(y)``, count of ``max(1)[1] == y``, ``exp(xe / n)``, ``100 * n_valid / n``.
* run_all_evals on a params namespace with one step of every kind, and its scores through Trainer.save_best_model / end_epoch."""
import os
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from m3p_amd import synth
from oracle import ref_cpu

REL = 1e-6          # the same fp32 / fp64 sums in another order


@pytest.fixture(scope='module')
def G(golden_dir):
    return dict(np.load(os.path.join(golden_dir, 'eval_lm.npz')))


def _mask_params(G):
    n_words, mask_index, pad_index, eos_index = (int(v) for v in G['params'])
    return SimpleNamespace(n_words=n_words, mask_index=mask_index, pad_index=pad_index, eos_index=eos_index,
                           word_pred=float(G['word_pred']), word_mass=float(G['word_mass']))


# ------------------------------------------------------------------------------------------------ the evaluator's masking
@pytest.mark.parametrize('seed', [0, 5])
def test_eval_mask_out_is_the_reference_bit_for_bit(G, seed):
    """Two consecutive batches under ONE RandomState(seed): the second batch's draws depend on the state the first left."""
    from m3p_amd.evaluation import eval_mask_out
    assert seed in G['seeds'].tolist()
    P = _mask_params(G)
    rng = np.random.RandomState(seed)
    forced = 0
    for b in range(2):
        key = 'mask_out.s%d.b%d.' % (seed, b)
        x_in, lengths = torch.from_numpy(G[key + 'x_in']), torch.from_numpy(G[key + 'lengths'])
        assert int(lengths.min()) == 3
        x, y, pred_mask = eval_mask_out(x_in.clone(), lengths, P, rng)
        assert pred_mask.dtype == torch.bool
        for got, name in ((x, 'x'), (y, 'y'), (pred_mask, 'pred_mask')):
            assert np.array_equal(got.numpy(), G[key + name]), key + name
        assert torch.equal(x_in[pred_mask], y) and bool((x[pred_mask] == P.mask_index).all()) and torch.equal(x[~pred_mask], x_in[~pred_mask])
        per_sentence = pred_mask.sum(0)
        assert int(per_sentence.min()) >= 1
        forced += int((per_sentence[lengths == 3] == 1).sum())
    assert forced >= 1          # the three-symbol sentences take the forced pick (their only candidate is position 1)
    # a fresh generator on the second batch alone gives another selection: the carried state is what the fixture pins
    key = 'mask_out.s%d.b1.' % seed
    _, _, pm = eval_mask_out(torch.from_numpy(G[key + 'x_in']), torch.from_numpy(G[key + 'lengths']), P, np.random.RandomState(seed))
    assert not np.array_equal(pm.numpy(), G[key + 'pred_mask'])


@pytest.mark.parametrize('seed', [0, 5])
def test_eval_mask_sent_is_the_reference_bit_for_bit(G, seed):
    from m3p_amd.evaluation import eval_mask_sent
    P = _mask_params(G)
    rng = np.random.RandomState(seed)
    for b in range(2):
        key = 'mask_sent.s%d.b%d.' % (seed, b)
        x_in, lengths = torch.from_numpy(G[key + 'x_in']), torch.from_numpy(G[key + 'lengths'])
        out = eval_mask_sent(x_in.clone(), lengths, P, rng)
        for got, name in zip(out, ('x1', 'len1', 'x2', 'len2', 'y', 'pred_mask', 'positions')):
            assert got.dtype == (torch.bool if name == 'pred_mask' else torch.int64), name
            assert np.array_equal(got.numpy(), G[key + name]), key + name
        x1, len1, x2, len2, y, pred_mask, pos = out
        assert int(pred_mask.sum()) == int(len2.sum()) == y.numel()
    key = 'mask_sent.s%d.b1.' % seed
    again = eval_mask_sent(torch.from_numpy(G[key + 'x_in']), torch.from_numpy(G[key + 'lengths']), P, np.random.RandomState(seed))
    assert not np.array_equal(again[0].numpy(), G[key + 'x1'])


# ------------------------------------------------------------------------------------------------ the loops on the oracle
class OracleModel:
    """Answers the calls the evaluation functions make with oracle.ref_cpu on CPU tensors and keeps (word scores, y) of every
    predict_stats call."""

    def __init__(self, P, sd):
        self.P, self.sd, self.training, self.calls, self.modes = P, sd, True, [], []

    def eval(self):
        self.training = False
        return self

    def train(self):
        self.training = True
        return self

    def __call__(self, mode, **kw):
        assert not self.training and not torch.is_grad_enabled()
        sd, L, H = self.sd, self.P.n_layers, self.P.n_heads
        self.modes.append(mode if mode != 'crossfwd' else 'crossfwd/%s%s' % (kw.get('stream_', 'text'), '/causal' if kw['causal'] else ''))
        if mode == 'jointfwd':
            assert kw['langs'] is None and not kw['causal']
            return ref_cpu.jointfwd(sd, L, H, kw['x'], kw['lengths'], kw['x_img'], kw['lengths_img'], kw['image_loc'])
        if mode == 'crossfwd':
            if kw.get('stream_', 'text') == 'img':
                return ref_cpu.crossfwd_img(sd, L, H, kw['x'], kw['lengths'], kw['image_loc'], langs=kw.get('langs'))
            if kw['causal']:
                return ref_cpu.decoder_crossfwd(sd, L, H, kw['x'], kw['lengths'], kw['src_enc'], kw['src_len'], kw.get('positions'),
                                                kw.get('langs'), kw.get('enc_mask'))
            return ref_cpu.crossfwd_text(sd, L, H, kw['x'], kw['lengths'], langs=kw.get('langs'), positions=kw.get('positions'))
        assert mode == 'predict_stats', mode
        tensor, pred_mask, y = kw['tensor'], kw['pred_mask'], kw['y']
        rows = tensor[pred_mask.unsqueeze(-1).expand_as(tensor)].view(-1, tensor.shape[-1])
        scores = ref_cpu.word_scores(sd, rows)
        self.calls.append((scores, y))
        V = scores.shape[1]
        first = torch.where(scores == scores.max(1, keepdim=True)[0], torch.arange(V)[None, :], torch.full((1, 1), V)).min(1)[0]
        return F.cross_entropy(scores, y, reduction='sum').double(), (first == y).sum(), len(y)

    def restated(self):
        """The reference's per-batch arithmetic on the oracle's scores -> (ppl, acc, n_words)."""
        n_words = xe_loss = n_valid = 0
        for scores, y in self.calls:
            loss = F.cross_entropy(scores, y, reduction='mean')
            n_words += y.size(0)
            xe_loss += loss.item() * len(y)
            n_valid += (scores.max(1)[1] == y).sum().item()
        return np.exp(xe_loss / n_words), 100. * n_valid / n_words, n_words


@pytest.fixture
def cpu_batches(monkeypatch):
    from m3p_amd import evaluation as E
    monkeypatch.setattr(E, 'to_cuda', lambda *a: list(a))
    return E


def _close(a, b):
    return abs(a - b) <= REL * abs(b)


def _check(stub, scores, keys):
    ppl, acc, n = stub.restated()
    assert list(scores) == list(keys), list(scores)
    assert _close(scores[keys[0]], ppl) and _close(scores[keys[1]], acc), (scores, ppl, acc)
    assert stub.training                    # back in the mode it came in
    return n


def _mt_params(**over):
    P, sd, x1, len1, x2, len2 = synth.mt_case()
    for k, v in dict(langs=['en', 'zh'], word_pred=0.15, word_mass=0.5, ft_lgs=[], mt_only_text=False, refine_image=False, **over).items():
        setattr(P, k, v)
    return P, sd, x1, len1, x2, len2


def _second_batch(x2, len2, seed=5):
    """Another batch of target sentences of the same shape."""
    rs = np.random.RandomState(seed)
    x = x2.clone()
    for b in range(x.shape[1]):
        n = int(len2[b])
        x[1:n - 1, b] = torch.from_numpy(rs.randint(3, 1000, size=n - 2))
    return x


def test_evaluate_mt_and_ntg_on_the_oracle(cpu_batches):
    E = cpu_batches
    P, sd, x1, len1, x2, len2 = _mt_params()
    batches = [((x1, len1), (x2, len2)), ((x1, len1), (_second_batch(x2, len2), len2))]
    stub = OracleModel(P, sd)
    scores = E.evaluate_mt(stub, P, iter(batches), OrderedDict(), 'valid', 'en', 'zh')
    n = _check(stub, scores, ['valid_en-zh_mt_ppl', 'valid_en-zh_mt_acc'])
    assert n == 2 * int((len2 - 1).sum()) and stub.modes[:3] == ['crossfwd/text', 'crossfwd/text/causal', 'predict_stats']
    # text-to-text generation: the same loop with lang1's id on both sides, its own keys
    stub2 = OracleModel(P, sd)
    scores2 = E.evaluate_ntg(stub2, P, iter(batches), OrderedDict(), 'valid', 'en')
    _check(stub2, scores2, ['valid_en_NTG_ppl', 'valid_en_NTG_acc'])
    assert not _close(scores2['valid_en_NTG_ppl'], scores['valid_en-zh_mt_ppl'])        # (the target side's language id differs)
    # a wrapped model (.module) is unwrapped
    stub3 = OracleModel(P, sd)
    scores3 = E.evaluate_mt(SimpleNamespace(module=stub3), P, iter(batches), {}, 'valid', 'en', 'zh')
    assert scores3 == dict(scores)


@pytest.mark.parametrize('ft_lgs,lang_id', [([], 0), (['zh', 'en'], 1)])
def test_evaluate_ic_on_the_oracle(cpu_batches, ft_lgs, lang_id):
    E = cpu_batches
    P, sd, x_img, loc, img_len, x2, len2 = synth.ic_case()
    P.ft_lgs, P.langs = ft_lgs, ['en', 'zh']
    R, B = x_img.shape[0], x_img.shape[1]
    x1_mask = (torch.arange(R)[None, :] < img_len[:, None]).long()
    vis = (x_img.transpose(0, 1).contiguous(), x1_mask, loc.transpose(0, 1).contiguous(), list(range(B)))
    batches = [((x2, len2, None), vis), ((_second_batch(x2, len2), len2, None), vis)]
    stub = OracleModel(P, sd)
    scores = E.evaluate_ic(stub, P, iter(batches), OrderedDict(), 'valid', 'coco', 'img')
    _check(stub, scores, ['valid_coco-img_IC_ppl', 'valid_coco-img_IC_acc'])
    assert stub.modes[:3] == ['crossfwd/img', 'crossfwd/text/causal', 'predict_stats']
    # the language id is ft_lgs[0]'s, 'en' without fine-tuning languages: restated directly for the first batch
    enc = ref_cpu.crossfwd_img(sd, P.n_layers, P.n_heads, x_img, img_len, loc, langs=torch.full((R, B), lang_id)).transpose(0, 1)
    dec = ref_cpu.decoder_crossfwd(sd, P.n_layers, P.n_heads, x2, len2, enc, img_len, langs=x2.clone().fill_(lang_id))
    pred_mask, y = synth.mt_targets(x2, len2)
    want, _ = ref_cpu.predict_mlm(sd, dec, pred_mask, y)
    assert float((stub.calls[0][0] - want).abs().max()) < 1e-5


@pytest.mark.parametrize('only_text', [False, True])
def test_evaluate_mt_ic_on_the_oracle(cpu_batches, only_text):
    E = cpu_batches
    P, sd, x_src, len_src, x_img, loc, img_len, x2, len2 = synth.mt_ic_case()
    P.ft_lgs, P.langs, P.mt_only_text, P.refine_image = ['en', 'zh'], ['en', 'zh'], only_text, False
    R, B = x_img.shape[0], x_img.shape[1]
    vis = (x_img.transpose(0, 1).contiguous(), torch.ones(B, R, dtype=torch.long), loc.transpose(0, 1).contiguous(), list(range(B)))
    batches = [((x_src, len_src, None), (x2, len2, None), vis), ((x_src, len_src, None), (_second_batch(x2, len2), len2, None), vis)]
    stub = OracleModel(P, sd)
    scores = E.evaluate_mt_ic(stub, P, iter(batches), OrderedDict(), 'valid', 'coco', 'img')
    _check(stub, scores, ['valid_coco-img_IC_ppl', 'valid_coco-img_IC_acc'])
    assert stub.modes[0] == ('crossfwd/text' if only_text else 'jointfwd')
    # the decoder attends over len_all = len1 + src_len source positions (src_len alone under mt_only_text)
    if only_text:
        enc = ref_cpu.crossfwd_text(sd, P.n_layers, P.n_heads, x_src, len_src, langs=x_src.clone().fill_(0)).transpose(0, 1)
        len_all = len_src
    else:
        enc = ref_cpu.jointfwd(sd, P.n_layers, P.n_heads, x_src, len_src, x_img, img_len, loc).transpose(0, 1)
        len_all = img_len + len_src
    dec = ref_cpu.decoder_crossfwd(sd, P.n_layers, P.n_heads, x2, len2, enc, len_all, langs=x2.clone().fill_(1))
    pred_mask, y = synth.mt_targets(x2, len2)
    want, _ = ref_cpu.predict_mlm(sd, dec, pred_mask, y)
    assert float((stub.calls[0][0] - want).abs().max()) < 1e-5


def test_evaluate_mass_on_the_oracle(cpu_batches):
    E = cpu_batches
    P, sd, x1, len1, x2, len2 = _mt_params()
    batches = [(x1, len1), (x2, len2)]
    stub = OracleModel(P, sd)
    scores = E.evaluate_mass(stub, P, iter(batches), OrderedDict(), 'valid', 'en')
    _check(stub, scores, ['valid_en-en_mass_ppl', 'valid_en-en_mass_acc'])
    # first batch restated: RandomState(0) span, <mask> positions hidden from the decoder, explicit positions
    m1, l1, m2, l2, y, pred_mask, pos = E.eval_mask_sent(x1, len1, P, np.random.RandomState(0))
    enc = ref_cpu.crossfwd_text(sd, P.n_layers, P.n_heads, m1, l1, langs=m1.clone().fill_(0)).transpose(0, 1)
    enc_mask = m1.ne(P.mask_index).transpose(0, 1)
    assert not bool(enc_mask.all())
    dec = ref_cpu.decoder_crossfwd(sd, P.n_layers, P.n_heads, m2, l2, enc, l1, positions=pos, langs=m2.clone().fill_(0), enc_mask=enc_mask)
    want, _ = ref_cpu.predict_mlm(sd, dec, pred_mask, y)
    assert float((stub.calls[0][0] - want).abs().max()) < 1e-5 and torch.equal(stub.calls[0][1], y)
    blind = ref_cpu.decoder_crossfwd(sd, P.n_layers, P.n_heads, m2, l2, enc, l1, positions=pos, langs=m2.clone().fill_(0))
    assert float((blind - dec).abs().max()) > 1e-4               # enc_mask does something on this batch


def _stream_batches(P):
    from m3p_amd.datasets import StreamDataset
    sent, pos, _ = synth.token_stream()
    ds = StreamDataset(sent, pos, SimpleNamespace(bptt=16, batch_size=4, eos_index=synth.EOS, lang2id=P.lang2id))
    return list(ds.get_iterator(shuffle=False))


def _text_langs_params():
    cfg, P, sd, batch, langs = synth.text_langs_case()
    P.langs, P.word_pred = ['en', 'zh'], 0.15
    return cfg, P, sd


def test_evaluate_mlm_mono_stream_on_the_oracle(cpu_batches):
    E = cpu_batches
    cfg, P, sd = _text_langs_params()
    batches = _stream_batches(P)
    assert len(batches) >= 3
    stub = OracleModel(P, sd)
    scores = E.evaluate_mlm(stub, P, iter(batches), OrderedDict(), 'valid', 'zh', None)
    _check(stub, scores, ['valid_zh_mlm_ppl', 'valid_zh_mlm_acc'])
    # the batches restated: one RandomState(0) over the whole data set, langs filled with the language's id (n_langs > 1)
    rng = np.random.RandomState(0)
    for (x, lengths), (got, y_got) in zip(batches, stub.calls):
        xm, y, pred_mask = E.eval_mask_out(x, lengths, P, rng)
        out = ref_cpu.crossfwd_text(sd, P.n_layers, P.n_heads, xm, lengths, langs=xm.clone().fill_(1))
        want, _ = ref_cpu.predict_mlm(sd, out, pred_mask, y)
        assert torch.equal(y, y_got) and float((got - want).abs().max()) < 1e-5
    # deterministic: a second call scores the same words
    again = E.evaluate_mlm(OracleModel(P, sd), P, iter(batches), OrderedDict(), 'valid', 'zh', None)
    assert again == scores
    # an empty data set keeps the reference's sentinels
    assert E.evaluate_mlm(OracleModel(P, sd), P, iter([]), {}, 'valid', 'zh', None) == {'valid_zh_mlm_ppl': 1e9, 'valid_zh_mlm_acc': 0.}
    # a monolingual model gets no language ids
    P1 = synth.model_params(cfg['emb_dim'], cfg['n_heads'], cfg['n_layers'], cfg['n_words'])
    P1.langs, P1.word_pred = ['en'], 0.15
    seen = {}

    class NoLangs(OracleModel):
        def __call__(self, mode, **kw):
            if mode == 'crossfwd':
                seen['langs'] = kw['langs']
            return OracleModel.__call__(self, mode, **kw)
    E.evaluate_mlm(NoLangs(P1, {k: v for k, v in sd.items()}), P1, iter(batches[:1]), {}, 'valid', 'en', None)
    assert seen['langs'] is None


def test_evaluate_mlm_tlm_pairs_on_the_oracle(cpu_batches):
    E = cpu_batches
    P, sd, x1, len1, x2, len2 = _mt_params()
    batches = [((x1, len1), (x2, len2)), ((x2, len2), (x1, len1))]
    stub = OracleModel(P, sd)
    scores = E.evaluate_mlm(stub, P, iter(batches), OrderedDict(), 'valid', 'en', 'zh')
    _check(stub, scores, ['valid_en-zh_mlm_ppl', 'valid_en-zh_mlm_acc'])
    from m3p_amd.utils import concat_batches
    x, lengths, positions, langs = concat_batches(x1, len1, 0, x2, len2, 1, P.pad_index, P.eos_index, reset_positions=True)
    xm, y, pred_mask = E.eval_mask_out(x, lengths, P, np.random.RandomState(0))
    out = ref_cpu.crossfwd_text(sd, P.n_layers, P.n_heads, xm, lengths, langs=langs, positions=positions)
    want, _ = ref_cpu.predict_mlm(sd, out, pred_mask, y)
    assert float((stub.calls[0][0] - want).abs().max()) < 1e-5 and int(positions[int(len1[1]), 1]) == 0


# ------------------------------------------------------------------------------------------------ run_all_evals and its consumers
def _all_steps_case():
    P, sd, x1, len1, x2, len2 = _mt_params()
    _, _, x_img, loc, img_len, _, _ = synth.ic_case()
    R, B = x_img.shape[0], x_img.shape[1]
    x1_mask = (torch.arange(R)[None, :] < img_len[:, None]).long()
    vis = (x_img.transpose(0, 1).contiguous(), x1_mask, loc.transpose(0, 1).contiguous(), list(range(B)))
    for k, v in dict(is_master=True, mlm_steps=[('en', None), ('zh', None), ('en', 'zh')], mass_steps=['en', 'zh'], mt_steps=[('en', 'zh')],
                     bt_steps=[], text_steps=[('en', None)], is_ntg=True, is_generation=True, is_mt=False,
                     cross_modal_steps=[('coco', 'img')], is_understanding=False, cross_rel_steps=[]).items():
        setattr(P, k, v)
    asked = []

    def get_iterator(data_set, lang1, lang2):
        asked.append((data_set, lang1, lang2))
        if lang1 == 'coco':
            return iter([((x2, len2, None), vis)])
        if lang2 is None:
            return iter([(x1, len1), (x2, len2)])
        return iter([((x1, len1), (x2, len2))])
    return P, sd, get_iterator, asked


def test_run_all_evals_keys_averages_and_master_rank(cpu_batches):
    E = cpu_batches
    P, sd, get_iterator, asked = _all_steps_case()
    stub = OracleModel(P, sd)
    scores = E.run_all_evals(stub, P, get_iterator, 7)
    assert isinstance(scores, OrderedDict) and scores['epoch'] == 7 and list(scores)[0] == 'epoch'
    per_set = {'valid_en_mlm', 'valid_zh_mlm', 'valid_en-zh_mlm', 'valid_en-en_mass', 'valid_zh-zh_mass', 'valid_en-zh_mt', 'valid_zh-en_mt',
               'valid_en_NTG', 'valid_coco-img_IC', 'valid_mlm', 'valid_mass'}
    assert set(scores) == {'epoch'} | {k + s for k in per_set for s in ('_ppl', '_acc')}
    assert all(d == 'valid' for d, _, _ in asked)
    # the mass pairs join the translation set (both directions), every data set is asked for once
    assert sorted(asked, key=str) == sorted([('valid', 'en', None), ('valid', 'zh', None), ('valid', 'en', 'zh'),      # mlm
                                             ('valid', 'en', None), ('valid', 'zh', None),                            # mass
                                             ('valid', 'en', 'zh'), ('valid', 'zh', 'en'),                            # mt
                                             ('valid', 'en', 'en'), ('valid', 'coco', 'img')], key=str)      # ntg, ic
    for task, names in (('mlm', ['valid_en_mlm', 'valid_zh_mlm']), ('mass', ['valid_en-en_mass', 'valid_zh-zh_mass'])):
        for s in ('_ppl', '_acc'):
            assert _close(scores['valid_%s%s' % (task, s)], np.mean([scores[n + s] for n in names]))
    assert all(np.isfinite(v) for v in scores.values()) and scores['valid_en_mlm_ppl'] != scores['valid_zh_mlm_ppl']
    assert stub.training
    # multimodal translation instead of captioning under is_mt; NTG only under is_ntg
    P.is_mt, P.is_ntg, P.ft_lgs = True, False, ['en', 'zh']
    x_src = get_iterator('valid', 'en', None)
    (xs, ls), _ = list(x_src)

    def get_iterator_mt(data_set, lang1, lang2):
        if lang1 == 'coco':
            (x2, len2, _), vis = next(get_iterator(data_set, lang1, lang2))
            return iter([((xs, ls, None), (x2, len2, None), (vis[0], torch.ones_like(vis[1]), vis[2], vis[3]))])
        return get_iterator(data_set, lang1, lang2)
    stub2 = OracleModel(P, sd)
    scores2 = E.run_all_evals(stub2, P, get_iterator_mt, 8)
    assert 'valid_en_NTG_ppl' not in scores2 and 'jointfwd' in stub2.modes and 'crossfwd/img' not in stub2.modes
    assert scores2['valid_coco-img_IC_ppl'] != scores['valid_coco-img_IC_ppl']
    # a rank that is not the master evaluates nothing
    P.is_master = False
    idle = OracleModel(P, sd)
    assert E.run_all_evals(idle, P, get_iterator, 9) == OrderedDict({'epoch': 9}) and not idle.modes


def test_run_all_evals_understanding_averages(monkeypatch):
    """cross_rel_steps go through the existing evaluate_understanding_tasks; the averages keep the reference's pairing of flags
    and keys (xevaluator.py:226-234)."""
    from m3p_amd import evaluation as E

    def fake(model, params, iterator, scores, data_set, lang1, lang2):
        scores['%s_%s-%s_rel_t2i_acc' % (data_set, lang1, lang2)] = {'coco': 40.0, 'flicker': 60.0}[lang1]
        scores['%s_%s-%s_rel_i2t_acc' % (data_set, lang1, lang2)] = {'coco': 10.0, 'flicker': 30.0}[lang1]
        return scores
    monkeypatch.setattr(E, 'evaluate_understanding_tasks', fake)
    P = SimpleNamespace(is_master=True, is_understanding=True, is_slide=False, cross_rel_steps=[('coco', 'img'), ('flicker', 'img')],
                        t2i_flag=True, i2t_flag=True)
    scores = E.run_all_evals(None, P, lambda *a: iter([]), 0)
    assert scores['valid_I2T_acc'] == 20.0 and scores['valid_T2I_acc'] == 50.0
    P.t2i_flag = False
    assert 'valid_I2T_acc' not in E.run_all_evals(None, P, lambda *a: iter([]), 0)


def test_scores_drive_best_model_and_early_stopping(cpu_batches, tmp_path):
    """run_all_evals -> Trainer.save_best_model / end_epoch: '_valid_mlm_ppl' (lower is better) saves on an improvement only,
    a stopping criterion over valid_en-zh_mt_acc ends the run after `patience` epochs without one."""
    from m3p_amd.model.transformer import TransformerModel
    from m3p_amd.trainer import XTrainer
    E = cpu_batches
    P, sd, get_iterator, _ = _all_steps_case()
    for k, v in synth.trainer_params(langs=['en', 'zh'], dump_path=str(tmp_path), validation_metrics='_valid_mlm_ppl',
                                     stopping_criterion='valid_en-zh_mt_acc,1', mass_steps=P.mass_steps,
                                     cross_modal_steps=P.cross_modal_steps, is_ntg=True).items():
        setattr(P, k, v)
    scores = E.run_all_evals(OracleModel(P, sd), P, get_iterator, 0)
    m = TransformerModel(P, is_encoder=True, with_output=True, is_crossModal=True)
    tr = XTrainer(m, {}, P)
    assert tr.metrics == [('valid_mlm_ppl', False)] and tr.stopping_criterion == ('valid_en-zh_mt_acc', True)
    tr.save_best_model(scores)
    best = os.path.join(str(tmp_path), 'best-valid_mlm_ppl.pth')
    assert tr.best_metrics['valid_mlm_ppl'] == scores['valid_mlm_ppl'] and os.path.isfile(best)
    tr.end_epoch(scores)
    assert tr.epoch == 1 and tr.best_stopping_criterion == scores['valid_en-zh_mt_acc'] and tr.decrease_counts == 0
    assert os.path.isfile(os.path.join(str(tmp_path), 'checkpoint.pth'))
    # a worse epoch: higher perplexity does not replace the best model; the accuracy did not improve either
    os.remove(best)
    worse = OrderedDict(scores, epoch=1)
    worse['valid_mlm_ppl'] = scores['valid_mlm_ppl'] * 1.5
    tr.save_best_model(worse)
    assert not os.path.isfile(best) and tr.best_metrics['valid_mlm_ppl'] == scores['valid_mlm_ppl']
    tr.end_epoch(worse)
    assert tr.decrease_counts == 1
    # a better one is saved
    better = OrderedDict(scores, epoch=2)
    better['valid_mlm_ppl'] = scores['valid_mlm_ppl'] * 0.5
    tr.save_best_model(better)
    assert os.path.isfile(best) and tr.best_metrics['valid_mlm_ppl'] == better['valid_mlm_ppl']
    with pytest.raises(SystemExit):         # the second epoch in a row without a better accuracy: patience 1 is used up
        tr.end_epoch(better)


def test_scoring_head_is_forward_only():
    from m3p_amd import functional as Fn
    m = SimpleNamespace(training=True)
    with torch.enable_grad(), pytest.raises(NotImplementedError):
        Fn.mlm_eval_head(m, torch.zeros(2, 1, 4), torch.ones(2, 1, dtype=torch.bool), torch.zeros(2, dtype=torch.long))
    # the chunking keeps every chunk on whole 256-row tiles where the count allows, within the bound
    assert Fn._eval_chunks(4864) == [(0, 2560), (2560, 4864)]
    assert Fn._eval_chunks(300) == [(0, 300)] and Fn._eval_chunks(4096) == [(0, 4096)]
    for n in (1, 255, 4097, 9000, 3 * 4096 + 1):
        ch = Fn._eval_chunks(n)
        assert ch[0][0] == 0 and ch[-1][1] == n and all(a[1] == b[0] for a, b in zip(ch, ch[1:]))
        assert all(0 < r1 - r0 <= Fn.EVAL_CHUNK_ROWS for r0, r1 in ch)
