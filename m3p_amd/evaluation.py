"""Retrieval scoring on the MI355X model - the arithmetic of ``evaluate_image_retrieval``
(M3P/src/evaluation/xevaluator.py:1528-1657): every image is scored against every caption with
the cross-encoder (``jointfwd`` + ``predict(is_relation)`` under ``no_grad``), then
Recall@{1,5,10} is read off the (n_img, n_cap) score matrix in both directions (:1621-1657).

Differences from the reference, on purpose:
  * the image broadcast is an index gather on the device: one encoder call covers a tile of
    ``img_block`` images x ``chunk`` captions (the reference ``repeat``s one retrieval batch of
    images over a caption split, :1563-1564, and loops in Python);
  * scores stay on the device until the metric is read;
  * images are sharded over ranks by stride (the reference slices the image list by
    ``local_rank``, dataset_finetune.py:1218-1219) and the shards can be all-gathered.

Valid-set matching accuracy (``evaluate_t2i`` / ``evaluate_i2t`` / ``evaluate_understanding_tasks``,
xevaluator.py:1262-1417): each dataset item contributes ``sample_n`` (text, image) sequences, one of them the true
pair; a group counts as correct when its highest relation score sits on ``pos_labels``.

Valid-set perplexity and accuracy of the language-model objectives (``evaluate_mlm`` evaluator.py:240-270 / xevaluator.py:389-446,
``evaluate_mass`` :493-539, ``evaluate_mt`` :604-677, ``evaluate_ic`` :696-780, ``evaluate_mt_ic`` :799-884, ``evaluate_ntg``
:1119-1175) and ``run_all_evals`` (:120-235): the reference's batches and score keys, with the evaluator's own seeded masking
(``eval_mask_out`` :89-118, ``eval_mask_sent`` :541-602).  Per batch the reference reads ``loss.item() * len(y)`` and
``(word_scores.max(1)[1] == y).sum().item()`` back to the host; here ``predict_stats`` leaves both on the device, they are
summed there, and a data set costs ONE host read.  Ties of the maximum count for the lowest word id (the reference leaves them
open).  ``evaluate_clm`` (:329-387) scores next-word prediction on the monolingual stream or on joined pairs, without a masking
RNG; by default through the causal pass that ``Trainer.clm_step`` trains (the call the reference left commented out, :373),
``causal=False`` reproduces the reference's live line (:371-372), in which every position sees its own target.
Not built: the ``eval_bleu`` branches (hypothesis files, BLEU scripts), ``evaluate_slide`` and the test-set captioning
generators.
"""
from collections import OrderedDict

import numpy as np
import torch
import torch.distributed as dist

from .utils import concat_batches, to_cuda


@torch.no_grad()
def relation_score_matrix(model, x, lengths, x_img, image_loc, chunk=256, img_block=4, rank=0, world=1, refine_image=False):
    """x (T, n_cap) int64, lengths (n_cap,), x_img (R, n_img, 2048), image_loc (R, n_img, 5), all on the device.
    Returns (scores [n_img_local, n_cap] fp32, image indices of this rank)."""
    was_training = model.training
    model.eval()
    dev = x.device
    n_cap, n_img = x.shape[1], x_img.shape[1]
    R = x_img.shape[0]
    mine = torch.arange(rank, n_img, world, device=dev)
    out = torch.empty((mine.numel(), n_cap), dtype=torch.float32, device=dev)
    for r0 in range(0, mine.numel(), img_block):
        imgs = mine[r0:r0 + img_block]
        ni = imgs.numel()
        for c0 in range(0, n_cap, chunk):
            nc = min(n_cap, c0 + chunk) - c0
            # sequence j of the tile = (image j // nc, caption c0 + j % nc)
            img_of = imgs.repeat_interleave(nc)
            xi = x_img.index_select(1, img_of)
            li = image_loc.index_select(1, img_of)
            xt = x[:, c0:c0 + nc].repeat(1, ni)
            lt = lengths[c0:c0 + nc].repeat(ni)
            enc = model('jointfwd', x=xt, lengths=lt, x_img=xi, lengths_img=torch.full((ni * nc,), R, dtype=torch.long, device=dev),
                        causal=False, langs=None, image_loc=li, refine_image=refine_image)
            s = model('predict', tensor=enc.transpose(0, 1), is_relation=True)
            out[r0:r0 + ni, c0:c0 + nc] = s.view(ni, nc).float()
    if was_training:
        model.train()
    return out, mine


def gather_score_matrix(local_scores, mine, n_img, group=None):
    """All ranks' shards -> the full (n_img, n_cap) matrix on every rank (shards are strided: image i lives on rank
    i % world; short shards are padded to the longest for the collective)."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    if world == 1:
        return local_scores
    n_cap = local_scores.shape[1]
    per = (n_img + world - 1) // world
    buf = torch.zeros((per, n_cap), dtype=local_scores.dtype, device=local_scores.device)
    buf[:local_scores.shape[0]] = local_scores
    parts = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(parts, buf, group=group)
    full = torch.empty((n_img, n_cap), dtype=local_scores.dtype, device=local_scores.device)
    for r in range(world):
        idx = torch.arange(r, n_img, world, device=local_scores.device)
        full[idx] = parts[r][:idx.numel()]
    return full


def recall_at_k(scores, gt, ks=(1, 5, 10)):
    """scores [n_query, n_cand]; gt[q] = index of the ground-truth candidate (or a bool mask
    [n_query, n_cand] when several candidates are correct, e.g. 5 captions per image):
    fraction of queries with a correct candidate among the K best."""
    order = torch.argsort(scores, dim=1, descending=True)
    if gt.dim() == 1:
        rank = (order == gt[:, None]).float().argmax(dim=1)
    else:
        hit = torch.gather(gt, 1, order)
        rank = hit.float().argmax(dim=1)
    return {k: float((rank < k).float().mean()) for k in ks}


def retrieval_recalls(scores, labels):
    """xevaluator.py:1621-1657 on an (n_img, n_cap) score matrix and its 0/1 label matrix, vectorised:
    -> (t2i_r1, t2i_r5, t2i_r10, i2t_r1, i2t_r5, i2t_r10).  image -> sentence counts, per image, the first positive
    among its 10 best captions; sentence -> image counts, per caption, every positive among its 10 best images (the
    reference loop has no early exit there) and divides by the number of captions."""
    n_img, n_cap = scores.shape
    lab = labels.to(scores.device) == 1
    out = []
    # sentence -> image
    top = scores.t().topk(min(10, n_img), dim=-1).indices            # (n_cap, 10) image ids
    hit = torch.gather(lab.t(), 1, top)
    out += [float(hit[:, :k].sum()) / n_cap for k in (1, 5, 10)]
    # image -> sentence
    top = scores.topk(min(10, n_cap), dim=-1).indices                # (n_img, 10) caption ids
    hit = torch.gather(lab, 1, top)
    first = torch.where(hit.any(dim=1), hit.float().argmax(dim=1), torch.full((n_img,), 10**6, device=scores.device))
    out += [float((first < k).sum()) / n_img for k in (1, 5, 10)]
    return tuple(out)


@torch.no_grad()
def _matching_accuracy(model, params, batch):
    """One collate batch -> (#groups whose best-scoring member is the labelled pair, #groups).  Both layouts the
    reference unpacks: the pre-training tuples (t2i: (x1, len1, labels), (img, mask, loc, obj, pos, ori, ids); i2t with
    the extra (x2, len2) and CLCM labels) and the fine-tuning one ((x1, len1, lang_p), (img, mask, loc, pos, ids)).
    The per-position language ids the reference assembles (:1317-1326) feed ``langs``, which jointfwd ignores
    (transformer.py:937-938) - not built."""
    model = getattr(model, 'module', model)
    was_training = model.training
    model.eval()
    text, visual = batch[0], batch[-1]
    x1, len1 = text[0], text[1]
    if getattr(params, 'is_pretrain', False):
        if len(batch) == 3:                 # i2t: (clcm_labels, img, img_mask, img_loc, obj_labels, pos_labels, img_ori, img_ids)
            img, img_mask, img_loc, pos_labels = visual[1], visual[2], visual[3], visual[5]
        else:                               # t2i: (img, img_mask, img_loc, obj_labels, pos_labels, img_ori, img_ids)
            img, img_mask, img_loc, pos_labels = visual[0], visual[1], visual[2], visual[4]
    else:                                   # (img, img_mask, img_loc, pos_labels, img_ids); retrieval_collate adds obj_labels
        img, img_mask, img_loc = visual[0], visual[1], visual[2]
        pos_labels = visual[4] if len(visual) == 6 else visual[3]
    img_len = img_mask.sum(dim=1)
    x1, len1, x_img, loc, img_len = to_cuda(x1, len1, img.transpose(0, 1), img_loc.transpose(0, 1), img_len)
    enc = model('jointfwd', x=x1, lengths=len1, x_img=x_img, lengths_img=img_len, causal=False, langs=None,
                image_loc=loc, refine_image=getattr(params, 'refine_image', False))
    scores = model('predict', tensor=enc.transpose(0, 1), is_relation=True)
    pred = scores.view(-1, params.sample_n).float().argmax(dim=1).cpu()         # the step's one device read
    label = torch.from_numpy(np.asarray(pos_labels)).reshape(-1)
    if was_training:
        model.train()
    return int((pred == label).sum()), int(label.numel())


def evaluate_t2i(model, params, batch):
    """xevaluator.py:1309-1359."""
    return _matching_accuracy(model, params, batch)


def evaluate_i2t(model, params, batch):
    """xevaluator.py:1361-1417 (the same arithmetic on the i2t tuple)."""
    return _matching_accuracy(model, params, batch)


def evaluate_understanding_tasks(model, params, iterator, scores, data_set, lang1, lang2):
    """xevaluator.py:1262-1307: accumulates both accuracies over ``iterator`` (pairs of (t2i_batch, i2t_batch), what
    ``get_iterator(data_set, lang1, lang2)`` yields there) into ``scores`` under the reference's keys."""
    assert data_set in ('valid', 'test')
    t2i_acc = t2i_n = i2t_acc = i2t_n = 0
    for t2i_batch, i2t_batch in iterator:
        a, n = evaluate_t2i(model, params, t2i_batch)
        t2i_acc, t2i_n = t2i_acc + a, t2i_n + n
        a, n = evaluate_i2t(model, params, i2t_batch)
        i2t_acc, i2t_n = i2t_acc + a, i2t_n + n
    scores['%s_%s-%s_rel_t2i_acc' % (data_set, lang1, lang2)] = 100. * t2i_acc / t2i_n
    scores['%s_%s-%s_rel_i2t_acc' % (data_set, lang1, lang2)] = 100. * i2t_acc / i2t_n
    return scores


# ---------------------------------------------------------------------------------------------------------------------
# perplexity / accuracy of the language-model objectives
# ---------------------------------------------------------------------------------------------------------------------
def eval_mask_out(x, lengths, params, rng):
    """The evaluator's word selection (xevaluator.py:89-118; NOT the trainer's ``masking.mask_out``): Bernoulli(word_pred)
    per position from ``rng`` (a ``RandomState`` the caller seeds once per data set, so every epoch scores the same
    words), never the first row nor a sentence's last symbol or padding; a sentence left without a target gets one at
    ``rng.randint(1, len - 1)``.  Every selected word becomes <mask>.  -> (x, original ids, bool mask (slen, bs))."""
    slen, bs = x.size()
    sel = rng.rand(slen, bs) <= params.word_pred
    sel[0] = 0
    for i, n in enumerate(lengths.tolist()):
        sel[n - 1:, i] = 0
        if not sel[:n - 1, i].any():
            sel[rng.randint(1, n - 1), i] = 1
    pred_mask = torch.from_numpy(sel.astype(np.uint8)).bool()
    real = x[pred_mask]
    x = x.masked_fill(pred_mask, params.mask_index)
    assert 0 <= int(x.min()) and int(x.max()) < params.n_words
    return x, real, pred_mask


def eval_mask_sent(x, lengths, params, rng):
    """The evaluator's MASS span (xevaluator.py:541-602): per sentence of l symbols a span of max(1, round(l * word_mass) - 1)
    of them starting at 1 (p >= 0.8), at the latest start (p >= 0.6) or anywhere between; inside it the encoder input
    shows <mask> (p >= 0.2), a random word (p >= 0.05) or the word itself; the decoder reads the word BEFORE each hidden
    one at that word's position.  RNG order: per sentence the start's draws, then one or two draws per hidden word.
    -> (x1, len1, x2, len2, y, pred_mask, positions)."""
    pad = params.pad_index
    bs = lengths.size(0)
    inputs, prevs, outs, poss = [], [], [], []
    for i in range(bs):
        words = x[:lengths[i], i].tolist()
        n = len(words)
        span = max(1, round(n * params.word_mass) - 1)
        end = n - span + 1
        p = rng.rand()
        start = 1 if p >= 0.8 else (end - 1 if p >= 0.6 else rng.randint(1, end))
        shown = list(words)
        for j in range(start, min(start + span, n)):
            p = rng.rand()
            shown[j] = params.mask_index if p >= 0.2 else (rng.randint(params.n_words) if p >= 0.05 else words[j])
        hidden = range(start, min(start + span, n))
        inputs.append(shown)
        outs.append([words[j] for j in hidden])
        prevs.append([words[j - 1] for j in hidden])
        poss.append([j - 1 for j in hidden])
    len1 = lengths.clone()
    len2 = torch.LongTensor([len(o) for o in outs])
    x1 = torch.full((int(len1.max()), bs), pad, dtype=torch.long)
    x2, y, pos = (torch.full((int(len2.max()), bs), pad, dtype=torch.long) for _ in range(3))
    for i in range(bs):
        x1[:len1[i], i] = torch.LongTensor(inputs[i])
        x2[:len2[i], i] = torch.LongTensor(prevs[i])
        y[:len2[i], i] = torch.LongTensor(outs[i])
        pos[:len2[i], i] = torch.LongTensor(poss[i])
    pred_mask = y != pad
    return x1, len1, x2, len2, y.masked_select(pred_mask), pred_mask, pos


def _host_read(t):
    """The ONE device-to-host read of an evaluated data set (tests count the calls)."""
    return t.tolist()


class _LMStats:
    """Sums of the batches' (loss_sum, n_correct) kept where ``predict_stats`` left them - device scalars - and the word
    count, which the host knows (len(y))."""

    def __init__(self):
        self.xe = self.ok = None
        self.n = 0

    def add(self, loss_sum, n_correct, n):
        self.xe = loss_sum.double() if self.xe is None else self.xe + loss_sum.double()
        self.ok = n_correct.long() if self.ok is None else self.ok + n_correct.long()
        self.n += int(n)

    def write(self, scores, ppl_name, acc_name, empty=None):
        """np.exp(xe_loss / n_words), 100 * n_valid / n_words under the reference's keys; ``empty``: the (ppl, acc) of a data
        set without a word (evaluate_mlm only: the others divide)."""
        if self.n == 0 and empty is not None:
            scores[ppl_name], scores[acc_name] = empty
            return scores
        xe, ok = _host_read(torch.stack([self.xe, self.ok.double()]))     # (a count is exact in fp64 below 2^53)
        scores[ppl_name] = float(np.exp(xe / self.n))
        scores[acc_name] = 100. * int(round(ok)) / self.n
        return scores


class _eval_mode:
    """``model.module`` if wrapped, in eval mode; training mode restored on exit if it was on."""

    def __init__(self, model):
        self.model = getattr(model, 'module', model)

    def __enter__(self):
        self.was_training = self.model.training
        self.model.eval()
        return self.model

    def __exit__(self, *exc):
        if self.was_training:
            self.model.train()
        return False


def _next_word_targets(x2, len2):
    """Predict word t + 1 from position t, nothing from a sentence's last word (xevaluator.py:636-640)."""
    alen = torch.arange(int(len2.max()), dtype=torch.long, device=len2.device)
    pred_mask = alen[:, None] < len2[None] - 1
    y = x2[1:].masked_select(pred_mask[:-1])
    assert len(y) == int((len2 - 1).sum())
    return pred_mask, y


def _decode_and_score(model, stats, enc1, len1, x2, len2, langs2, pred_mask, y, **kw):
    dec2 = model('crossfwd', stream_='text', x=x2, lengths=len2, langs=langs2, causal=True, src_enc=enc1, src_len=len1, **kw)
    stats.add(*model('predict_stats', tensor=dec2, pred_mask=pred_mask, y=y))


@torch.no_grad()
def evaluate_mlm(model, params, iterator, scores, data_set, lang1, lang2):
    """xevaluator.py:389-446: masked-word perplexity and accuracy on the monolingual stream (``lang2 is None``, batches
    (x, lengths)) or on TLM pairs (batches ((x1, len1), (x2, len2)) joined with reset positions), the same words every
    call (RandomState(0))."""
    assert data_set in ('valid', 'test')
    assert lang1 in params.langs and (lang2 is None or lang2 in params.langs)
    rng = np.random.RandomState(0)
    lang1_id = params.lang2id[lang1]
    lang2_id = params.lang2id[lang2] if lang2 is not None else None
    stats = _LMStats()
    with _eval_mode(model) as m:
        for batch in iterator:
            if lang2 is None:
                x, lengths = batch
                positions = None
                langs = x.clone().fill_(lang1_id) if params.n_langs > 1 else None
            else:
                (sent1, len1), (sent2, len2) = batch
                x, lengths, positions, langs = concat_batches(sent1, len1, lang1_id, sent2, len2, lang2_id, params.pad_index,
                                                              params.eos_index, reset_positions=True)
            x, y, pred_mask = eval_mask_out(x, lengths, params, rng)
            x, y, pred_mask, lengths, positions, langs = to_cuda(x, y, pred_mask, lengths, positions, langs)
            tensor = m('crossfwd', stream_='text', x=x, lengths=lengths, positions=positions, langs=langs, causal=False)
            stats.add(*m('predict_stats', tensor=tensor, pred_mask=pred_mask, y=y))
    name = '%s_%s' % (data_set, lang1) if lang2 is None else '%s_%s-%s' % (data_set, lang1, lang2)
    return stats.write(scores, name + '_mlm_ppl', name + '_mlm_acc', empty=(1e9, 0.))


@torch.no_grad()
def evaluate_clm(model, params, iterator, scores, data_set, lang1, lang2, causal=True):
    """xevaluator.py:329-387: next-word perplexity and accuracy on the monolingual stream (``lang2 is None``, batches
    (x, lengths)) or on pairs (batches ((x1, len1), (x2, len2)) joined with reset positions); word t + 1 is scored from
    position t, nothing from a sentence's last word (:362-364).  No word is masked, so there is no RNG.
    ``causal=True`` (the default here) runs ``crossfwd(stream_='text', causal=True)``, the pass ``Trainer.clm_step`` trains
    and the call the reference left commented out (:373, as ``fwd``).  ``causal=False`` is the reference's live line
    (:371-372): the bidirectional text stream, in which position t attends word t + 1 - the number the reference prints, not
    a language-model perplexity.  Like the reference, a data set without a word divides by zero."""
    assert data_set in ('valid', 'test')
    assert lang1 in params.langs and (lang2 is None or lang2 in params.langs)
    lang1_id = params.lang2id[lang1]
    lang2_id = params.lang2id[lang2] if lang2 is not None else None
    stats = _LMStats()
    with _eval_mode(model) as m:
        for batch in iterator:
            if lang2 is None:
                x, lengths = batch
                positions = None
                langs = x.clone().fill_(lang1_id) if params.n_langs > 1 else None
            else:
                (sent1, len1), (sent2, len2) = batch
                x, lengths, positions, langs = concat_batches(sent1, len1, lang1_id, sent2, len2, lang2_id, params.pad_index,
                                                              params.eos_index, reset_positions=True)
            pred_mask, y = _next_word_targets(x, lengths)
            x, lengths, positions, langs, pred_mask, y = to_cuda(x, lengths, positions, langs, pred_mask, y)
            tensor = m('crossfwd', stream_='text', x=x, lengths=lengths, positions=positions, langs=langs, causal=bool(causal))
            stats.add(*m('predict_stats', tensor=tensor, pred_mask=pred_mask, y=y))
    if stats.n == 0:
        raise ZeroDivisionError('evaluate_clm: no word to score in %s (%s, %s)' % (data_set, lang1, lang2))
    name = '%s_%s' % (data_set, lang1) if lang2 is None else '%s_%s-%s' % (data_set, lang1, lang2)
    return stats.write(scores, name + '_clm_ppl', name + '_clm_acc')


@torch.no_grad()
def evaluate_mass(model, params, iterator, scores, data_set, lang1, lang2=None):
    """xevaluator.py:493-539: the hidden span of ``eval_mask_sent`` decoded over the masked sentence; the decoder may not
    look at the source's <mask> positions (``enc_mask``) and reads its inputs at their original positions."""
    assert data_set in ('valid', 'test') and lang1 in params.langs
    rng = np.random.RandomState(0)
    lang_id = params.lang2id[lang1]
    stats = _LMStats()
    with _eval_mode(model) as m:
        for x1, len1 in iterator:
            x1, len1, x2, len2, y, pred_mask, positions = eval_mask_sent(x1, len1, params, rng)
            langs1, langs2 = x1.clone().fill_(lang_id), x2.clone().fill_(lang_id)
            enc_mask = x1.ne(params.mask_index).transpose(0, 1)
            x1, len1, langs1, x2, len2, langs2, y, positions, pred_mask, enc_mask = to_cuda(
                x1, len1, langs1, x2, len2, langs2, y, positions, pred_mask, enc_mask)
            enc1 = m('crossfwd', stream_='text', x=x1, lengths=len1, langs=langs1, causal=False).transpose(0, 1)
            _decode_and_score(m, stats, enc1, len1, x2, len2, langs2, pred_mask, y, positions=positions, enc_mask=enc_mask)
    name = '%s_%s-%s' % (data_set, lang1, lang1)
    return stats.write(scores, name + '_mass_ppl', name + '_mass_acc')


def _evaluate_text_pair(model, params, iterator, stats, lang1_id, lang2_id):
    """The loop evaluate_mt and evaluate_ntg share: source sentence encoded, target teacher-forced over it."""
    with _eval_mode(model) as m:
        for (x1, len1), (x2, len2) in iterator:
            langs1, langs2 = x1.clone().fill_(lang1_id), x2.clone().fill_(lang2_id)
            pred_mask, y = _next_word_targets(x2, len2)
            x1, len1, langs1, x2, len2, langs2, y, pred_mask = to_cuda(x1, len1, langs1, x2, len2, langs2, y, pred_mask)
            enc1 = m('crossfwd', stream_='text', x=x1, lengths=len1, langs=langs1, causal=False).transpose(0, 1)
            _decode_and_score(m, stats, enc1, len1, x2, len2, langs2, pred_mask, y)


@torch.no_grad()
def evaluate_mt(model, params, iterator, scores, data_set, lang1, lang2):
    """xevaluator.py:604-677 without the BLEU branch: next-word perplexity and accuracy of the translation lang1 -> lang2."""
    assert data_set in ('valid', 'test') and lang1 in params.langs and lang2 in params.langs
    stats = _LMStats()
    _evaluate_text_pair(model, params, iterator, stats, params.lang2id[lang1], params.lang2id[lang2])
    name = '%s_%s-%s' % (data_set, lang1, lang2)
    return stats.write(scores, name + '_mt_ppl', name + '_mt_acc')


@torch.no_grad()
def evaluate_ntg(model, params, iterator, scores, data_set, lang1, lang2=None):
    """xevaluator.py:1119-1175: text-to-text generation pairs of one language (both sides carry lang1's id)."""
    assert data_set in ('valid', 'test')
    stats = _LMStats()
    _evaluate_text_pair(model, params, iterator, stats, params.lang2id[lang1], params.lang2id[lang1])
    return stats.write(scores, '%s_%s_NTG_ppl' % (data_set, lang1), '%s_%s_NTG_acc' % (data_set, lang1))


@torch.no_grad()
def evaluate_ic(model, params, iterator, scores, data_set, lang1, lang2):
    """xevaluator.py:696-780 without the BLEU branch: captions decoded over the image-only encoder stream.  Batches
    ((x2, len2, _), (x1, x1_mask, img_loc, img_id)) as caption_collate emits them; the language id of both streams is
    ``ft_lgs[0]``'s, or 'en' without fine-tuning languages."""
    assert data_set in ('valid', 'test')
    ft_lgs = getattr(params, 'ft_lgs', [])
    lang_id = params.lang2id[ft_lgs[0] if len(ft_lgs) > 0 else 'en']
    stats = _LMStats()
    with _eval_mode(model) as m:
        for (x2, len2, _), (x1, x1_mask, img_loc, _ids) in iterator:
            langs = x2.clone().fill_(lang_id)
            pred_mask, y = _next_word_targets(x2, len2)
            len1 = x1_mask.sum(dim=1)
            x1, img_loc = x1.transpose(0, 1), img_loc.transpose(0, 1)
            langs_img = x1_mask.transpose(0, 1).clone().fill_(lang_id)
            x1, len1, img_loc, x2, len2, y, langs, langs_img, pred_mask = to_cuda(x1, len1, img_loc, x2, len2, y, langs, langs_img,
                                                                                  pred_mask)
            enc1 = m('crossfwd', stream_='img', x=x1, lengths=len1, langs=langs_img, causal=False, cross_modal=True,
                     image_loc=img_loc, image_dist=None).transpose(0, 1)
            _decode_and_score(m, stats, enc1, len1, x2, len2, langs, pred_mask, y)
    name = '%s_%s-%s' % (data_set, lang1, lang2)
    return stats.write(scores, name + '_IC_ppl', name + '_IC_acc')


@torch.no_grad()
def evaluate_mt_ic(model, params, iterator, scores, data_set, lang1, lang2):
    """xevaluator.py:799-884 without the BLEU branch: the target decoded over jointfwd(regions | source words) - or, with
    ``mt_only_text``, over the source's text stream alone.  Batches ((x_src, src_len, _), (x2, len2, _), (x1, x1_mask,
    img_loc, img_id)) as mt_caption_collate emits them; languages ``ft_lgs[0]`` -> ``ft_lgs[1]``.  Same keys as evaluate_ic."""
    assert data_set in ('valid', 'test')
    src_id, tgt_id = params.lang2id[params.ft_lgs[0]], params.lang2id[params.ft_lgs[1]]
    refine = getattr(params, 'refine_image', False)
    stats = _LMStats()
    with _eval_mode(model) as m:
        for (x_src, src_len, _), (x2, len2, _), (x1, x1_mask, img_loc, _ids) in iterator:
            lang_src, langs = x_src.clone().fill_(src_id), x2.clone().fill_(tgt_id)
            pred_mask, y = _next_word_targets(x2, len2)
            len1 = x1_mask.sum(dim=1)
            x1, img_loc = x1.transpose(0, 1), img_loc.transpose(0, 1)
            x1, len1, img_loc, x2, len2, y, langs, lang_src, x_src, src_len, pred_mask = to_cuda(
                x1, len1, img_loc, x2, len2, y, langs, lang_src, x_src, src_len, pred_mask)
            if getattr(params, 'mt_only_text', False):
                enc = m('crossfwd', stream_='text', x=x_src, lengths=src_len, langs=lang_src, causal=False, refine_image=refine)
                len_all = src_len
            else:
                enc = m('jointfwd', x=x_src, lengths=src_len, x_img=x1, lengths_img=len1, causal=False, langs=None,
                        image_loc=img_loc, refine_image=refine)
                len_all = len1 + src_len
            _decode_and_score(m, stats, enc.transpose(0, 1), len_all, x2, len2, langs, pred_mask, y)
    name = '%s_%s-%s' % (data_set, lang1, lang2)
    return stats.write(scores, name + '_IC_ppl', name + '_IC_acc')


def run_all_evals(model, params, get_iterator, epoch, ema=None):
    """`_run_all_evals`, inside the context manager `ema` when one is given - ``Trainer.ema_weights()``: the model then computes
    with the exponential moving average of its weights (Adam.enable_ema) and the scores, under their usual names, are the
    averaged model's.  Entering and leaving that context is a collective under data parallelism, so every rank does both,
    whether it evaluates or not."""
    if ema is None:
        return _run_all_evals(model, params, get_iterator, epoch)
    with ema:
        return _run_all_evals(model, params, get_iterator, epoch)


def _run_all_evals(model, params, get_iterator, epoch):
    """The scores ``Trainer.save_best_model`` / ``end_epoch`` consume, after every epoch: xevaluator.py:120-235 for the tasks
    built here (``evaluate_clm`` over ``params.clm_steps`` first, as there) plus evaluator.py:250-252's ``evaluate_mlm`` over
    ``params.mlm_steps``, on the 'valid' split.
    ``get_iterator(data_set, lang1, lang2)`` is the caller's (``XTrainer.get_iterator`` fits): ``lang2`` is None for the
    monolingual sets (MLM stream, MASS sentences), the second language for pairs, and ``lang1`` again for the text-to-text
    pairs of ``evaluate_ntg`` (both sides in one language).  Only the master rank evaluates: the others return
    {'epoch': epoch}."""
    scores = OrderedDict({'epoch': epoch})
    g = lambda name, default: getattr(params, name, default)       # noqa: E731
    if g('is_master', True) is False:
        return scores
    data_set = 'valid'
    for lang1, lang2 in g('clm_steps', []):
        evaluate_clm(model, params, get_iterator(data_set, lang1, lang2), scores, data_set, lang1, lang2)
    for lang1, lang2 in g('mlm_steps', []):
        evaluate_mlm(model, params, get_iterator(data_set, lang1, lang2), scores, data_set, lang1, lang2)
    mass = list(g('mass_steps', []))
    for lang in mass:
        evaluate_mass(model, params, get_iterator(data_set, lang, None), scores, data_set, lang)
    pairs = list(g('mt_steps', [])) + [(l2, l3) for _, l2, l3 in g('bt_steps', [])] + [(a, b) for a in mass for b in mass if a != b]
    for lang1, lang2 in sorted(set(pairs)):
        evaluate_mt(model, params, get_iterator(data_set, lang1, lang2), scores, data_set, lang1, lang2)
    if g('is_ntg', False):
        for lang1, _ in g('text_steps', []):
            evaluate_ntg(model, params, get_iterator(data_set, lang1, lang1), scores, data_set, lang1)
    if g('is_generation', False):
        fn = evaluate_mt_ic if g('is_mt', False) else evaluate_ic
        for lang1, lang2 in sorted(set(g('cross_modal_steps', []))):
            fn(model, params, get_iterator(data_set, lang1, lang2), scores, data_set, lang1, lang2)
    rel = list(g('cross_rel_steps', []))
    if g('is_understanding', False) and not g('is_slide', False):
        for lang1, lang2 in sorted(set(rel)):
            evaluate_understanding_tasks(model, params, get_iterator(data_set, lang1, lang2), scores, data_set, lang1, lang2)
    # averages per task
    clm_mono = [l1 for l1, l2 in g('clm_steps', []) if l2 is None]
    if clm_mono:
        scores['%s_clm_ppl' % data_set] = np.mean([scores['%s_%s_clm_ppl' % (data_set, l)] for l in clm_mono])
        scores['%s_clm_acc' % data_set] = np.mean([scores['%s_%s_clm_acc' % (data_set, l)] for l in clm_mono])
    mono = [l1 for l1, l2 in g('mlm_steps', []) if l2 is None]
    if mono:
        scores['%s_mlm_ppl' % data_set] = np.mean([scores['%s_%s_mlm_ppl' % (data_set, l)] for l in mono])
        scores['%s_mlm_acc' % data_set] = np.mean([scores['%s_%s_mlm_acc' % (data_set, l)] for l in mono])
    if mass:
        scores['%s_mass_ppl' % data_set] = np.mean([scores['%s_%s-%s_mass_ppl' % (data_set, l, l)] for l in mass])
        scores['%s_mass_acc' % data_set] = np.mean([scores['%s_%s-%s_mass_acc' % (data_set, l, l)] for l in mass])
    if rel and g('is_understanding', False) and not g('is_slide', False):
        # (the reference's own pairing, :226-234: t2i_flag publishes the i2t accuracies as I2T, i2t_flag the t2i ones as T2I)
        if g('t2i_flag', False):
            scores['%s_I2T_acc' % data_set] = np.mean([scores['%s_%s-%s_rel_i2t_acc' % (data_set, a, b)] for a, b in rel])
        if g('i2t_flag', False):
            scores['%s_T2I_acc' % data_set] = np.mean([scores['%s_%s-%s_rel_t2i_acc' % (data_set, a, b)] for a, b in rel])
    return scores
