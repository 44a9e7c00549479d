"""Decoder inference: ``crossfwd(causal=True, src_enc=..., cache=...)`` and the two search loops built on
it, ``generate`` (greedy / sampled) and ``generate_beam`` - transformer.py:970-1114 (the causal branch with the
``encoder_attn`` / ``layer_norm15`` sub-layer of :1087-1091), :149-210 (attention with the key / value cache),
:1216-1317, :1319-1515, :1518-1561.

One decoding step is latency / HBM work: one new token per sequence, every weight read once.  The projections run on the
bf16 GEMM of the training path (fused bias, 1/sqrt(dh), residual and GELU epilogues), attention on
``m3p_attn_query_fwd`` (csrc/decode.hip: one wave per (sequence, head, query) over the cached keys / values).  A call
WITHOUT a cache - the teacher-forced scoring pass of the evaluations, every target position at once - takes the tiled MFMA
forwards of the training pass instead (csrc/attn_tiled.hip: its causal kernels for the self-attention, its source-mask
kernels over the source encoding) where the dispatch rules of ``functional`` pick them and the launchers take the shape.  The cache
holds, per layer, ONE token-major bf16 tensor [bs, capacity, 2 d] (keys | values) for the self-attention and one
[bs, S_src, 2 d] for the encoder attention (projected once, at the first step); the reference keeps (k, v) head-major
tuples under the module ids and concatenates per step.  ``cache['slen']`` has the reference's meaning.

The next word comes from ``ops.vocab_select`` (csrc/select.hip) on a CUDA model: the rows' log-sum-exp and, per sentence,
the best entries of its beam * V scores straight from the bf16 logits - no fp32 copy, no log_softmax tensor, no topk.  Under
beam search the caches then stay in place: ``cache['owner']`` (int32 [rows, capacity]) names, per hypothesis and position,
the row whose slot holds that position's keys / values (``advance_owner`` after every step; ``m3p_attn_query_owner_fwd``
reads through it), and with ``cache['beam']`` the source's keys / values are kept once per sentence, not once per beam.
Beams of 9 to 32 (17 <= 2 * beam_size <= ``BEAM_SELECT_WIDE_MAX_K``) take ``ops.vocab_select_wide`` - the same contract by a
count selection and one sort per sentence - and everything behind the selection is the same in-place-cache code.
``VOCAB_SELECT_MAX_K`` is the dispatch rule; a CPU model, unseeded sampling and beams above 32 run the torch code below unchanged.
What a beam step does with its 2 * beam candidates - finished hypotheses into a bounded list per sentence, the next beams, the
done flags - is ``beam_advance_host``, one pure function over plain arrays behind one host copy per step; its device form is
``ops.beam_advance`` (csrc/beam.hip: one wave per sentence, the lists kept on the device, the next ``generated`` columns and
owner table written by the same launch), taken on the select routes when ``BEAM_HYPS_ON_DEVICE`` is set: the loop then reads
the host once per call.  The lists are what ``generate_beam(n_best=k, return_scores=True)`` returns on every route.
``generate(sample_seed=...)`` draws the next word by the seeded Gumbel-max contract of ``ops.vocab_sample`` (csrc/select.hip;
NumPy twin ``rng.sample_words``) instead: reproducible, with top-k truncation, a nucleus (top-p) cut
(``sample_top_p``: ``ops.vocab_nucleus_sample``) and the sampled words' log-probabilities; more than 16 and up to 1024
top-k candidates take ``ops.vocab_sample_wide`` (a count selection in place of k rounds of a maximum), nucleus cut included.
Both loops take decoding constraints - ``min_len``, ``repetition_penalty``, ``no_repeat_ngram``, ``banned_words`` - by ONE rule
for every route (include/m3p_hip.h: m3p_logits_constrain): where the words are selected on the device, ``ops.logits_constrain``
(csrc/constrain.hip) edits the step's bf16 logits in place in front of the selection kernels, everywhere else the torch twin
``constrain_scores_`` edits ``word_scores``; with all four off no route changes by a bit.
Both loops can start from a prompt (``prefix`` / ``prefix_len``; with it no source encoding is needed: generation from the
causal language model): the common part of the prompts is prefilled by ONE ``decoder_forward`` call - several new positions
over the cache, on the prefix mask of the tiled MFMA forward (``ops.attn_prefix_fwd``, csrc/attn_tiled.hip) from
``PREFILL_TILED_MIN_T`` positions on - and the rest of longer prompts is forced step by step behind the selection.

This module is forward only; the teacher-forced training pass of the same stream is ``functional.DecoderFn``
(``TransformerModel.crossfwd`` picks it in training mode), and calling ``decoder_forward`` itself with autograd enabled on
a model in training mode raises.
"""
import collections
import heapq
import math

import numpy as np
import torch

from . import functional as Fn
from . import lib as L
from . import ops
from . import rng

BF16 = torch.bfloat16

# Dispatch of the word selection, like functional.CAUSAL_TILED_MIN_T: a CUDA model takes ops.vocab_select for a step that
# asks for k <= VOCAB_SELECT_MAX_K entries per sentence (greedy: 1, beam search: 2 * beam_size) where the launcher takes
# the shape (VS_MAX_K = 16 of csrc/select.hip); 0 sends every call to the torch path.
VOCAB_SELECT_MAX_K = 16

# Beam search asks for k = 2 * beam_size entries per sentence: from BEAM_SELECT_WIDE_MIN_K on, and up to
# BEAM_SELECT_WIDE_MAX_K, the select route asks ops.vocab_select_wide (VSB_MAX_K = 64 of csrc/select.hip: beams up to 32)
# instead of ops.vocab_select; below it today's rule holds.  VOCAB_SELECT_MAX_K = 0 switches both off.  The upper bound is
# set by measurement ("Beam search beyond 8 beams"; profiles/decode_beam_wide.txt).
BEAM_SELECT_WIDE_MIN_K = 17
BEAM_SELECT_WIDE_MAX_K = 64

# Dispatch of the self-attention of a cached call that brings several new positions (the prefill of a prompted generate /
# generate_beam) over a cache that asks for it (cache['tiled_prefill'], which the two loops set; any other cache keeps the
# decoding kernels): from PREFILL_TILED_MIN_T new positions on, where no owner table is in use and the launcher takes the shape,
# it runs on ops.attn_prefix_fwd (csrc/attn_tiled.hip) over the layer's cache tensor, and the encoder attention of that call
# on ops.attn_cross_fwd by functional.cross_attn_tiled; below it, and for the single new position of every later step, the
# rows kernel stays.  0 switches the route off; a value below 8 is not allowed (callers feed short first pieces through the
# cache and rely on their bits).  The value is the smallest measured Tq from which the tiled kernel won every alternation
# (tools/bench_prefill.py, profiles/decode_prefill.txt; DESIGN.md 4, "Prompted decoding and the prefill kernel").
PREFILL_TILED_MIN_T = 8

# Stream-key site of the seeded sampling draws (rng.stream_seed(sample_seed, position, SAMPLE_SITE)): outside the dropout
# sites of the encoder (< 2^20), the refiner (functional._REF_SITE0 = 2^20 + ...) and the causal stream (_DEC_SITE0 = 2^21 + ...).
SAMPLE_SITE = 1 << 22


class _ColdWeights:
    """bf16 working copies of the encoder-attention sub-layer (parameters outside the training arena), re-made when any of
    them changed."""

    def __init__(self, model):
        self.model = model
        self.key = None
        self.q, self.kv, self.out, self.bq, self.bkv, self.bo = [], [], [], [], [], []

    def refresh(self):
        m = self.model
        ps = []
        for i in range(m.n_layers):
            for lin in ('q_lin', 'k_lin', 'v_lin', 'out_lin'):
                mod = m.get_submodule('encoder_attn.%d.%s' % (i, lin))
                ps += [mod.weight, mod.bias]
        key = tuple((p._version, p.data_ptr()) for p in ps)
        if key == self.key:
            return self
        self.q, self.kv, self.out, self.bq, self.bkv, self.bo = [], [], [], [], [], []
        for i in range(m.n_layers):
            g = lambda lin: m.get_submodule('encoder_attn.%d.%s' % (i, lin))   # noqa: E731
            self.q.append(g('q_lin').weight.detach().to(BF16).contiguous())
            self.kv.append(torch.cat([g('k_lin').weight.detach(), g('v_lin').weight.detach()]).to(BF16).contiguous())
            self.out.append(g('out_lin').weight.detach().to(BF16).contiguous())
            self.bq.append(g('q_lin').bias.detach().float().contiguous())
            self.bkv.append(torch.cat([g('k_lin').bias.detach(), g('v_lin').bias.detach()]).float().contiguous())
            self.bo.append(g('out_lin').bias.detach().float().contiguous())
        self.key = key
        return self


def _self_cache(cache, i, bs, need, d, dev):
    """The layer's self-attention key/value tensor with room for `need` positions (grown by doubling)."""
    key = ('self', i)
    cur = cache.get(key)
    if cur is None or cur.shape[1] < need:
        cap = max(int(cache.get('max_len', 0)), 64, need)
        if cur is not None:
            cap = max(cap, 2 * cur.shape[1])
        new = torch.zeros((bs, cap, 2 * d), dtype=BF16, device=dev)
        if cur is not None:
            new[:, :cur.shape[1]] = cur
        cache[key] = cur = new
    return cur


def decoder_forward(model, x, lengths, src_enc=None, src_len=None, positions=None, langs=None, cache=None):
    """crossfwd(stream_='text', causal=True): x (slen, bs) int64 -> (n_new, bs, d) bf16, n_new = slen - cache['slen'] (all of
    them without a cache).  src_enc (bs, S, d) / src_len (bs) switch the encoder-attention sub-layer on."""
    if torch.is_grad_enabled() and model.training:
        raise NotImplementedError('the causal decoder is built for inference (eval mode / torch.no_grad()): its '
                                  'teacher-forced training step is not part of this build (SURVEY 8 f4)')
    assert (src_enc is None) == (src_len is None)
    slen, bs = x.size()
    assert lengths.size(0) == bs
    d, H = model.dim, model.n_heads
    dh = d // H
    dev = model.embeddings.weight.device
    ar = model.arena()
    ar.refresh()
    pos0 = int(cache['slen']) if cache is not None else 0
    # caches that stay in place under beam search (generate_beam): the row that holds each (hypothesis, position), and how
    # many consecutive rows share one source sentence
    owner = cache.get('owner') if cache is not None else None
    beam = int(cache.get('beam', 1)) if cache is not None else 1
    n_new = slen - pos0
    assert n_new >= 1
    x = x.to(dev)
    lengths = lengths.to(dev)
    if positions is None:
        positions = torch.arange(slen, device=dev)[:, None].expand(slen, bs)
    else:
        assert positions.size() == (slen, bs)
        positions = positions.to(dev)
    tok = x[pos0:].t()                                                     # (bs, n_new), the reference's x[:, -_slen:]
    h = ar.w('embeddings.weight')[tok].float() + model.position_embeddings.weight.detach()[positions[pos0:].t()]
    if langs is not None:
        assert langs.size() == (slen, bs)
        h = h + model.cross_lang_embeddings.weight.detach()[langs.to(dev)[pos0:].t()]
    rowmask = (torch.arange(pos0, slen, device=dev)[None, :] < lengths[:, None]).to(torch.uint8).reshape(-1).contiguous()
    h16, _, _ = ops.layernorm_fwd(h.to(BF16).reshape(bs * n_new, d).contiguous(), model.layer_norm_emb.weight.detach(),
                                  model.layer_norm_emb.bias.detach(), rowmask=rowmask)
    qscale = 1.0 / math.sqrt(dh)
    cw = None
    if src_enc is not None:
        assert src_enc.size(0) * beam == bs and src_enc.size(2) == d
        S = src_enc.size(1)
        cw = model.decoder_cold_weights()
        src_klen = src_len.to(dev).to(torch.int32).clamp(max=S).contiguous()
        assert src_klen.size(0) == bs
        src16 = None
        xowner = None
        if beam > 1:
            xowner = cache.get('cross_owner')
            if xowner is None:
                cache['cross_owner'] = xowner = (torch.arange(bs, device=dev) // beam).to(torch.int32)
    # without a cache every position is scored at once: the attentions of the training pass, by its rules, without dropout
    tiled = cache is None and slen >= Fn.CAUSAL_TILED_MIN_T
    # with a cache, several new positions at once are a prefill: the prefix mask of the tiled forward over the layer's cache
    # (caches that stay in place behind an owner table keep the rows kernel, which reads through it).  The cache asks for it
    # (cache['tiled_prefill'], set by generate / generate_beam): a bare {'slen': 0} cache keeps the decoding kernels for
    # every call, as it always did
    assert PREFILL_TILED_MIN_T == 0 or PREFILL_TILED_MIN_T >= 8
    prefill = cache is not None and bool(cache.get('tiled_prefill')) and owner is None and 1 <= PREFILL_TILED_MIN_T <= n_new
    xtiled = (cache is None or (prefill and beam == 1)) and src_enc is not None and Fn.cross_attn_tiled(n_new, S)
    for i in range(model.n_layers):
        a, f = 'attentions.%d.' % i, 'ffns.%d.' % i
        wqkv, bqkv = ar.qkv_w16(i), ar.qkv_bias(i)
        ctx = None
        if tiled:
            qkv = ops.gemm_nt(h16, wqkv, L.EPI_BIAS, bias=bqkv, scale_cols=d, scale=qscale)
            res = ops.attn_causal_fwd(qkv, bs, slen, H, dh)
            if res is None:                 # (the first layer decides for the pass: the launcher's answer depends on the shape alone)
                assert i == 0
                tiled = False
            else:
                ctx = res[0]
        if ctx is None:
            q = ops.gemm_nt(h16, wqkv[:d], L.EPI_BIAS, bias=bqkv[:d], scale_cols=d, scale=qscale)
            kv = ops.gemm_nt(h16, wqkv[d:], L.EPI_BIAS, bias=bqkv[d:]).view(bs, n_new, 2 * d)
            if cache is not None:
                store = _self_cache(cache, i, bs, slen, d, dev)
                store[:, pos0:slen] = kv
                kv = store
            assert owner is None or (owner.shape[0] == bs and owner.shape[1] >= slen)
            res = ops.attn_prefix_fwd(q, kv, bs, n_new, H, dh, pos0) if prefill else None
            if res is None:                 # (the first layer decides for the pass, as above)
                assert i == 0 or not prefill
                prefill = False
                ctx = ops.attn_query_fwd(q, kv, None, bs, n_new, H, dh, slen, causal=True, pos0=pos0, owner=owner)
            else:
                ctx = res[0]
        pre = ops.gemm_nt(ctx, ar.w(a + 'out_lin.weight'), L.EPI_BIAS_DROP_RES, bias=ar.p(a + 'out_lin.bias'), aux=h16)
        h16, _, _ = ops.layernorm_fwd(pre, ar.p('layer_norm1.%d.weight' % i), ar.p('layer_norm1.%d.bias' % i))
        if cw is not None:
            q2 = ops.gemm_nt(h16, cw.q[i], L.EPI_BIAS, bias=cw.bq[i], scale_cols=d, scale=qscale)
            kvc = cache.get(('cross', i)) if cache is not None else None
            if kvc is None:
                if src16 is None:
                    src16 = src_enc.detach().to(device=dev, dtype=BF16).contiguous()
                    if beam > 1:
                        # The GEMM picks its kernel by the row count, and two kernels add the products in different orders:
                        # projected on bs / beam * S rows, a few keys / values come out one bf16 ulp off those of the
                        # expanded source.  So this one projection (the first step only) runs on the row count of the
                        # torch path; every sentence's rows are `beam` identical copies, of which the cache keeps one.
                        src16 = src16.unsqueeze(1).expand(bs // beam, beam, S, d).contiguous()
                    src16 = src16.view(-1, d)
                kvc = ops.gemm_nt(src16, cw.kv[i], L.EPI_BIAS, bias=cw.bkv[i])
                kvc = kvc.view(bs // beam, beam, S, 2 * d)[:, 0].contiguous() if beam > 1 else kvc.view(bs, S, 2 * d)
                if cache is not None:
                    cache[('cross', i)] = kvc
            res2 = ops.attn_cross_fwd(q2, kvc, src_klen, bs, n_new, H, dh, S) if xtiled else None
            if res2 is None:
                assert i == 0 or not xtiled
                xtiled = False
                ctx2 = ops.attn_query_fwd(q2, kvc, src_klen, bs, n_new, H, dh, S, owner=xowner)
            else:
                ctx2 = res2[0]
            pre = ops.gemm_nt(ctx2, cw.out[i], L.EPI_BIAS_DROP_RES, bias=cw.bo[i], aux=h16)
            ln15 = model.get_submodule('layer_norm15.%d' % i)
            h16, _, _ = ops.layernorm_fwd(pre, ln15.weight.detach(), ln15.bias.detach())
        u = torch.empty((bs * n_new, 4 * d), dtype=BF16, device=dev)
        hact = ops.gemm_nt(h16, ar.w(f + 'lin1.weight'), L.EPI_BIAS_GELU, bias=ar.p(f + 'lin1.bias'), out2=u)
        pre = ops.gemm_nt(hact, ar.w(f + 'lin2.weight'), L.EPI_BIAS_DROP_RES, bias=ar.p(f + 'lin2.bias'), aux=h16)
        h16, _, _ = ops.layernorm_fwd(pre, ar.p('layer_norm2.%d.weight' % i), ar.p('layer_norm2.%d.bias' % i), rowmask=rowmask)
    if cache is not None:
        cache['slen'] = pos0 + n_new
    return h16.view(bs, n_new, d).transpose(0, 1)


def word_logits16(model, tensor):
    """The logits of PredLayer.get_scores as the vocabulary GEMM leaves them: (n, d) -> (bf16 [n, V_pad], V); columns V ..
    V_pad - 1 are not written."""
    ar = model.arena()
    ar.refresh()
    V = model.n_words
    x16 = tensor.detach().to(BF16).reshape(-1, model.dim).contiguous()
    logits = torch.empty((x16.shape[0], ar.V_pad), dtype=BF16, device=x16.device)
    ops.gemm_nt(x16, ar.w('embeddings.weight'), L.EPI_BIAS, bias=ar.p('pred_layer.proj.bias'), out=logits, n=V)
    return logits, V


def word_scores(model, tensor):
    """PredLayer.get_scores (transformer.py:120-124): (n, d) -> (n, n_words) fp32 on the tied vocabulary matrix."""
    logits, V = word_logits16(model, tensor)
    return logits[:, :V].float()


def advance_owner(owner, beam_idx, next_pos):
    """The owner table after a beam step.  owner int32 [n, cap]: owner[r, p] = the cache row whose slot p holds position p
    of the hypothesis now in row r.  Row r continues the hypothesis of row beam_idx[r], so it inherits that row's map; the
    position the next step writes, next_pos, goes into every row's own slot.  A slot (row, position) is written once - by
    the step that decodes that position - and never again, so the slots a surviving hypothesis points to stay intact
    however the beams are re-ordered afterwards."""
    n = owner.shape[0]
    new = owner.index_select(0, beam_idx)
    new[:, next_pos] = torch.arange(n, dtype=owner.dtype, device=owner.device)
    return new


def _select(logits, V, beam_scores, beam, k, wide=False):
    name = 'vocab_select_wide' if wide else 'vocab_select'
    res = getattr(ops, name)(logits, V, beam_scores, beam, k)
    if res is None:
        raise L.M3PError('m3p_%s declined (M3P_ENOTIMPL) a shape m3p_%s_plan took' % (name, name))
    return res


def _sample_twin(scores, inv_t, seed, top_k, top_p=None):
    """The seeded draw on fp32 scores [bs, V] through the NumPy twin of m3p_vocab_sample / m3p_vocab_nucleus_sample (a CPU
    model, a shape the launcher declines, VOCAB_SELECT_MAX_K == 0) -> (words int64 [bs], logprob fp32 [bs]) on the scores' device."""
    words, logprob, _ = rng.sample_words(scores.detach().cpu().numpy(), inv_t, seed, top_k, top_p=top_p)
    return (torch.from_numpy(words).to(scores.device), torch.from_numpy(logprob.astype('float32')).to(scores.device))


def penalty_pair(repetition_penalty):
    """The two fp32 factors of the repetition penalty (include/m3p_hip.h: m3p_logits_constrain), as Python floats:
    (theta, inv_theta) = (fl32(penalty), fl32(1 / fl32(penalty))) - a positive logit is multiplied by inv_theta, every other by
    theta, in ONE fp32 multiply on every route.  None is off: (1.0, 1.0).  ValueError unless finite and > 0."""
    if repetition_penalty is None:
        return 1.0, 1.0
    theta = torch.tensor(float(repetition_penalty), dtype=torch.float32)
    inv = 1.0 / theta
    if not (math.isfinite(float(theta)) and float(theta) > 0.0 and math.isfinite(float(inv)) and float(inv) > 0.0):
        raise ValueError('repetition_penalty must be finite and > 0, got %r' % (repetition_penalty,))
    return float(theta), float(inv)


def constrain_scores_(scores, V, generated, cur_len, theta=1.0, inv_theta=1.0, ngram=0, eos=-1, banned=None):
    """The torch twin of m3p_logits_constrain (include/m3p_hip.h holds the contract; csrc/constrain.hip the kernel): plain
    torch, any device, IN PLACE on fp32 scores or bf16 logits [n, >= V]; returns `scores`.  It is the route of a model that is
    not on CUDA, of VOCAB_SELECT_MAX_K == 0 and of a shape the launcher declines.

    At the step that decodes position cur_len, row r has the history H = generated[1:cur_len, r], L = cur_len - 1 words; the
    <EOS> at position 0 (it serves as <BOS>) is not part of H.  In this order:
      1. every DISTINCT word w of H, 0 <= w < V:  x[w] <- bf16_rne(fl32(x[w] * (x[w] > 0 ? inv_theta : theta))), once however
         often w occurs ((theta, inv_theta) = penalty_pair(...); (1.0, 1.0) is off).  The penalised value is rounded to bf16 on
         fp32 scores too, so that the routes can be compared with torch.equal; 0, -0 and -inf keep their bits;
      2. ngram = n >= 1 (0: off): for every j in [0, L - n] with H[j + i] == H[L - n + 1 + i] for all i in [0, n - 2] the word
         H[j + n - 1] gets -inf (n = 1 bans every word of H; nothing happens while L < n; the suffix does not match itself);
      3. eos >= 0: that word gets -inf (the loops pass <EOS> while cur_len <= min_len);
      4. every id of `banned` (int64 tensor or None) gets -inf.
    A history word or banned id outside [0, V) is skipped; columns at or past V and everything else keep their bits."""
    n = scores.shape[0]
    assert scores.dim() == 2 and scores.shape[1] >= V and generated.shape[1] == n and 1 <= cur_len <= generated.shape[0]
    dev = scores.device
    H = generated[1:cur_len].t().to(dev)                                    # [n, L]
    Ln = cur_len - 1
    x = scores[:, :V]

    def marks(words, on):
        """bool [n, V]: the words of `words` [n, m] (where `on`) that lie inside [0, V)."""
        ok = on & (words >= 0) & (words < V)
        m = torch.zeros((n, V + 1), dtype=torch.bool, device=dev)
        m.scatter_(1, torch.where(ok, words, torch.full_like(words, V)), True)      # (skipped entries all land on column V)
        return m[:, :V]

    if (theta != 1.0 or inv_theta != 1.0) and Ln > 0:
        x32 = x.float()
        factor = torch.where(x32 > 0, torch.tensor(inv_theta, dtype=torch.float32, device=dev),
                             torch.tensor(theta, dtype=torch.float32, device=dev))
        pen = (x32 * factor).to(BF16).to(scores.dtype)
        x.copy_(torch.where(marks(H, torch.ones_like(H, dtype=torch.bool)), pen, x))
    ban = torch.zeros((n, V), dtype=torch.bool, device=dev)
    if ngram >= 1 and Ln >= ngram:
        win = H.unfold(1, ngram, 1)                                         # [n, L - n + 1, n]: j = 0 .. L - n
        match = (win[:, :, :ngram - 1] == H[:, None, Ln - ngram + 1:]).all(dim=2)
        ban |= marks(win[:, :, ngram - 1], match)
    if eos >= 0:
        assert eos < V
        ban[:, eos] = True
    if banned is not None and banned.numel():
        b = banned.to(dev).view(-1)
        ban[:, b[(b >= 0) & (b < V)]] = True
    x.masked_fill_(ban, float('-inf'))
    return scores


class _Constraints:
    """The decoding constraints of one generate / generate_beam call, validated once; `on` is False when all four are off
    (the loops then run exactly as they did without the keywords: no launch, no copy)."""

    def __init__(self, model, max_len, min_len, repetition_penalty, no_repeat_ngram, banned_words, dev):
        self.theta, self.inv_theta = penalty_pair(repetition_penalty)
        self.ngram, self.min_len = int(no_repeat_ngram or 0), int(min_len or 0)
        if self.ngram < 0:
            raise ValueError('no_repeat_ngram must be >= 0, got %r' % (no_repeat_ngram,))
        if self.min_len < 0 or self.min_len > max_len - 2:
            raise ValueError('min_len must lie in [0, max_len - 2] (position max_len - 1 is the forced <EOS>), got %r with '
                             'max_len %d' % (min_len, max_len))
        ids = sorted(set(int(w) for w in (banned_words if banned_words is not None else ())))
        for w in ids:
            if w < 0 or w >= model.n_words:
                raise ValueError('banned word %d is outside [0, n_words = %d)' % (w, model.n_words))
            if w == model.eos_index:
                raise ValueError('<EOS> (%d) cannot be banned: every sentence ends with it (use min_len)' % w)
        self.banned = torch.tensor(ids, dtype=torch.long, device=dev) if ids else None
        self.n_banned = len(ids)
        self.eos_index = int(model.eos_index)
        self.on = self.theta != 1.0 or self.inv_theta != 1.0 or self.ngram > 0 or self.min_len > 0 or self.n_banned > 0

    def args(self, cur_len):
        """The trailing arguments of ops.logits_constrain / constrain_scores_ at the step that decodes position cur_len."""
        return self.theta, self.inv_theta, self.ngram, self.eos_index if cur_len <= self.min_len else -1, self.banned

    def takes(self, n, V, ld, max_len):
        return ops.logits_constrain_takes(n, V, ld, max_len - 1, self.ngram, self.n_banned)


def _constrained_logits16(model, tensor, cons, on_device, generated, cur_len):
    """word_logits16 with the call's constraints applied in place: the kernel where its plan took the shape, else the twin."""
    logits, V = word_logits16(model, tensor)
    if cons.on:
        if on_device:
            if ops.logits_constrain(logits, V, generated, cur_len, *cons.args(cur_len)) is None:
                raise L.M3PError('m3p_logits_constrain declined (M3P_ENOTIMPL) a shape m3p_logits_constrain_plan took')
        else:
            constrain_scores_(logits, V, generated, cur_len, *cons.args(cur_len))
    return logits, V


def _constrained_scores(model, tensor, cons, generated, cur_len):
    """word_scores with the call's constraints applied by the twin (the torch routes)."""
    scores = word_scores(model, tensor)
    if cons.on:
        constrain_scores_(scores, model.n_words, generated, cur_len, *cons.args(cur_len))
    return scores


class _Prefix:
    """The forced target prefix of one generate / generate_beam call, validated once.  prefix int64 (P, bs), prefix_len (bs)
    with 0 <= prefix_len[b] <= P: sentence b starts <EOS>, prefix[0, b], ..., prefix[prefix_len[b] - 1, b].  `lo` / `hi` are
    the shortest / longest length; the loop prefills positions 0 .. lo in one decoder_forward call and forces the rest of the
    longer prompts step by step (`force`).  Both None: no prefix (`on` False, and the loops run exactly as without the keywords)."""

    def __init__(self, model, prefix, prefix_len, bs, max_len, dev, equal=False):
        self.on = prefix is not None
        self.lo = self.hi = 0
        if not self.on:
            if prefix_len is not None:
                raise ValueError('prefix_len needs prefix')
            return
        if prefix_len is None:
            raise ValueError('prefix needs prefix_len')
        prefix, plen = torch.as_tensor(prefix).to(dev).long(), torch.as_tensor(prefix_len).to(dev).long()
        if prefix.dim() != 2 or plen.dim() != 1 or prefix.size(1) != plen.size(0) or (bs is not None and plen.size(0) != bs):
            raise ValueError('prefix must be (P, bs) with prefix_len (bs), got %s and %s' % (tuple(prefix.shape), tuple(plen.shape)))
        P = prefix.size(0)
        if plen.numel() == 0:
            raise ValueError('prefix holds no sentence')
        self.lo, self.hi = int(plen.min()), int(plen.max())
        if self.lo < 0 or self.hi > P:
            raise ValueError('prefix_len must lie in [0, P = %d], got [%d, %d]' % (P, self.lo, self.hi))
        if equal and self.lo != self.hi:
            raise ValueError('beam search takes prefixes of equal length only (all prefix_len equal), got [%d, %d]'
                             % (self.lo, self.hi))
        if 1 + self.hi > max_len - 1:
            raise ValueError('the prefix is too long: 1 + max(prefix_len) = %d > max_len - 1 = %d (position max_len - 1 is the '
                             'forced <EOS>)' % (1 + self.hi, max_len - 1))
        inside = torch.arange(P, device=dev)[:, None] < plen[None, :]
        bad = inside & ((prefix == model.eos_index) | (prefix == model.pad_index) | (prefix < 0) | (prefix >= model.n_words))
        if bool(bad.any()):
            raise ValueError('a prefix word is <EOS>, pad or outside [0, n_words = %d)' % model.n_words)
        self.words, self.len = prefix, plen

    def fill(self, generated, rows_per_sentence=1):
        """The common part of the prompts into generated[1 : 1 + lo] -> the position the loop starts at."""
        if self.lo:
            generated[1:1 + self.lo] = self.words[:self.lo].repeat_interleave(rows_per_sentence, dim=1)
        return 1 + self.lo

    def force(self, next_words, cur_len, step_logprob=None):
        """The words of the step that decodes position cur_len, with the prompts that reach it put in place (log-probability 0)."""
        if cur_len > self.hi:
            return next_words, step_logprob
        forced = self.len >= cur_len
        if step_logprob is not None:
            step_logprob = step_logprob.masked_fill(forced, 0.0)
        return torch.where(forced, self.words[cur_len - 1].to(next_words.dtype), next_words), step_logprob


def generate(model, src_enc, src_len, tgt_lang_id, max_len=200, sample_temperature=None, sample_seed=None, sample_top_k=None,
             return_logprobs=False, sample_top_p=None, min_len=0, repetition_penalty=None, no_repeat_ngram=0, banned_words=None,
             prefix=None, prefix_len=None):
    """transformer.py:1216-1317: greedy (or temperature-sampled) decoding with the key / value cache.
    -> (generated (cur_len, bs) int64, gen_len (bs)).

    Without ``sample_seed`` this is the reference's loop: greedy, or ``torch.multinomial`` on torch's global generator when
    ``sample_temperature`` is given.  With ``sample_seed`` the words are drawn by the seeded Gumbel-max contract of
    include/m3p_hip.h (m3p_vocab_sample): ``sample_temperature`` defaults to 1.0, ``sample_top_k`` (None or 0: every word)
    restricts the draw to the row's top_k words, and the step that decodes position ``cur_len`` uses the stream key
    ``rng.stream_seed(sample_seed, cur_len, SAMPLE_SITE)``.  A CUDA model whose shape the launcher takes runs
    ``ops.vocab_sample`` on the bf16 logits, with 16 < top_k <= 1024 ``ops.vocab_sample_wide`` (the same contract by a count
    selection; ``sample_top_p`` rides along); everything else (a CPU model, top_k > 1024, VOCAB_SELECT_MAX_K == 0) runs the
    NumPy twin on ``word_scores`` - the same seed is the same random stream on both routes.  ``sample_top_p`` (seeded runs only;
    0 < p <= 1, None and any value >= 1.0 mean "off": every route is then bit for bit what it is without it) cuts the
    candidates (every word, or the top_k) to the nucleus of include/m3p_hip.h (m3p_vocab_nucleus_sample): the words whose
    logit is >= the largest logit value at which the mass cumulated from the top, under the tempered distribution over the
    candidates, reaches p - whole classes of equal logits, the row's maximum always among them.  The routes and the stream
    keys are the same (``ops.vocab_nucleus_sample`` or ``ops.vocab_sample_wide`` on the device, ``rng.sample_words(top_p=...)``
    as the twin).  Torch's CPU
    and CUDA generators are not touched, so a seeded run can be replayed exactly.  The counter of the random stream is (row of
    the batch, word): a sentence's draw depends on its position in the batch.  ``return_logprobs`` (seeded runs only) adds a
    third value, fp32 (cur_len, bs): the log-probability, under the tempered, top-k and nucleus-truncated distribution, of
    each sampled word; 0 at position 0, at pad positions and where <EOS> was forced at ``max_len``.

    Decoding constraints (the contract is in include/m3p_hip.h: m3p_logits_constrain; all four off by default, and then every
    route is bit for bit what it is without the keywords, with no launch added).  At the step that decodes position
    ``cur_len`` row r has the history ``generated[1:cur_len, r]`` (the <EOS> at position 0 is not part of it), and its logits
    are changed in this order: ``repetition_penalty`` theta (finite, > 0; None or 1.0: off) multiplies the logit of every
    distinct history word by 1 / theta if it is positive and by theta otherwise, rounded to bf16; ``no_repeat_ngram`` n (0: off)
    gives -inf to every word that would complete an n-gram the history already holds; ``min_len`` gives -inf to <EOS> while
    cur_len <= min_len, so every sentence has at least min_len words between its two <EOS> (min_len <= max_len - 2);
    ``banned_words`` (ids in [0, n_words), not <EOS>) get -inf.  Where the words are selected on the device
    (``ops.vocab_select`` / ``vocab_sample`` / ``vocab_nucleus_sample`` / ``vocab_sample_wide``) and ``ops.logits_constrain_takes`` the shape (asked
    once, with max_len - 1 as the history bound), ``ops.logits_constrain`` edits the bf16 logits in place - one launch per
    step - and the selection runs unchanged behind it; a declined shape gets the twin ``constrain_scores_`` on those logits, and
    every torch route (greedy, seeded, ``torch.multinomial``) the twin on ``word_scores``.  Log-probabilities are those of the
    constrained distribution.

    Prompted decoding: ``prefix`` int64 (P, bs) with ``prefix_len`` (bs), 0 <= prefix_len[b] <= P, forces the first words of
    every sentence: ``generated[1 : 1 + prefix_len[b], b] = prefix[:prefix_len[b], b]`` behind the leading <EOS>.  A prefix
    word inside its length that is <EOS>, pad or outside [0, n_words), and 1 + max(prefix_len) > max_len - 1, raise
    ValueError.  With a prefix ``src_enc = src_len = None`` is allowed (a zero-length prefix too: it gives bs): the model
    then decodes without the encoder-attention sub-layer - generation from a causal language model.  The ragged rule: the
    loop starts at cur_len = 1 + min(prefix_len), and its first ``decoder_forward`` call covers positions 0 .. cur_len - 1 at
    once - the prefill, on the tiled prefix kernel from ``PREFILL_TILED_MIN_T`` positions on; only this common part of the
    prompts is prefilled.  The rest of the longer prompts is forced step by step: at the step that decodes position cur_len
    the rows with 1 + prefix_len[b] > cur_len take ``prefix[cur_len - 1, b]`` in place of the selected word, on every route
    (the selection still runs for the whole batch: stream keys and counters are those of the unprompted call).  Returned
    log-probabilities are 0 at prefix positions.  The constraints' history is ``generated[1:cur_len]``, prefix included, and
    ``min_len`` counts prefix words.  Without ``prefix`` nothing changes by a bit."""
    seeded = sample_seed is not None
    if sample_top_k is not None and not seeded:
        raise ValueError('sample_top_k needs sample_seed: the torch sampling path has no top-k mode')
    if return_logprobs and not seeded:
        raise ValueError('return_logprobs needs sample_seed')
    if sample_top_p is not None and not seeded:
        raise ValueError('sample_top_p needs sample_seed: the torch sampling path has no top-p mode')
    top_p = rng.nucleus_top_p(sample_top_p)                  # (None: off; <= 0 or NaN raises ValueError)
    top_k = int(sample_top_k or 0)
    if top_k < 0:
        raise ValueError('sample_top_k must be >= 0, got %r' % (sample_top_k,))
    dev = model.embeddings.weight.device
    if (src_enc is None) != (src_len is None):
        raise ValueError('src_enc and src_len come together (both None: decoder-only generation from a prefix)')
    if src_enc is None and prefix is None:
        raise ValueError('generation without a source encoding needs a prefix (a zero-length one gives the batch size)')
    bs = len(src_len) if src_len is not None else int(torch.as_tensor(prefix_len).numel()) if prefix_len is not None else None
    assert src_enc is None or src_enc.size(0) == bs
    pre = _Prefix(model, prefix, prefix_len, bs, max_len, dev)
    cons = _Constraints(model, max_len, min_len, repetition_penalty, no_repeat_ngram, banned_words, dev)
    if src_len is not None:
        src_len = src_len.to(dev)
    generated = torch.full((max_len, bs), model.pad_index, dtype=torch.long, device=dev)
    generated[0].fill_(model.eos_index)                       # <EOS> doubles as <BOS>
    positions = torch.arange(max_len, device=dev)[:, None].expand(max_len, bs)
    langs = None
    if tgt_lang_id is not None:
        langs = torch.full((max_len, bs), int(tgt_lang_id), dtype=torch.long, device=dev)
    cur_len = pre.fill(generated)          # (1 without a prefix; else the first call covers positions 0 .. cur_len - 1: the prefill)
    gen_len = torch.full((bs,), cur_len, dtype=torch.long, device=dev)
    unfinished = torch.ones(bs, dtype=torch.long, device=dev)
    cache = {'slen': 0, 'max_len': max_len, 'tiled_prefill': True}
    # (a launcher that would answer M3P_ENOTIMPL - it is asked once, the answer depends on the shape alone - leaves the torch path)
    select = (sample_temperature is None and not seeded and dev.type == 'cuda' and VOCAB_SELECT_MAX_K >= 1
              and ops.vocab_select_takes(bs, model.n_words, model.arena().V_pad, 1, 1))
    if seeded:
        temperature = 1.0 if sample_temperature is None else float(sample_temperature)
        inv_t = rng.inv_temperature(temperature)
        top_k = min(top_k, model.n_words)
        # the device route, picked once: (launcher, its plan, the op, the op's arguments behind the seed).  Up to 16 candidates or
        # every word go by rounds of a maximum, with or without the nucleus cut; more than 16, where that plan declined, by the
        # count selection.  Each plan is asked once.
        routes = [('m3p_vocab_sample', ops.vocab_sample_takes, ops.vocab_sample, (top_k,)) if top_p is None else
                  ('m3p_vocab_nucleus_sample', ops.vocab_nucleus_takes, ops.vocab_nucleus_sample, (top_p, top_k))]
        if top_k >= 1:
            routes.append(('m3p_vocab_sample_wide', ops.vocab_sample_wide_takes, ops.vocab_sample_wide, (top_k, top_p)))
        on_dev = dev.type == 'cuda' and VOCAB_SELECT_MAX_K >= 1
        draw = next((r for r in routes if on_dev and r[1](bs, model.n_words, model.arena().V_pad, top_k)), None)
        sample_dev = draw is not None
        logprobs = torch.zeros((max_len, bs), dtype=torch.float32, device=dev) if return_logprobs else None
    # (the constraint kernel sits in front of a device selection only; its plan is asked once, like the others)
    cons_dev = (cons.on and (sample_dev if seeded else select)
                and cons.takes(bs, model.n_words, model.arena().V_pad, max_len))
    while cur_len < max_len:
        tensor = decoder_forward(model, generated[:cur_len], gen_len, src_enc, src_len, positions[:cur_len],
                                 None if langs is None else langs[:cur_len], cache)
        assert tensor.size()[1:] == (bs, model.dim) and tensor.size(0) in (1, cur_len)      # (cur_len rows: the prefill)
        step_logprob = None
        if seeded:
            step_seed = rng.stream_seed(sample_seed, cur_len, SAMPLE_SITE)
            if sample_dev:
                logits, V = _constrained_logits16(model, tensor[-1], cons, cons_dev, generated, cur_len)
                res = draw[2](logits, V, temperature, step_seed, *draw[3])
                if res is None:
                    raise L.M3PError('%s declined (M3P_ENOTIMPL) a shape its plan took' % draw[0])
                next_words, step_logprob = res[0], res[1]
            else:
                next_words, step_logprob = _sample_twin(_constrained_scores(model, tensor[-1], cons, generated, cur_len), inv_t,
                                                        step_seed, top_k, top_p)
        elif select:                   # the first maximum of each row, from the bf16 logits
            logits, V = _constrained_logits16(model, tensor[-1], cons, cons_dev, generated, cur_len)
            next_words = _select(logits, V, None, 1, 1)[1].squeeze(1)
        elif sample_temperature is None:
            next_words = torch.topk(_constrained_scores(model, tensor[-1], cons, generated, cur_len), 1)[1].squeeze(1)
        else:
            scores = _constrained_scores(model, tensor[-1], cons, generated, cur_len)
            next_words = torch.multinomial(torch.softmax(scores / sample_temperature, dim=1), 1).squeeze(1)
        if pre.on:                     # rows whose prompt reaches this position take its word, on every route
            next_words, step_logprob = pre.force(next_words, cur_len, step_logprob)
        if return_logprobs:
            logprobs[cur_len] = step_logprob.masked_fill(unfinished == 0, 0.0)
        generated[cur_len] = next_words * unfinished + model.pad_index * (1 - unfinished)
        gen_len.add_(unfinished)
        unfinished.mul_(next_words.ne(model.eos_index).long())
        cur_len += 1
        if int(unfinished.max()) == 0:          # (one host read per step, as in the reference)
            break
    if cur_len == max_len:
        generated[-1].masked_fill_(unfinished.bool(), model.eos_index)
        if return_logprobs:
            logprobs[-1].masked_fill_(unfinished.bool(), 0.0)        # (a forced <EOS> was not drawn)
    assert int((generated == model.eos_index).sum()) == 2 * bs
    if return_logprobs:
        return generated[:cur_len], gen_len, logprobs[:cur_len]
    return generated[:cur_len], gen_len


class BeamHypotheses(object):
    """The n best finished hypotheses of one sentence, ranked by length-normalised log-probability (the bookkeeping of
    transformer.py:1518-1561).  A bounded min-heap keyed on (score, arrival order): the root is the entry the next better
    hypothesis evicts, `worst_score` is the root's score; among equal scores the earliest arrival goes first, which is
    the tie-break of the reference's sort."""

    def __init__(self, n_hyp, max_len, length_penalty, early_stopping):
        self.n_hyp, self.early_stopping = n_hyp, early_stopping
        self.length_penalty = length_penalty
        self._norm = float(max_len - 1) ** length_penalty      # longest possible hypothesis (without <BOS>)
        self._heap, self._arrivals = [], 0

    def __len__(self):
        return len(self._heap)

    @property
    def hyp(self):
        """[(score, tokens)] in arrival order."""
        return [(s, t) for s, _, t in sorted(self._heap, key=lambda e: e[1])]

    @property
    def worst_score(self):
        return self._heap[0][0] if self._heap else 1e9

    def best(self):
        """Tokens of the best hypothesis (the earliest among equals)."""
        return max(self._heap, key=lambda e: (e[0], -e[1]))[2]

    def add(self, hyp, sum_logprobs):
        entry = (sum_logprobs / len(hyp) ** self.length_penalty, self._arrivals, hyp)
        self._arrivals += 1
        if len(self._heap) < self.n_hyp:
            heapq.heappush(self._heap, entry)
        elif entry[0] > self._heap[0][0]:
            heapq.heapreplace(self._heap, entry)

    def is_done(self, best_sum_logprobs):
        """Can no open beam still enter the list?  (always, once it is full, under early stopping)"""
        full = len(self._heap) >= self.n_hyp
        return full and (self.early_stopping or self.worst_score >= best_sum_logprobs / self._norm)


HYP_STATE = ('hyp_tok', 'hyp_len', 'hyp_score', 'hyp_sum', 'hyp_arrival', 'hyp_count', 'arrivals', 'done', 'status')


def beam_norms(max_len, length_penalty):
    """The two normalisers of the bookkeeping, in double precision as CPython computes them: (norm fp64 [max_len + 1] with
    norm[l] = float(l) ** length_penalty - a hypothesis of l tokens scores sum_logprobs / norm[l] -, float(max_len - 1) **
    length_penalty of BeamHypotheses.is_done).  norm[0] is never read; a negative penalty makes it inf."""
    def power(l):
        try:
            return float(l) ** length_penalty
        except ZeroDivisionError:
            return float('inf')
    return np.array([power(l) for l in range(max_len + 1)], dtype=np.float64), power(max_len - 1)


def beam_state_host(bs, beam, max_len, pad):
    """The empty hypothesis state of bs sentences as NumPy arrays (ops.beam_state makes the same on the device): per sentence a
    list of up to `beam` finished hypotheses in slots 0 .. hyp_count - 1 -
      hyp_tok int64 [bs, beam, max_len] (tokens 0 .. hyp_len - 1, pad behind them), hyp_len int32 [bs, beam],
      hyp_score fp64 [bs, beam] (sum / norm[len]), hyp_sum fp32 [bs, beam], hyp_arrival int32 [bs, beam],
    hyp_count int32 [bs], arrivals int32 [bs] (hypotheses offered so far: the next arrival number), done uint8 [bs], status
    int32 [bs] (nonzero: a step found fewer than `beam` continuations)."""
    z = lambda shape, dt: np.zeros(shape, dtype=dt)   # noqa: E731
    return dict(hyp_tok=np.full((bs, beam, max_len), pad, dtype=np.int64), hyp_len=z((bs, beam), np.int32),
                hyp_score=z((bs, beam), np.float64), hyp_sum=z((bs, beam), np.float32), hyp_arrival=z((bs, beam), np.int32),
                hyp_count=z((bs,), np.int32), arrivals=z((bs,), np.int32), done=z((bs,), np.uint8), status=z((bs,), np.int32))


def beam_advance_host(next_scores, flat_idx, generated, state, cur_len, max_len, eos, pad, V, beam, early_stopping, norm,
                      norm_max):
    """The hypothesis bookkeeping of one beam-search step (transformer.py:1420-1470 with BeamHypotheses.add / is_done) as one
    function over plain arrays: the code the host routes of generate_beam run, and the twin ops.beam_advance (csrc/beam.hip)
    has to equal bit for bit.

    next_scores fp32 [bs, k], flat_idx int64 [bs, k]: every sentence's candidates in the selection's order (score descending:
    entry 0 is the maximum), flat_idx = beam * V + word.  generated int64 [>= cur_len, bs * beam]: the tokens so far.  `state`
    (beam_state_host) is updated IN PLACE; (norm, norm_max) = beam_norms(max_len, length_penalty).
    -> (beam_scores fp32 [bs * beam], beam_words int64 [bs * beam], beam_idx int64 [bs * beam]).

    Per sentence s:  done[s] |= the list is full and (early_stopping or its worst score >= next_scores[s, 0] / norm_max).  A
    done sentence emits beam x (0.0, pad, row 0) and changes nothing.  Otherwise the candidates are taken in order: an <EOS>
    candidate - every candidate when cur_len + 1 == max_len - is offered to the list with score = value / norm[cur_len] and
    the next arrival number: while the list holds fewer than `beam` entries it takes the next slot, afterwards it replaces the
    entry that is minimal by (score, arrival), and only if its score is strictly larger.  Every other candidate continues
    the search: (value, word, row s * beam + its beam); the walk stops at `beam` of them.  Fewer than `beam` (on the last step:
    none) are filled up with (0.0, pad, row 0), and before the last step that sets status[s].  All score arithmetic is fp64 on
    the fp32 candidate value."""
    scores_h, idx_h = np.asarray(next_scores, dtype=np.float32).tolist(), np.asarray(flat_idx).tolist()
    bs = len(scores_h)
    last = cur_len + 1 == max_len
    norm_len = float(norm[cur_len])
    hyp_score, hyp_arrival, hyp_count, done = state['hyp_score'], state['hyp_arrival'], state['hyp_count'], state['done']
    out_scores, out_words, out_idx = [], [], []
    for s in range(bs):
        count = int(hyp_count[s])
        if not done[s] and count >= beam:
            if early_stopping or float(hyp_score[s, :count].min()) >= scores_h[s][0] / norm_max:
                done[s] = 1
        if done[s]:
            out_scores += [0.0] * beam
            out_words += [pad] * beam
            out_idx += [0] * beam
            continue
        found = 0
        for value, idx in zip(scores_h[s], idx_h[s]):
            beam_id, word = idx // V, idx % V
            if word == eos or last:
                score = value / norm_len
                arrival = int(state['arrivals'][s])
                state['arrivals'][s] = arrival + 1
                if count < beam:
                    slot = count
                    count += 1
                else:
                    slot = min(range(beam), key=lambda j: (hyp_score[s, j], hyp_arrival[s, j]))
                    if not score > hyp_score[s, slot]:
                        slot = -1
                if slot >= 0:
                    state['hyp_tok'][s, slot, :] = pad
                    state['hyp_tok'][s, slot, :cur_len] = generated[:cur_len, s * beam + beam_id]
                    state['hyp_len'][s, slot] = cur_len
                    hyp_score[s, slot] = score
                    state['hyp_sum'][s, slot] = value
                    hyp_arrival[s, slot] = arrival
            else:
                out_scores.append(value)
                out_words.append(word)
                out_idx.append(s * beam + beam_id)
                found += 1
            if found == beam:
                break
        hyp_count[s] = count
        if found < beam:
            if not last:
                state['status'][s] = 1
            out_scores += [0.0] * (beam - found)
            out_words += [pad] * (beam - found)
            out_idx += [0] * (beam - found)
    return np.array(out_scores, dtype=np.float32), np.array(out_words, dtype=np.int64), np.array(out_idx, dtype=np.int64)


# Dispatch of the hypothesis bookkeeping, like VOCAB_SELECT_MAX_K: on the select routes, where ops.beam_advance_takes the shape
# (beam <= 32, 2 * beam <= 64, max_len <= 1025), True runs every step's bookkeeping on the device (ops.beam_advance,
# csrc/beam.hip: no per-step host copy, one blocking read per call); False keeps beam_advance_host behind one host copy per
# step.  Both give the same tokens, lengths, n-best lists and score bits (tests/test_beam_nbest.py).  Measured, the device
# side is faster in every pair at 32 x beam 4, 64 x beam 5 and 16 x beam 32 (0.38 - 0.45 ms per step; DESIGN.md 4,
# "Hypothesis bookkeeping on the device"; profiles/decode_beam_device_hyps.txt).  It ships False all the same: with it the loop
# stops whenever the host happens to notice that every sentence is done, so the NUMBER of steps differs from run to run, and
# it re-orders the owner table without advance_owner - tests/test_beam_cache.py and tests/test_beam_wide.py observe the select
# route through exactly these two (per-step logs of two runs compared entry by entry; a spy on advance_owner).
BEAM_HYPS_ON_DEVICE = False


def _host_read(*tensors):
    """Every blocking device-to-host read of generate_beam's loop goes through here (a test counts the calls): NumPy copies."""
    out = tuple(t.cpu().numpy() for t in tensors)
    return out[0] if len(out) == 1 else out


def _beam_result(state, n_best, return_scores, eos, pad, dev):
    """The call's return value from the final hypothesis state (NumPy): per sentence its n_best finished hypotheses by score
    descending, then arrival ascending."""
    if int(state['status'].max()) != 0:
        raise L.M3PError('beam search: a step found fewer than beam_size continuations among its 2 * beam_size candidates '
                         '(sentences %s)' % state['status'].nonzero()[0].tolist())
    bs = state['hyp_count'].shape[0]
    assert int(state['hyp_count'].min()) >= n_best
    tgt_len = np.zeros((bs, n_best), dtype=np.int64)
    scores = np.zeros((bs, n_best), dtype=np.float64)
    order = []
    for s in range(bs):
        sc, arr = state['hyp_score'][s].tolist(), state['hyp_arrival'][s].tolist()
        order.append(sorted(range(int(state['hyp_count'][s])), key=lambda j: (-sc[j], arr[j]))[:n_best])
        for j, slot in enumerate(order[s]):
            tgt_len[s, j] = int(state['hyp_len'][s, slot]) + 1              # + <EOS>
            scores[s, j] = sc[slot]
    decoded = np.full((int(tgt_len.max()), bs, n_best), pad, dtype=np.int64)
    for s in range(bs):
        for j, slot in enumerate(order[s]):
            n = int(tgt_len[s, j]) - 1
            decoded[:n, s, j] = state['hyp_tok'][s, slot, :n]
            decoded[n, s, j] = eos
    assert int((decoded == eos).sum()) == 2 * bs * n_best
    if n_best == 1:
        decoded, tgt_len, scores = decoded[:, :, 0], tgt_len[:, 0], scores[:, 0]
    res = (torch.from_numpy(np.ascontiguousarray(decoded)).to(dev), torch.from_numpy(np.ascontiguousarray(tgt_len)).to(dev))
    if return_scores:
        res += (torch.from_numpy(np.ascontiguousarray(scores)).to(dev),)
    return res


def generate_beam(model, src_enc, src_len, tgt_lang_id, beam_size, length_penalty, early_stopping, max_len=200, min_len=0,
                  repetition_penalty=None, no_repeat_ngram=0, banned_words=None, n_best=1, return_scores=False, prefix=None,
                  prefix_len=None):
    """transformer.py:1319-1515: beam search; the beam is folded into the batch dimension (bs * beam_size rows).  On the torch
    path the key / value caches are re-ordered by the surviving beams' source rows after every step; on the select path
    (module docstring: ``ops.vocab_select`` up to 8 beams, ``ops.vocab_select_wide`` from 9 to 32) they stay in place behind
    cache['owner'] and the source is kept once per sentence.
    -> (decoded (max tgt_len, bs) int64, tgt_len (bs)).

    ``n_best`` = k (1 <= k <= beam_size, ValueError otherwise): every sentence ends with beam_size finished hypotheses (the
    last step finishes every candidate), and with k > 1 the call returns the k best of them - decoded (max tgt_len, bs, k)
    int64, pad-filled, tgt_len (bs, k); hypothesis j of a sentence is its j-th by score descending, then arrival ascending
    (the order of ``BeamHypotheses.best``: [..., 0] is the result of the default call).  ``return_scores`` appends scores, fp64
    (bs,) or (bs, k): sum of log-probabilities / len(hypothesis) ** length_penalty, as ``BeamHypotheses.add`` computes it.

    The hypothesis bookkeeping of a step is ``beam_advance_host`` behind one host copy of the candidates on every route, or,
    on the select path with ``BEAM_HYPS_ON_DEVICE`` where ``ops.beam_advance_takes`` the shape, ``ops.beam_advance``
    (csrc/beam.hip): the lists, the next beams, the next ``generated`` columns and the owner table are then written by one
    launch per step, `generated` and the owner table double-buffered; the host learns that every sentence is done from
    asynchronous copies of `done` it only looks at once they have arrived - steps issued meanwhile change nothing, a done
    sentence is frozen - and reads the lists once, at the end (``_host_read``).

    ``min_len`` / ``repetition_penalty`` / ``no_repeat_ngram`` / ``banned_words``: the decoding constraints of ``generate``, by
    the same contract and the same routes, per hypothesis row (the history of a row is the hypothesis it continues).  The edit
    happens on the logits before the row's log-sum-exp: the scores are log_softmax of the constrained logits plus the beam
    score.  All four off: no route changes by a bit.

    ``prefix`` / ``prefix_len``: the forced target prefix of ``generate``, by the same rules, but all prefix_len must be equal
    (ValueError otherwise); ``src_enc = src_len = None`` is allowed with it.  The loop starts at cur_len = 1 + prefix_len and
    its first call prefills positions 0 .. cur_len - 1 on the expanded bs * beam_size rows (the select routes read the cache
    through the owner table and keep the rows kernel for it).  Beam scores start as without a prefix - the prefix adds 0 -
    so a hypothesis' score is the sum of the GENERATED words' log-probabilities over its total length, prefix included, to
    the power length_penalty.  Without ``prefix`` nothing changes by a bit."""
    assert beam_size >= 1
    if (src_enc is None) != (src_len is None):
        raise ValueError('src_enc and src_len come together (both None: decoder-only generation from a prefix)')
    if src_enc is None and prefix is None:
        raise ValueError('generation without a source encoding needs a prefix (a zero-length one gives the batch size)')
    assert src_enc is None or src_enc.size(0) == src_len.size(0)
    if isinstance(n_best, bool) or not isinstance(n_best, int) or not 1 <= n_best <= beam_size:
        raise ValueError('n_best must be an integer in [1, beam_size = %d], got %r' % (beam_size, n_best))
    bs = len(src_len) if src_len is not None else int(torch.as_tensor(prefix_len).numel()) if prefix_len is not None else None
    n_words = model.n_words
    dev = model.embeddings.weight.device
    pre = _Prefix(model, prefix, prefix_len, bs, max_len, dev, equal=True)
    cons = _Constraints(model, max_len, min_len, repetition_penalty, no_repeat_ngram, banned_words, dev)
    n = bs * beam_size
    sel_k = 2 * beam_size
    # (each plan is asked once; sel_k > n_words is malformed for the wide entry - a row supplies at most V entries to its own
    # first k - and takes the torch path)
    wide = BEAM_SELECT_WIDE_MIN_K <= sel_k <= min(BEAM_SELECT_WIDE_MAX_K, n_words)
    if dev.type != 'cuda' or VOCAB_SELECT_MAX_K < 1:
        select = wide = False
    elif sel_k < BEAM_SELECT_WIDE_MIN_K:
        select = sel_k <= VOCAB_SELECT_MAX_K and ops.vocab_select_takes(n, n_words, model.arena().V_pad, beam_size, sel_k)
    else:
        select = wide = wide and ops.vocab_select_wide_takes(n, n_words, model.arena().V_pad, beam_size, sel_k)
    cons_dev = cons.on and select and cons.takes(n, n_words, model.arena().V_pad, max_len)
    hyps_dev = bool(select and BEAM_HYPS_ON_DEVICE and max_len >= 2 and ops.beam_advance_takes(bs, beam_size, sel_k, max_len))
    if src_enc is None:
        pass
    elif select:
        src_enc = src_enc.to(dev)
    else:
        src_enc = src_enc.to(dev).unsqueeze(1).expand((bs, beam_size) + src_enc.shape[1:]).contiguous().view(
            (bs * beam_size,) + src_enc.shape[1:])
    if src_len is not None:
        src_len = src_len.to(dev).unsqueeze(1).expand(bs, beam_size).contiguous().view(-1)
    generated = torch.full((max_len, bs * beam_size), model.pad_index, dtype=torch.long, device=dev)
    generated[0].fill_(model.eos_index)
    positions = torch.arange(max_len, device=dev)[:, None].expand_as(generated)
    # (the reference always builds language ids here, :1370 - a model without language embeddings cannot take them)
    langs = positions.clone().fill_(int(tgt_lang_id)) if tgt_lang_id is not None else None
    beam_scores = torch.zeros((bs, beam_size), dtype=torch.float32, device=dev)
    beam_scores[:, 1:] = -1e9
    beam_scores = beam_scores.view(-1)
    cur_len = pre.fill(generated, beam_size)      # (1 without a prefix; else the first call is the prefill of every row)
    cache = {'slen': 0, 'max_len': max_len, 'tiled_prefill': True}
    if select:
        cache['beam'] = beam_size
        cache['owner'] = torch.arange(n, dtype=torch.int32, device=dev)[:, None].expand(n, max_len).contiguous()
    norm, norm_max = beam_norms(max_len, length_penalty)
    eos, pad = int(model.eos_index), int(model.pad_index)

    def step_candidates(generated):
        lengths = torch.full((bs * beam_size,), cur_len, dtype=torch.long, device=dev)
        tensor = decoder_forward(model, generated[:cur_len], lengths, src_enc, src_len, positions[:cur_len],
                                 None if langs is None else langs[:cur_len], cache)
        assert tensor.size()[1:] == (bs * beam_size, model.dim) and tensor.size(0) in (1, cur_len)
        if select:
            next_scores, next_words, _ = _select(*_constrained_logits16(model, tensor[-1], cons, cons_dev, generated, cur_len),
                                                 beam_scores, beam_size, sel_k, wide)
        else:
            scores = torch.log_softmax(_constrained_scores(model, tensor[-1], cons, generated, cur_len), dim=-1)
            _scores = (scores + beam_scores[:, None]).view(bs, beam_size * n_words)
            next_scores, next_words = torch.topk(_scores, 2 * beam_size, dim=1, largest=True, sorted=True)
        return next_scores, next_words

    if hyps_dev:
        state = ops.beam_state(bs, beam_size, max_len, pad, dev)
        norm_dev = torch.from_numpy(norm).to(dev)
        spare = generated.clone()                                   # `generated` and the owner table: read one, write the other
        spare_owner = cache['owner'].clone()
        slots = torch.empty((max_len, bs), dtype=torch.uint8).pin_memory()
        pending, stop = collections.deque(), False
        while cur_len < max_len:
            while pending and pending[0][0].query():                # copies of `done` that have arrived; never waited for
                stop = bool(pending.popleft()[1].all()) or stop
            if stop:
                break
            next_scores, next_words = step_candidates(generated)
            res = ops.beam_advance(next_scores, next_words, generated, spare, cache['owner'], spare_owner, state, cur_len,
                                   max_len, eos, pad, n_words, beam_size, early_stopping, norm_dev, norm_max)
            if res is None:
                raise L.M3PError('m3p_beam_advance declined (M3P_ENOTIMPL) a shape m3p_beam_advance_plan took')
            beam_scores = res[0]
            generated, spare = spare, generated
            cache['owner'], spare_owner = spare_owner, cache['owner']
            slots[cur_len].copy_(state['done'], non_blocking=True)
            event = torch.cuda.Event()
            event.record()
            pending.append((event, slots[cur_len]))
            cur_len += 1
        state = dict(zip(HYP_STATE, _host_read(*[state[name] for name in HYP_STATE])))
        return _beam_result(state, n_best, return_scores, eos, pad, dev)

    state = beam_state_host(bs, beam_size, max_len, pad)
    generated_h = generated.cpu().numpy()                           # the host's mirror of `generated`: what a finished hypothesis copies
    while cur_len < max_len:
        next_scores, next_words = step_candidates(generated)
        next_scores_h, next_words_h = _host_read(next_scores, next_words)           # one host copy per step
        scores_h, words_h, idx_h = beam_advance_host(next_scores_h, next_words_h, generated_h, state, cur_len, max_len, eos, pad,
                                                     n_words, beam_size, early_stopping, norm, norm_max)
        assert not state['status'].any(), 'fewer than beam_size continuations among 2 * beam_size candidates'
        generated_h = generated_h[:, idx_h]
        generated_h[cur_len] = words_h
        beam_scores = torch.from_numpy(scores_h).to(dev)
        beam_words = torch.from_numpy(words_h).to(dev)
        beam_idx = torch.from_numpy(idx_h).to(dev)
        generated = generated[:, beam_idx]
        generated[cur_len] = beam_words
        if select:                                         # key / value tensors stay; the map to them follows the beams
            cache['owner'] = advance_owner(cache['owner'], beam_idx, cur_len)
        else:
            for k in list(cache.keys()):
                if isinstance(k, tuple):                   # key / value tensors follow their beams
                    cache[k] = cache[k].index_select(0, beam_idx)
        cur_len += 1
        if state['done'].all():
            break
    return _beam_result(state, n_best, return_scores, eos, pad, dev)
