"""Validation scoring on the GPU: ce_eval_kernel (csrc/heads.hip), TransformerModel.predict_stats, and the evaluation loops
of m3p_amd/evaluation.py end to end against the oracle.  Run with -s to see each figure before it is asserted."""
import math
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from m3p_amd import synth
from oracle import ref_cpu
from tests.util import F32_OUT, assert_gemm_bound, poisoned_outputs

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16

LOSS_RTOL = 5e-3        # the project's loss bar
MARGIN = 0.02           # oracle top-2 margin under which bf16 scores may land on the other word (tests/test_decoder.py)
MAX_EXCLUDED = 0.10     # share of a batch's rows that may fall under it


# ------------------------------------------------------------------------------------------------ the kernel
def _planted_logits(n, V, seed):
    """bf16 logits [n, ld > V] drawn in fp32 (N(0, 3)) and rounded, int64 targets, with rows planted for the cases the lowest-
    index rule and the pad columns must get right.  Thread t of the row's block reads the 8-column groups t, t + 1024, ...;
    wave w of the first trip covers columns [512 w, 512 w + 512)."""
    ld = (V + 255) // 256 * 256 if V % 256 else V + 64
    gen = torch.Generator(device='cuda').manual_seed(seed)
    logits = (torch.randn((n, ld), generator=gen, device='cuda', dtype=torch.float32) * 3.0).to(BF16)
    y = torch.randint(0, V, (n,), generator=gen, device='cuda')
    top = 30.0                                          # exact in bf16, above every draw
    plants = [
        [5, 2],                                         # two maxima inside one 16-byte group
        [8 * 3 + 1, 8 * 40],                            # ... in two threads of one wave
        [3000, 600, 1500],                              # three, in three waves
        [8 * (7 + 2048) + 1, 8 * 7 + 3],                # ... in two chunks of one thread (trips 0 and 2)
        [8 * (5 + 1024), 8 * 900 + 2],                  # a low thread's later chunk against a high thread's first: 7202 wins
        [0],                                            # the maximum at column 0
        [V - 1],                                        # ... at column V - 1
        [V - 1, 0],                                     # both ends
    ]
    want = {}
    for r, cols in enumerate(plants):
        cols = [c for c in cols if c < V]
        if r >= n or not cols:
            continue
        logits[r, cols] = top
        want[r] = min(cols)
    # pad columns [V, ld): a larger finite value, +inf, NaN - row by row - which must never be seen
    pad = logits[:, V:]
    pad[0::3] = 60.0
    pad[1::3] = float('inf')
    pad[2::3] = float('nan')
    # targets: on the argmax for the planted column-0 row, off it for the others; the random rows have both kinds
    for r, c in want.items():
        y[r] = c if r == 5 else (c + 1) % V
    return logits, y, ld, want


def _loss_bound(row_loss, x64, y, V, what):
    """The bound of tests/test_small_kernels.py::_ce_bounds on the row losses, restated: an fp64 log-sum-exp as the reference;
    a sum of V positive terms with fp32 exp (a depth-V sum of O(1) relative error), 2^-20 absolute for the fast exp / log,
    and the fp32 rounding of lse and of the target logit the loss is the difference of."""
    lse = torch.logsumexp(x64, -1)
    xt = x64.gather(1, y[:, None])[:, 0]
    return assert_gemm_bound(row_loss, lse - xt, torch.ones_like(lse), V, F32_OUT, F32_OUT * (lse.abs() + xt.abs()) + 2.0 ** -20,
                             what=what + ' row loss')


def _lowest_argmax(x):
    """The contract, computed by torch on the stored values: the lowest column at which the row's maximum is attained."""
    V = x.shape[1]
    cols = torch.arange(V, device=x.device)[None, :]
    return torch.where(x == x.max(1, keepdim=True)[0], cols, torch.full_like(cols, V)).min(1)[0]


@pytest.mark.parametrize('n,V', [(1, 64), (9, 1000), (33, 4100), (70, 250002), (4864, 250002)])
def test_ce_eval_kernel(n, V):
    from m3p_amd import ops
    logits, y, ld, want = _planted_logits(n, V, seed=11 + n)
    assert ld > V and ld % 8 == 0 and logits.stride(0) == ld
    before = logits.view(torch.int16).clone()
    with poisoned_outputs():
        row_loss, row_argmax = ops.ce_eval(logits, V, y)
    torch.cuda.synchronize()
    assert row_loss.dtype == torch.float32 and row_argmax.dtype == torch.int32 and row_loss.shape == row_argmax.shape == (n,)
    assert torch.equal(logits.view(torch.int16), before), 'the logits are read only'
    assert bool(torch.isfinite(row_loss).all()), 'a row loss was not written (or a pad column leaked into it)'
    worst, ref_arg = 0.0, []
    for r0 in range(0, n, 256):                         # (fp64 temporaries of 256 rows: 0.5 GB at the vocabulary width)
        x = logits[r0:r0 + 256, :V]
        ref_arg.append(_lowest_argmax(x))
        worst = max(worst, _loss_bound(row_loss[r0:r0 + 256], x.double(), y[r0:r0 + 256], V, 'ce_eval (%d, %d)' % (n, V)))
    ref_arg = torch.cat(ref_arg)
    print('ce_eval (%d, %d): row loss reaches %.3f of its bound' % (n, V, worst))
    assert torch.equal(row_argmax.long(), ref_arg), 'rows %s' % torch.nonzero(row_argmax.long() != ref_arg).view(-1)[:8].tolist()
    for r, c in want.items():                           # the planted rows say what they were planted for
        assert int(row_argmax[r]) == c, (r, int(row_argmax[r]), c)
    hit = row_argmax.long() == y
    if n >= 9:
        assert bool(hit[5]) and not bool(hit[0])        # target on / off the argmax
    # bad arguments are refused
    from m3p_amd import lib as L
    bad = L.load().m3p_ce_eval(logits.data_ptr(), ld - 1, n, V, y.data_ptr(), row_loss.data_ptr(), row_argmax.data_ptr(), L.stream())
    assert bad != 0
    assert L.load().m3p_ce_eval(logits.data_ptr() + 2, ld, n, V, y.data_ptr(), row_loss.data_ptr(), row_argmax.data_ptr(), L.stream()) != 0
    assert L.load().m3p_ce_eval(logits.data_ptr(), ld, n, ld + 8, y.data_ptr(), row_loss.data_ptr(), row_argmax.data_ptr(), L.stream()) != 0


# ------------------------------------------------------------------------------------------------ the head
def _model(P, sd, train=False):
    from m3p_amd.model.transformer import TransformerModel
    torch.manual_seed(0)
    m = TransformerModel(P, is_encoder=True, with_output=True, is_crossModal=True).cuda()
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected
    return m.train() if train else m.eval()


def _reference_stats(m, tensor, pred_mask, y):
    """ops.ce_eval on the logits of a decoder.word_scores-style projection of the gathered rows -> (loss_sum fp64, hits, logits)."""
    from m3p_amd import lib as L, ops
    ar = m.arena()
    ar.refresh()
    V = m.n_words
    rows = tensor[pred_mask].contiguous()
    logits = torch.empty((rows.shape[0], ar.V_pad), dtype=BF16, device='cuda')
    ops.gemm_nt(rows, ar.w('embeddings.weight'), L.EPI_BIAS, bias=ar.p('pred_layer.proj.bias'), out=logits, n=V)
    row_loss, row_argmax = ops.ce_eval(logits, V, y)
    return row_loss.sum(dtype=torch.float64), row_argmax.long() == y, logits[:, :V]


def test_predict_stats_on_the_views_the_passes_return():
    P, sd, x_src, len_src, x_img, loc, img_len, x2, len2 = synth.mt_ic_case()
    m = _model(P, sd)
    R, d = x_img.shape[0], P.emb_dim
    with torch.no_grad():
        enc = m('jointfwd', x=x_src.cuda(), lengths=len_src.cuda(), x_img=x_img.cuda(), lengths_img=img_len.cuda(), causal=False,
                langs=None, image_loc=loc.cuda(), refine_image=False)
        dec = m('crossfwd', stream_='text', x=x2.cuda(), lengths=len2.cuda(), langs=x2.clone().fill_(1).cuda(), causal=True,
                src_enc=enc.transpose(0, 1), src_len=(img_len + len_src).cuda())
    text = enc[R:]                                       # the slice the trainer hands the head: rows of the pass's buffer
    assert not text.is_contiguous() and not dec.is_contiguous()
    shifted = torch.zeros((text.shape[0], text.shape[1], d + 8), dtype=BF16, device='cuda')[..., 8:]
    shifted.copy_(text)                                  # rows that do not start on a multiple of d: the head must copy
    wide = torch.zeros((text.shape[0], text.shape[1], 2 * d), dtype=BF16, device='cuda')[..., :d]
    wide.copy_(text)                                     # non-contiguous, but every row on a multiple of d: read in place
    mask_src = (torch.arange(x_src.shape[0])[:, None] < len_src[None, :]).cuda()
    mask_tgt, y_tgt = synth.mt_targets(x2, len2)
    gen = torch.Generator().manual_seed(3)
    for name, tensor, pred_mask, y in (('encoder_out[R:]', text, mask_src, None), ('decoder output', dec, mask_tgt.cuda(), y_tgt.cuda()),
                                       ('unaligned rows', shifted, mask_src, None), ('wide rows', wide, mask_src, None)):
        n = int(pred_mask.sum())
        assert n % 256 != 0
        if y is None:                                    # half the targets on the best-scoring word
            y = torch.randint(3, P.n_words, (n,), generator=gen).cuda()
            best = _lowest_argmax(_reference_stats(m, tensor, pred_mask, y)[2])
            y = torch.where(torch.arange(n, device='cuda') % 2 == 0, best, y)
        want_loss, want_hit, ref_logits = _reference_stats(m, tensor, pred_mask, y)
        loss_sum, n_correct, n_got = m.predict_stats(tensor, pred_mask, y)
        assert n_got == n and loss_sum.dtype == torch.float64 and n_correct.dtype == torch.int64
        assert loss_sum.dim() == n_correct.dim() == 0 and loss_sum.is_cuda and n_correct.is_cuda
        # one chunk, the same projection launch: the same bits
        assert float(loss_sum) == float(want_loss) and int(n_correct) == int(want_hit.sum()), name
        assert 0 < int(n_correct) < n or name == 'decoder output'
        # the training-side route to the same count: predict(get_scores=True)'s fp32 scores under the lowest-index rule
        with torch.no_grad():
            scores, loss = m('predict', tensor=tensor, pred_mask=pred_mask, y=y, get_scores=True)
        assert scores.dtype == torch.float32 and int((_lowest_argmax(scores) == y).sum()) == int(n_correct), name
        assert abs(float(loss) * n - float(loss_sum)) < 1e-4 * abs(float(loss_sum))
        # through the dispatcher as the evaluator calls it
        again = m('predict_stats', tensor=tensor, pred_mask=pred_mask, y=y)
        assert float(again[0]) == float(loss_sum) and int(again[1]) == int(n_correct)
    # the head refuses to run where autograd would expect a gradient from it
    m.train()
    with torch.enable_grad(), pytest.raises(NotImplementedError):
        m.predict_stats(text, mask_src, y)
    with torch.no_grad():                                # training mode under no_grad is fine (forward only)
        assert m.predict_stats(dec, mask_tgt.cuda(), y_tgt.cuda())[2] == int(mask_tgt.sum())


def test_predict_stats_over_several_chunks():
    """5003 prediction rows: two chunks (2560 on the full-tile projection + 2443 on the ragged one), not a multiple of 256.
    The reference projects all rows in ONE ragged launch; where the two launches' kernels differ a logit may move by one bf16
    rounding (2^-8 of itself), which moves a row's loss by at most that and can only change the argmax of a row whose two best
    reference logits are closer than two roundings of the best."""
    from m3p_amd import functional as Fn
    P, sd, *_ = synth.mt_case()
    m = _model(P, sd)
    d, V, n = P.emb_dim, P.n_words, 5003
    assert n > Fn.EVAL_CHUNK_ROWS and len(Fn._eval_chunks(n)) == 2
    gen = torch.Generator(device='cuda').manual_seed(21)
    tensor = (torch.randn((48, 160, d), generator=gen, device='cuda') * 4.0).to(BF16)[8:]        # a view into a larger buffer
    flat = torch.zeros(40 * 160, dtype=torch.bool, device='cuda')
    flat[torch.randperm(40 * 160, generator=gen, device='cuda')[:n]] = True
    pred_mask = flat.view(40, 160)
    y = torch.randint(3, V, (n,), generator=gen, device='cuda')
    _, _, ref_logits = _reference_stats(m, tensor, pred_mask, y)
    y = torch.where(torch.arange(n, device='cuda') % 2 == 0, _lowest_argmax(ref_logits), y)
    want_loss, want_hit, ref_logits = _reference_stats(m, tensor, pred_mask, y)
    loss_sum, n_correct, n_got = m.predict_stats(tensor, pred_mask, y)
    assert n_got == n
    x = ref_logits.float()
    assert abs(float(loss_sum) - float(want_loss)) <= n * 2.0 ** -8 * float(x.abs().max())
    top2 = x.topk(2, dim=1)[0]
    sure = (top2[:, 0] - top2[:, 1]) >= 2.0 ** -7 * top2[:, 0].abs()
    got_hit = _hits_of(m, tensor, pred_mask, y)
    assert int(got_hit.sum()) == int(n_correct)
    print('multi-chunk: %d of %d rows compared, loss sums %.6f / %.6f' % (int(sure.sum()), n, float(loss_sum), float(want_loss)))
    assert int(sure.sum()) > n // 2 and torch.equal(got_hit[sure], want_hit[sure])
    with torch.no_grad():
        scores, _ = m('predict', tensor=tensor, pred_mask=pred_mask, y=y, get_scores=True)
    assert torch.equal(got_hit[sure], (_lowest_argmax(scores) == y)[sure])


def _hits_of(m, tensor, pred_mask, y):
    """Row by row what predict_stats counted: the launcher's outputs, collected chunk by chunk."""
    from m3p_amd import ops
    seen, real = [], ops.ce_eval

    def spy(logits, V, target):
        out = real(logits, V, target)
        seen.append(out[1].long() == target)
        return out
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, 'ce_eval', spy)
        m.predict_stats(tensor, pred_mask, y)
    return torch.cat(seen)


# ------------------------------------------------------------------------------------------------ end to end against the oracle
def oracle_mt(P, sd, x1, len1, x2, len2):
    """The oracle's word scores and targets of a translation batch (en -> zh) - and its encoder output."""
    enc = ref_cpu.crossfwd_text(sd, P.n_layers, P.n_heads, x1, len1, langs=x1.clone().fill_(0)).transpose(0, 1)
    dec = ref_cpu.decoder_crossfwd(sd, P.n_layers, P.n_heads, x2, len2, enc, len1, langs=x2.clone().fill_(1))
    pred_mask, y = synth.mt_targets(x2, len2)
    return ref_cpu.predict_mlm(sd, dec, pred_mask, y)[0], y, enc


def oracle_ic(P, sd, x_img, loc, img_len, x2, len2):
    R, B = x_img.shape[0], x_img.shape[1]
    enc = ref_cpu.crossfwd_img(sd, P.n_layers, P.n_heads, x_img, img_len, loc, langs=torch.zeros((R, B), dtype=torch.long)).transpose(0, 1)
    dec = ref_cpu.decoder_crossfwd(sd, P.n_layers, P.n_heads, x2, len2, enc, img_len, langs=x2.clone().fill_(0))
    pred_mask, y = synth.mt_targets(x2, len2)
    return ref_cpu.predict_mlm(sd, dec, pred_mask, y)[0], y, enc


def half_greedy_targets(P, sd, enc, src_len, x2, len2, tgt_lang_id, seed):
    """A second batch of targets: the first half of the sentences are the oracle's own greedy decodings of their sources (teacher-
    forced, the oracle scores every word of them right), the others fresh random sentences.  With the tied embedding matrix
    these untrained models score the word they have just read highest, so every decoding is <EOS> <EOS> - one predicted row
    per sentence - and the oracle gets no row of a random sentence right; the random sentences are therefore three symbols
    long (two rows each), which puts the oracle's accuracy at a third of the batch."""
    B = x2.shape[1]
    gen, gen_len, _ = ref_cpu.greedy_decode(sd, P.n_layers, P.n_heads, enc, src_len, tgt_lang_id, max_len=x2.shape[0])
    rs = np.random.RandomState(seed)
    lens = torch.full_like(len2, 3)
    lens[:B // 2] = gen_len[:B // 2]
    out = torch.full((int(lens.max()), B), synth.PAD, dtype=torch.long)
    for b in range(B):
        n = int(lens[b])
        if b < B // 2:
            out[:n, b] = gen[:n, b]
        else:
            out[0, b] = out[n - 1, b] = synth.EOS
            out[1:n - 1, b] = torch.from_numpy(rs.randint(3, P.n_words, size=n - 2))
    return out, lens


def oracle_summary(scores, y):
    """-> (xe_loss / n_words, hits row by row, rows whose top-2 margin reaches MARGIN)."""
    top2 = scores.topk(2, dim=1)[0]
    return float(F.cross_entropy(scores, y, reduction='mean')), scores.max(1)[1] == y, (top2[:, 0] - top2[:, 1]) >= MARGIN


@pytest.fixture
def rows_seen(monkeypatch):
    """(row_argmax == target) of every ops.ce_eval launch, in order: what the evaluation counted, row by row."""
    from m3p_amd import ops
    seen, real = [], ops.ce_eval

    def spy(logits, V, target):
        out = real(logits, V, target)
        seen.append((out[1].long() == target).cpu())
        return out
    monkeypatch.setattr(ops, 'ce_eval', spy)
    return seen


def _against_oracle(scores, ppl_key, acc_key, rows_seen, oracle_scores, y, second):
    """The bars of one evaluated batch.  First (recorded) batch: no row under the margin.  Second: at most MAX_EXCLUDED of
    them, and an oracle accuracy that makes the count mean something."""
    want_loss, want_hit, sure = oracle_summary(oracle_scores, y)
    n = y.numel()
    got_hit = torch.cat(rows_seen)
    del rows_seen[:]
    got_loss = math.log(scores[ppl_key])
    print('%s: xe / n %.5f (oracle %.5f), hits %d (oracle %d) of %d, %d rows under the margin (smallest %.3f)' % (
        ppl_key, got_loss, want_loss, int(got_hit.sum()), int(want_hit.sum()), n, int((~sure).sum()),
        float((oracle_scores.topk(2, dim=1)[0] @ torch.tensor([1.0, -1.0])).min())))
    assert got_hit.numel() == n and abs(scores[acc_key] - 100. * int(got_hit.sum()) / n) < 1e-9
    assert abs(got_loss - want_loss) <= LOSS_RTOL * abs(want_loss)
    if second:
        assert int((~sure).sum()) <= MAX_EXCLUDED * n
        assert 0.30 <= float(want_hit.float().mean()) <= 0.90
    else:
        assert bool(sure.all())
    assert torch.equal(got_hit[sure], want_hit[sure])
    if bool(sure.all()):
        assert scores[acc_key] == 100. * int(want_hit.sum()) / n


def test_evaluate_mt_against_the_oracle(rows_seen):
    from m3p_amd import evaluation as E
    P, sd, x1, len1, x2, len2 = synth.mt_case()
    P.langs = ['en', 'zh']
    m = _model(P, sd, train=True)
    sc, y, enc = oracle_mt(P, sd, x1, len1, x2, len2)
    scores = E.evaluate_mt(m, P, iter([((x1, len1), (x2, len2))]), OrderedDict(), 'valid', 'en', 'zh')
    assert list(scores) == ['valid_en-zh_mt_ppl', 'valid_en-zh_mt_acc'] and m.training
    _against_oracle(scores, 'valid_en-zh_mt_ppl', 'valid_en-zh_mt_acc', rows_seen, sc, y, second=False)
    x2b, len2b = half_greedy_targets(P, sd, enc, len1, x2, len2, 1, seed=5)
    sc, y, _ = oracle_mt(P, sd, x1, len1, x2b, len2b)
    scores = E.evaluate_mt(m, P, iter([((x1, len1), (x2b, len2b))]), OrderedDict(), 'valid', 'en', 'zh')
    _against_oracle(scores, 'valid_en-zh_mt_ppl', 'valid_en-zh_mt_acc', rows_seen, sc, y, second=True)


def _ic_batch(x_img, loc, img_len, x2, len2):
    R, B = x_img.shape[0], x_img.shape[1]
    x1_mask = (torch.arange(R)[None, :] < img_len[:, None]).long()
    return (x2, len2, None), (x_img.transpose(0, 1).contiguous(), x1_mask, loc.transpose(0, 1).contiguous(), list(range(B)))


def test_evaluate_ic_against_the_oracle(rows_seen):
    from m3p_amd import evaluation as E
    P, sd, x_img, loc, img_len, x2, len2 = synth.ic_case()
    P.langs, P.ft_lgs = ['en', 'zh'], []
    m = _model(P, sd, train=True)
    sc, y, enc = oracle_ic(P, sd, x_img, loc, img_len, x2, len2)
    scores = E.evaluate_ic(m, P, iter([_ic_batch(x_img, loc, img_len, x2, len2)]), OrderedDict(), 'valid', 'coco', 'img')
    assert list(scores) == ['valid_coco-img_IC_ppl', 'valid_coco-img_IC_acc'] and m.training
    _against_oracle(scores, 'valid_coco-img_IC_ppl', 'valid_coco-img_IC_acc', rows_seen, sc, y, second=False)
    x2b, len2b = half_greedy_targets(P, sd, enc, img_len, x2, len2, 0, seed=5)
    sc, y, _ = oracle_ic(P, sd, x_img, loc, img_len, x2b, len2b)
    scores = E.evaluate_ic(m, P, iter([_ic_batch(x_img, loc, img_len, x2b, len2b)]), OrderedDict(), 'valid', 'coco', 'img')
    _against_oracle(scores, 'valid_coco-img_IC_ppl', 'valid_coco-img_IC_acc', rows_seen, sc, y, second=True)


def mlm_case():
    """The two-language cfg1 model and the token stream cut into (16, 4) batches, as StreamDataset serves them."""
    from m3p_amd.datasets import StreamDataset
    cfg, P, sd, _, _ = synth.text_langs_case()
    for k, v in synth.trainer_params(langs=['en', 'zh'], batch_size=4, mlm_steps=[('zh', None)], clm_steps=[],
                                     optimizer='adam_inverse_sqrt,beta1=0.9,beta2=0.98,lr=0.002,warmup_updates=4').items():
        setattr(P, k, v)
    sent, pos, _ = synth.token_stream()
    ds = StreamDataset(sent, pos, SimpleNamespace(bptt=16, batch_size=4, eos_index=synth.EOS, lang2id=P.lang2id))
    return P, sd, list(ds.get_iterator(shuffle=False))


def oracle_mlm(P, sd, batches):
    """The oracle's word scores and targets over the data set, under the evaluator's masking (one RandomState(0))."""
    from m3p_amd.evaluation import eval_mask_out
    rng = np.random.RandomState(0)
    scores, ys = [], []
    for x, lengths in batches:
        xm, y, pred_mask = eval_mask_out(x, lengths, P, rng)
        out = ref_cpu.crossfwd_text(sd, P.n_layers, P.n_heads, xm, lengths, langs=xm.clone().fill_(1))
        scores.append(ref_cpu.predict_mlm(sd, out, pred_mask, y)[0])
        ys.append(y)
    return torch.cat(scores), torch.cat(ys)


def test_evaluate_mlm_against_the_oracle_and_after_training(rows_seen):
    from m3p_amd import evaluation as E
    from m3p_amd.trainer import XTrainer
    P, sd, batches = mlm_case()
    m = _model(P, sd, train=True)
    sc, y = oracle_mlm(P, sd, batches)
    before = E.evaluate_mlm(m, P, iter(batches), OrderedDict(), 'valid', 'zh', None)
    assert list(before) == ['valid_zh_mlm_ppl', 'valid_zh_mlm_acc'] and m.training
    want_loss, want_hit, sure = oracle_summary(sc, y)
    n = y.numel()
    got_hit = torch.cat(rows_seen)
    del rows_seen[:]
    print('mlm: xe / n %.5f (oracle %.5f), %d of %d rows under the margin' % (math.log(before['valid_zh_mlm_ppl']), want_loss,
                                                                           int((~sure).sum()), n))
    assert abs(math.log(before['valid_zh_mlm_ppl']) - want_loss) <= LOSS_RTOL * abs(want_loss)
    assert int((~sure).sum()) <= MAX_EXCLUDED * n and torch.equal(got_hit[sure], want_hit[sure])
    # deterministic: the same words are scored on every call
    assert E.evaluate_mlm(m, P, iter(batches), OrderedDict(), 'valid', 'zh', None) == before
    del rows_seen[:]
    # thirty training steps on those sentences (the trainer's own masking), then the perplexity is lower
    tr = XTrainer(m, {}, P)
    np.random.seed(7); torch.manual_seed(7)
    for it in range(30):
        x, lengths = batches[it % len(batches)]
        xm, yy, pred_mask = tr.mask_out(x, lengths)
        tr.mlm_step_on_batch(xm, lengths, pred_mask, yy, 'zh', 1.0, langs=xm.clone().fill_(1).cuda())
        tr.iter()
    after = E.evaluate_mlm(m, P, iter(batches), OrderedDict(), 'valid', 'zh', None)
    print('mlm perplexity %.2f -> %.2f after 30 steps' % (before['valid_zh_mlm_ppl'], after['valid_zh_mlm_ppl']))
    assert after['valid_zh_mlm_ppl'] < before['valid_zh_mlm_ppl'] and m.training


def test_one_host_read_per_data_set(monkeypatch):
    from m3p_amd import evaluation as E
    P, sd, x1, len1, x2, len2 = synth.mt_case()
    P.langs = ['en', 'zh']
    m = _model(P, sd)
    reads, real = [], E._host_read

    def counted(t):
        reads.append(tuple(t.shape))
        return real(t)
    monkeypatch.setattr(E, '_host_read', counted)
    batches = [((x1, len1), (x2, len2))] * 5
    scores = E.evaluate_mt(m, P, iter(batches), OrderedDict(), 'valid', 'en', 'zh')
    assert len(reads) == 1, reads
    one = E.evaluate_mt(m, P, iter(batches[:1]), OrderedDict(), 'valid', 'en', 'zh')
    assert abs(scores['valid_en-zh_mt_ppl'] - one['valid_en-zh_mt_ppl']) < 1e-9 * one['valid_en-zh_mt_ppl']
    assert scores['valid_en-zh_mt_acc'] == one['valid_en-zh_mt_acc'] and not m.training
