"""The MLM head without a gradient pass over the logits: the shifted-exponential epilogue of the
vocabulary projection and the head built on it, against fp64.

The projection stores e[n, v] = bf16(exp(x[n, v] - c_n)), c_n = the target's own logit + 40, an exact 0 at the target column and
at the pad columns, and the fp32 sums of the rounded values per (row, 64-column block); the normaliser 1 / Sigma_n is applied
to the [n, d] operands of the two gradient products and the target's term (p_y - 1) stays in fp32 (csrc/heads.hip)."""
import math

import pytest
import torch

from tests.test_model_parity import CFGS, _build
from tests.util import (ATTN_CTX_RTOL, BF16_OUT, F32_OUT, KAPPA, ROW_FLOOR, U32, accum_bound, assert_exact_zero, block_bound,
                        gemm_bound, poisoned_outputs)

pytestmark = pytest.mark.gpu

SHIFT = 40.0
BF16 = torch.bfloat16


def _prod64(a, w):
    a64, w64 = a.double(), w.double()
    return a64 @ w64.t(), a64.abs() @ w64.abs().t()


@pytest.mark.parametrize('M,N,V,K', [(1024, 1280, 1217, 128), (1024, 512, 512, 64)])
def test_shifted_exponential_epilogue_every_element(M, N, V, K):
    """Every stored value against fp64 exp(x - c_n) for the c_n the launch was handed: one bf16 rounding, the GEMM's element
    bound on x (it moves e by e dx), the fp32 evaluation of the exponent (its roundings are relative to |x| and |c|: 4 u (|x| +
    |c|) covers the bias add, the product c log2(e) and the fma) and the 2^-20 of the fast exponential; results below fp32's
    smallest normal number may flush to zero.  Pad and target columns hold exact zeros; every block sum is the fp32 sum of the 64
    stored values of its block (worst case of a depth-64 sum: 64 u sum |values|)."""
    from m3p_amd import ops, lib as L
    g = torch.Generator(device='cuda').manual_seed(M + N + K)
    a = torch.randn((M, K), device='cuda', generator=g).to(BF16)
    w = (torch.randn((N, K), device='cuda', generator=g) * (1.2 / math.sqrt(K))).to(BF16)
    bias = torch.randn((N,), device='cuda', generator=g) * 0.5
    y = torch.randint(0, V, (M,), device='cuda', generator=g)
    y[5], y[6], y[7] = V - 1, 0, V - 1                                  # the last valid column, the first, a repeated id
    rows = torch.arange(M, device='cuda')
    with poisoned_outputs():
        row_t, row_ref = ops.ce_shift_target(a, w, bias, y)
        stats = torch.empty((N // 64, M), dtype=torch.float32, device='cuda')
        stats.untyped_storage().fill_(0xFF)
        e = ops.gemm_nt(a, w, L.EPI_BIAS_LSE, bias=bias, out2=stats, scale_cols=V, row_ref=row_ref)
    p64, ap64 = _prod64(a, w)
    x64, ax64 = p64 + bias.double(), ap64 + bias.double().abs()
    # (a) the target's logit: a depth-K fp32 dot product plus the bias
    t64 = x64[rows, y]
    t_err = (row_t.double() - t64).abs() / (KAPPA * math.sqrt(K) * U32 * ax64[rows, y] + F32_OUT * t64.abs() + 1e-300)
    print('target logit: worst error %.3g x its bound' % float(t_err.max()))
    assert float(torch.nan_to_num(t_err, nan=math.inf).max()) <= 1.0
    c = row_ref[:, 0].contiguous().view(torch.float32)
    assert torch.equal(c, row_t + SHIFT) and torch.equal(row_ref[:, 1].long(), y)
    # the epilogue, every element
    c64 = c.double()[:, None]
    ref = torch.exp(x64 - c64)
    ref[rows, y] = 0.0
    ref[:, V:] = 0.0
    eps = ref * (2.0 ** -20 + 4 * U32 * (x64.abs() + c64.abs())) + 2.0 ** -126
    worst, at = gemm_bound(e, ref, ref * ax64, K, BF16_OUT, eps)
    print('e: worst error %.3g x the elementwise bound at %s' % (worst, at))
    assert worst <= 1.0, (worst, at)
    assert_exact_zero(e[:, V:], 'pad columns')
    assert_exact_zero(e[rows, y], 'target columns')
    # the block sums: of the ROUNDED values
    sums = e.float().double().view(M, N // 64, 64).sum(-1).t()
    err = torch.nan_to_num((stats.double() - sums).abs(), nan=math.inf)
    bound = 64 * U32 * sums
    print('block sums: worst error %.3g x the depth-64 bound' % float((err / (bound + 1e-300)).max()))
    assert bool((err <= bound).all())


def _reference(H, E, b, y, g):
    """fp64 loss rows and gradients of the tied projection + mean cross-entropy times the upstream gradient g, with the sums of
    absolute values the accumulation bounds take."""
    n = H.shape[0]
    rows = torch.arange(n, device=H.device)
    H64, E64 = H.double(), E.double()
    x = H64 @ E64.t() + b.double()
    ax = H64.abs() @ E64.abs().t() + b.double().abs()
    lse = torch.logsumexp(x, 1)
    loss_n = lse - x[rows, y]
    G = torch.exp(x - lse[:, None])
    p_y = G[rows, y].clone()
    G[rows, y] = torch.expm1(-loss_n)                              # p_y - 1 without cancellation
    G *= g / n
    return dict(loss_n=loss_n, t=x[rows, y], p_y=p_y, accx=KAPPA * math.sqrt(H.shape[1]) * U32 * ax.max(1).values,
                dH=G @ E64, dE=G.t() @ H64, adE=G.abs().t() @ H64.abs(), db=G.sum(0), adb=G.abs().sum(0))


class _Head:
    """The `tiles` configuration's head (d = 256, V = 5000, 4096 predicted rows: whole tiles everywhere) with a vocabulary
    matrix of this test's own: logits ~ N(0, 1.2^2) + bias.  Column 0 of the matrix is zero but for one word, PLANT, so a
    hidden row that is a multiple of the first unit vector has the logits bias[v] everywhere and any chosen logit at PLANT."""
    PLANT = 4000
    G_UP = 0.5          # the upstream gradient of the loss

    def __init__(self):
        cfg = CFGS['tiles']
        self.m, _, sd = _build(cfg)
        self.m.train()
        self.d, self.V = cfg['emb_dim'], cfg['n_words']
        self.T, self.B = cfg['n_pred'], cfg['B']
        self.n = self.T * self.B
        g = torch.Generator().manual_seed(11)
        E = (torch.randn((self.V, self.d), generator=g) * (1.2 / math.sqrt(self.d))).to(BF16).float()
        E[:, 0] = 0.0
        E[self.PLANT, 0] = 1.0
        b = torch.randn((self.V,), generator=g) * 0.5
        for k in sd:
            if k in ('embeddings.weight', 'pred_layer.proj.weight'):
                sd[k] = E.clone()
            if k == 'pred_layer.proj.bias':
                sd[k] = b.clone()
        self.m.load_state_dict(sd, strict=False)
        self.E, self.b = E.cuda(), b.cuda()
        self.H = torch.randn((self.n, self.d), generator=g).to(BF16).cuda()
        y = torch.randint(0, self.V, (self.n,), generator=g)
        y[10:20] = 123                                                  # an id that repeats across rows
        y[20] = y[21] = self.V - 1                                      # the last word
        self.y = y.cuda()
        self._refs = {}

    def run(self, H, y, scores):
        """One forward and backward of MLMHeadFn: (mean loss, dH, dE, db)."""
        m = self.m
        m.arena().zero_grad()
        tensor = H.view(self.T, self.B, self.d).clone().requires_grad_(True)
        mask = torch.ones((self.T, self.B), dtype=torch.bool, device='cuda')
        _, loss = m('predict', tensor=tensor, pred_mask=mask, y=y, get_scores=scores)
        (loss * self.G_UP).backward()
        torch.cuda.synchronize()
        own = dict(m.named_parameters())
        return (float(loss), tensor.grad.view(self.n, self.d).float().clone(), own['embeddings.weight'].grad.clone(),
                own['pred_layer.proj.bias'].grad.clone())

    def reference(self, key, H, y):
        if key not in self._refs:
            self._refs[key] = _reference(H, self.E, self.b, y, self.G_UP)
        return self._refs[key]


@pytest.fixture(scope='module')
def head():
    return _Head()


def _distances(head, got, ref):
    """Each output's distance from the fp64 reference in units of its bound (<= 1 passes).
    loss: a row's log-sum-exp moves by at most one bf16 rounding of the stored values it sums (relative: BF16_OUT absolute in
      the logarithm) and twice the GEMM's element bound on a logit; the path that reads the target's logit back from the bf16
      tensor adds BF16_OUT |t_n|.  The mean loss is held to the mean of the rows' bounds.
    dH: rows of G E with G rounded to bf16 and the result stored in bf16 - the two roundings of the attention context's P V
      (ATTN_CTX_RTOL, rows below ROW_FLOOR of the RMS row measured against it).
    dE: G^T H in fp32 over n rows, both operands rounded to bf16 once: BF16_OUT sum |G| |H| beside the accumulation term.
    db: n addends gathered in any order, each rounded to bf16 once."""
    loss, dH, dE, db = got
    lb = BF16_OUT * (1.0 + ref['t'].abs()) + 2.0 * ref['accx']
    out = {'loss': abs(loss - float(ref['loss_n'].mean())) / float(lb.mean())}
    worst, at, ratio = block_bound(dH, ref['dH'], ('row',), ATTN_CTX_RTOL, ROW_FLOOR)
    out['dH'] = ratio
    out['dE'] = gemm_bound(dE, ref['dE'], ref['adE'], head.n, F32_OUT, BF16_OUT * ref['adE'])[0]
    out['db'] = accum_bound(db, ref['db'], ref['adb'], head.n, BF16_OUT * ref['adb'])[0]
    return out


def test_head_forward_and_backward_on_both_paths(head):
    """MLMHeadFn on the shifted-exponential path (no scores wanted) and on the path that stores logits and rewrites them into
    their gradient (scores wanted), each against fp64 and each held to the same bounds."""
    from m3p_amd import functional as Fn
    assert Fn._CE_FUSED_LSE and Fn._VOCAB_FULL_TILES and head.n >= 4096 and head.n % 256 == 0
    ref = head.reference('plain', head.H, head.y)
    new = _distances(head, head.run(head.H, head.y, scores=False), ref)
    old = _distances(head, head.run(head.H, head.y, scores=True), ref)
    for k in ('loss', 'dH', 'dE', 'db'):
        print('%-4s distance / bound: shifted exponential %.3g, logits rewritten in place %.3g' % (k, new[k], old[k]))
    for k in ('loss', 'dH', 'dE', 'db'):
        assert new[k] <= 1.0, (k, new[k])
        assert old[k] <= 1.0, (k, old[k])


def test_confident_and_hopeless_rows(head):
    """Rows whose target logit is 12 and 25 above every other logit (p_y - 1 is -3e-2 and -7e-8: a bf16 p_y minus 1 would be
    all rounding error) and rows whose target is 60 below the maximum: loss, dH row and db finite and within the bounds."""
    from m3p_amd import ops, lib as L
    H, y = head.H.clone(), head.y.clone()
    b, P = head.b, head.PLANT
    others = b.clone()
    others[P] = -math.inf
    top = float(others.max())
    H[:4] = 0.0
    y[0] = y[1] = P
    y[2], y[3] = 7, head.V - 1
    # (bf16 rounds these to within 2^-8 of themselves, 0.03 at 12 and 0.125 at 60: an eighth on top keeps the margins nominal)
    H[0, 0] = 12.125 + top - float(b[P])
    H[1, 0] = 25.125 + top - float(b[P])
    H[2, 0] = 60.125 + float(b[7]) - float(b[P])
    H[3, 0] = 60.125 + float(b[head.V - 1]) - float(b[P])
    ref = head.reference('planted', H, y)
    x = H[:4].double() @ head.E.double().t() + b.double()
    margins = [float(x[0, P] - others.double().max()), float(x[1, P] - others.double().max()),
               float(x[2].max() - x[2, 7]), float(x[3].max() - x[3, head.V - 1])]
    print('planted margins:', margins)
    assert margins[0] >= 12 and margins[1] >= 25 and margins[2] >= 60 and margins[3] >= 60
    got = head.run(H, y, scores=False)
    loss, dH, dE, db = got
    assert math.isfinite(loss) and bool(torch.isfinite(dH[:4]).all()) and bool(torch.isfinite(db).all())
    dist = _distances(head, got, ref)
    print('planted rows, distance / bound:', dist)
    for k in ('loss', 'dH', 'dE', 'db'):
        assert dist[k] <= 1.0, (k, dist[k])
    # the planted rows on their own, against their OWN norm (no floor): a row of dH is (1 - p_y) / n times a difference of
    # embedding rows, its terms are no larger than the row itself, so the two roundings hold relative to the row
    worst, at, ratio = block_bound(dH[:4], ref['dH'][:4], ('row',), ATTN_CTX_RTOL, 0.0)
    print('planted dH rows against their own norm: %.3g x the bound (row %s)' % (ratio, at))
    assert ratio <= 1.0
    # the rows' losses from the launchers the head calls.  The row sum of the other columns carries one bf16 rounding of its
    # addends: the loss moves by at most BF16_OUT (1 - p_y); the logits' own error and a few fp32 roundings of the row kernel
    ar = head.m.arena()
    ar.refresh()
    o = ar.offsets['pred_layer.proj.bias'][0]
    _, row_ref = ops.ce_shift_target(H, ar.w('embeddings.weight'), ar.p('pred_layer.proj.bias'), y)
    stats = torch.empty((ar.V_pad // 64, head.n), dtype=torch.float32, device='cuda')
    e = torch.empty((head.n, ar.V_pad), dtype=BF16, device='cuda')
    ops.gemm_nt(H, ar.w('embeddings.weight'), L.EPI_BIAS_LSE, bias=ar.master[o:o + ar.V_pad], out=e, n=ar.V_pad, out2=stats,
                scale_cols=head.V, row_ref=row_ref)
    _, row_loss, row_s, row_q, _ = ops.ce_shift_from_block_sums(e, stats, 1.0 / head.n, 1.0 / head.n)
    # (relative to the shift and the loss: SHIFT + log Sigma where the row is not confident)
    bound = BF16_OUT * (1.0 - ref['p_y']) + 2.0 * ref['accx'] + F32_OUT * (SHIFT + ref['loss_n'])
    r = torch.nan_to_num((row_loss.double() - ref['loss_n']).abs() / bound, nan=math.inf)
    print('row losses: worst %.3g x the bound (row %d); planted rows %s against %s' % (
        float(r.max()), int(r.argmax()), row_loss[:4].tolist(), ref['loss_n'][:4].tolist()))
    assert bool(torch.isfinite(row_loss).all()) and float(r.max()) <= 1.0
    # the target's coefficient q_n = (p_y - 1) / n, relative to itself: 1 - p_y = r / (1 + r) follows the other columns' mass r,
    # which carries the bf16 rounding of its addends and, in the exponent, the error of the logits and of the target's own
    q64 = torch.expm1(-ref['loss_n']) / head.n
    rq = (row_q.double() - q64).abs() / (q64.abs() * (BF16_OUT + 2.0 * ref['accx'] + F32_OUT * SHIFT) + 1e-300)
    print('q_n: worst %.3g x the bound (row %d)' % (float(rq.max()), int(rq.argmax())))
    assert float(torch.nan_to_num(rq, nan=math.inf).max()) <= 1.0
