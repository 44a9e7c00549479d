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
    # what a relative perturbation of every logit, |delta_nv| <= |x_nv|, moves the softmax by at most: d p_nv = p_nv (delta_nv -
    # sum_w p_nw delta_nw), so |d p_nv| <= p_nv (|x_nv| + sum_w p_nw |x_nw|); the target's p_y - 1 moves like p_y
    xG = G * (x.abs() + (G * x.abs()).sum(1, keepdim=True)) * (abs(g) / n)
    G[rows, y] = torch.expm1(-loss_n)                              # p_y - 1 without cancellation
    G *= g / n
    return dict(loss_n=loss_n, t=x[rows, y], p_y=p_y, accx=KAPPA * math.sqrt(H.shape[1]) * U32 * ax.max(1).values,
                dH=G @ E64, dE=G.t() @ H64, adE=G.abs().t() @ H64.abs(), xdE=xG.t() @ H64.abs(), db=G.sum(0), adb=G.abs().sum(0))


_MODELS = {}


def _model(d):
    """One model per width, shared by every head of that width: the `tiles` configuration (d = 256, V = 5000), or its
    vocabulary on a single layer of another width."""
    if d not in _MODELS:
        cfg = CFGS['tiles'] if d == CFGS['tiles']['emb_dim'] else dict(CFGS['tiles'], emb_dim=d, n_heads=d // 64, n_layers=1)
        _MODELS[d] = _build(cfg) + (cfg,)
    return _MODELS[d]


class _Head:
    """An MLM head of T x B predicted rows at width d - by default the `tiles` configuration's (d = 256, V = 5000, 4096
    predicted rows: whole tiles everywhere) - with a vocabulary matrix of this test's own: logits ~ N(0, 1.2^2) + bias.  Column 0
    of the matrix is zero but for one word, PLANT, so a hidden row that is a multiple of the first unit vector has the logits
    bias[v] everywhere and any chosen logit at PLANT.  The matrix and the bias depend on the width alone."""
    PLANT = 4000
    G_UP = 0.5          # the upstream gradient of the loss

    def __init__(self, T=None, B=None, d=None):
        tiles = CFGS['tiles']
        d = tiles['emb_dim'] if d is None else d
        self.m, _, sd, cfg = _model(d)
        self.m.train()
        self.d, self.V = cfg['emb_dim'], cfg['n_words']
        self.T, self.B = tiles['n_pred'] if T is None else T, tiles['B'] if B is None else B
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

    def run(self, H, y, scores, zero=True):
        """One forward and backward of MLMHeadFn: (mean loss, dH, dE, db).  zero=False: onto the gradients of the pass before."""
        m = self.m
        if zero:
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


def _distances(head, got, ref, passes=1, stored_logits=False):
    """Each output's distance from the fp64 reference in units of its bound (<= 1 passes).  passes: forward / backward passes
    since the gradients were zeroed - dE and db hold that many times the reference, gathered from that many times the terms; the
    loss and dH are the last pass's own.
    stored_logits: the path that stores the logits in bf16 and rewrites them into their gradient reads every logit back with one
      more rounding, |delta x| <= BF16_OUT |x|, in the exponent: G moves by up to BF16_OUT p (|x| + sum_w p_w |x_w|) g / n, and dE
      by that times |H| (ref['xdE']) on top of the term below.  Over 4096 rows the roundings of a word's column largely cancel
      and the plain bound holds (0.73); they cancel like sqrt(n), and at n ~ 1024 the fp64 restatement of the path with nothing
      but its bf16 roundings reaches 1.80 of the plain bound, the kernels 1.75 (tests/test_parity_bounds.py:
      test_head_bounds_need_the_stored_logits_rounding_below_4096_rows).  The callers at 4096 rows keep the plain bound.
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
    k = float(passes)
    eps = BF16_OUT * k * (ref['adE'] + ref['xdE'] if stored_logits else ref['adE'])
    out['dE'] = gemm_bound(dE, k * ref['dE'], k * ref['adE'], passes * head.n, F32_OUT, eps)[0]
    out['db'] = accum_bound(db, k * ref['db'], k * ref['adb'], passes * head.n, BF16_OUT * k * ref['adb'])[0]
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


# ---------------------------------------------------------------------------------------------------------------------
# Every band of the head's dispatch on the number of predicted rows n (MLMHeadFn in m3p_amd/functional.py):
#   n < 1024                        the logits over V columns, ce_fwd_bwd; the weight gradient over V rows
#   n >= 1024, n % 256 != 0         the logits over V columns, ce_fwd_bwd_colsum
#   n >= 1024, n % 256 == 0         whole tiles over V_pad columns: exp(logit - shift) and ce_shift_from_block_sums, or - scores
#                                   wanted - logits with block statistics and ce_from_block_stats
#   n >= 4096, n % 64 == 0          (any forward) the whole-tile weight gradient over V_pad rows: it covers (V_pad - V) d
#                                   elements behind the matrix, past the 5000 elements of the bias gradient
# ---------------------------------------------------------------------------------------------------------------------
BANDS = [  # d, T, B: n = T B
    (256, 341, 3),       # 1023: one below the threshold
    (256, 4, 256),       # 1024: the first whole-tile size; the shifted forward into the accumulating weight gradient
    (256, 103, 10),      # 1030: no multiple of 64
    (256, 17, 64),       # 1088: a multiple of 64, not of 256
    (256, 15, 256),      # 3840: the last whole-tile size below 4096
    (256, 41, 100),      # 4100: past 4096, no multiple of 64
    (256, 65, 64),       # 4160: the whole-tile weight gradient on a gradient whose pad columns the CE kernel zeroed
    (256, 17, 256),      # 4352: 17 whole tiles
    (1024, 4, 256),      # the width of BASELINE configs[3] at 1024 ...
    (1024, 17, 256)]     # ... and at 4352 rows
_HEADS = {}
WORST = {}


def _band_head(d, T, B):
    if (d, T, B) not in _HEADS:
        _HEADS[(d, T, B)] = _Head(T, B, d)
    return _HEADS[(d, T, B)]


class _HeadSpy:
    """Which launchers a forward / backward of the head went through: (epilogue, rows, columns, row_ref given) of every
    ops.gemm_nt, the names of the cross-entropy launchers, and (rows of the matrix, dw_is_zero) of every ops.gemm_wgrad."""
    CE = ('ce_fwd_bwd', 'ce_fwd_bwd_colsum', 'ce_from_block_stats', 'ce_shift_from_block_sums')

    def __init__(self, monkeypatch):
        from m3p_amd import ops
        self.nt, self.ce, self.wgrad = [], [], []
        real_nt, real_wg = ops.gemm_nt, ops.gemm_wgrad

        def nt(a, w, epilogue=0, **kw):
            self.nt.append((epilogue, a.shape[0], kw.get('n') or w.shape[0], kw.get('row_ref') is not None))
            return real_nt(a, w, epilogue, **kw)

        def wg(*a, **kw):
            self.wgrad.append((kw.get('n'), bool(kw.get('dw_is_zero'))))
            return real_wg(*a, **kw)

        def ce(name, real):
            def f(*a, **kw):
                self.ce.append(name)
                return real(*a, **kw)
            return f
        monkeypatch.setattr(ops, 'gemm_nt', nt)
        monkeypatch.setattr(ops, 'gemm_wgrad', wg)
        for name in self.CE:
            monkeypatch.setattr(ops, name, ce(name, getattr(ops, name)))

    def clear(self):
        del self.nt[:], self.ce[:], self.wgrad[:]

    def assert_band(self, head, scores, fresh=True):
        """The branch the table above names for head.n was taken, and no other."""
        from m3p_amd import lib as L
        n, V, Vp = head.n, head.V, head.m.arena().V_pad
        assert (V, Vp) == (5000, 5120)
        whole = n >= 1024 and n % 256 == 0
        if whole:
            fwd = (L.EPI_BIAS_LSE, n, Vp, not scores)
            ce = 'ce_from_block_stats' if scores else 'ce_shift_from_block_sums'
        else:
            fwd = (L.EPI_BIAS, n, V, False)
            ce = 'ce_fwd_bwd_colsum' if n >= 1024 else 'ce_fwd_bwd'
        wgrad = (Vp, fresh) if n >= 4096 and n % 64 == 0 else (V, False)
        assert self.nt == [fwd], (n, scores, self.nt, fwd)
        assert self.ce == [ce], (n, scores, self.ce, ce)
        assert self.wgrad == [wgrad], (n, scores, self.wgrad, wgrad)
        return '%s + %s + gemm_wgrad(n=%d)' % ({L.EPI_BIAS_LSE: 'EPI_BIAS_LSE', L.EPI_BIAS: 'EPI_BIAS'}[fwd[0]], ce, wgrad[0])


def what_of(d, n, scores):
    return 'd = %d, n = %d, %s' % (d, n, 'scores' if scores else 'no scores')


def _assert_rest_of_the_arena_zero(head, what):
    """After backward every element of the gradient arena outside the tied matrix and the output bias is exactly zero: the
    whole-tile weight gradient covers (V_pad - V) d elements behind the matrix, more than the bias gradient holds."""
    ar = head.m.arena()
    assert ar.stale is None and (ar.V_pad - head.V) * head.d > head.V
    rest = ar.grad.clone()
    for name in ('embeddings.weight', 'pred_layer.proj.bias'):
        o, cnt, _ = ar.offsets[name]
        rest[o:o + cnt] = 0
    o, cnt, _ = ar.offsets['embeddings.weight']
    assert cnt == head.V * head.d and rest.numel() > o + ar.V_pad * head.d      # parameters lie behind what the store covers
    assert_exact_zero(rest, what + ': the gradient arena outside embeddings.weight and pred_layer.proj.bias')


@pytest.mark.parametrize('scores', [False, True], ids=['shifted', 'scores'])
@pytest.mark.parametrize('d,T,B', BANDS, ids=['d%d-n%d' % (d, T * B) for d, T, B in BANDS])
def test_head_at_every_dispatch_band(d, T, B, scores, monkeypatch):
    """MLMHeadFn forward and backward against fp64 at both ends of every band of its dispatch, with and without scores, under
    the bounds of the 4096-row head (_distances: they depend neither on n nor on the path).  db[v] and dE[v] of the words no row
    targets are held like the others."""
    from m3p_amd import functional as Fn
    assert Fn._CE_FUSED_LSE and Fn._VOCAB_FULL_TILES
    head = _band_head(d, T, B)
    assert int(torch.bincount(head.y, minlength=head.V).eq(0).sum()) > 0         # words that no row targets
    ref = head.reference('plain', head.H, head.y)
    spy = _HeadSpy(monkeypatch)
    got = head.run(head.H, head.y, scores=scores)
    took = spy.assert_band(head, scores)
    what = what_of(d, head.n, scores)
    # The bound of the 4096-row head everywhere, but for dE where the logits are stored in bf16 (scores wanted, or no whole
    # tiles) AND fewer than 4096 rows are summed: there the rounding of the stored logits is counted (_distances).
    stored = (scores or head.n % 256 != 0 or head.n < 1024) and head.n < 4096
    dist = _distances(head, got, ref, stored_logits=stored)
    if stored:
        print('%s: dE reaches %.3g x the bound that leaves the rounding of the stored logits out' % (what, _distances(head, got, ref)['dE']))
    print('%s: %s' % (what, took))
    print('%s: distance / bound %s' % (what, ', '.join('%s %.3g' % (k, dist[k]) for k in ('loss', 'dH', 'dE', 'db'))))
    WORST[what] = (took, dist)
    for k in ('loss', 'dH', 'dE', 'db'):
        assert dist[k] <= 1.0, (what, k, dist[k])
    _assert_rest_of_the_arena_zero(head, what)


@pytest.mark.parametrize('d,T,B', [(256, 4, 256), (256, 17, 256)], ids=['n1024', 'n4352'])
def test_head_accumulates_on_a_second_pass(d, T, B, monkeypatch):
    """Two forward / backward passes without zeroing in between: the second is not the first product into the tied matrix's
    gradient, so it must add to it, not store over it.  Twice the reference, from twice the terms."""
    head = _band_head(d, T, B)
    ref = head.reference('plain', head.H, head.y)
    spy = _HeadSpy(monkeypatch)
    dists = []
    for k in (1, 2):
        spy.clear()
        got = head.run(head.H, head.y, scores=False, zero=(k == 1))
        spy.assert_band(head, False, fresh=(k == 1))
        dists.append(_distances(head, got, ref, passes=k))
        print('n = %d, pass %d: distance / bound %s' % (head.n, k, ', '.join('%s %.3g' % kv for kv in sorted(dists[-1].items()))))
    WORST['d = %d, n = %d, second pass' % (d, head.n)] = ('accumulated', dists[1])
    for k, dist in enumerate(dists):
        for key in ('loss', 'dH', 'dE', 'db'):
            assert dist[key] <= 1.0, (head.n, 'pass %d' % (k + 1), key, dist[key])
    _assert_rest_of_the_arena_zero(head, 'n = %d after two passes' % head.n)


def test_zz_report_every_band():
    """Not a check: the branch each band took and what its bounds were reached by (run with -s or -rP)."""
    for what in sorted(WORST):
        took, dist = WORST[what]
        print('%-36s %-62s %s' % (what, took, ' '.join('%s %.3f' % (k, dist[k]) for k in ('loss', 'dH', 'dE', 'db'))))
