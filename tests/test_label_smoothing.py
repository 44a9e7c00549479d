"""Label smoothing of the vocabulary head without a pass over the logits (csrc/smooth.hip): the two new
streaming kernels on their own, the head on every dispatch route against fp64 at eps = 0.1 with eps = 0 as the control, what
must not change (eps = 0 launches, evaluation), the cached mean row across optimizer steps, and the trainer's steps.

The definition is PyTorch's cross_entropy(label_smoothing=eps); m3p_amd.functional.label_smoothing_ref is its fp64 correction
on top of the plain head (tests/test_label_smoothing_cpu.py holds that twin to PyTorch)."""
import gc
import math
import os
import traceback

import pytest
import torch

from m3p_amd import synth
from tests.util import (ATTN_CTX_RTOL, BF16_OUT, F32_OUT, KAPPA, ROW_FLOOR, U32, accum_bound, assert_bits_equal,
                        assert_exact_zero, assert_guards, block_bound, gemm_bound, guarded, rel_l2)

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
SHIFT = 40.0
EPS = 0.1
NEW_LAUNCHERS = ('vocab_mean', 'ls_colsum_rows', 'ls_row_aux', 'ls_sum_rows', 'ce_shift_dh_smooth', 'ls_uniform_add')


# ---------------------------------------------------------------------------------------------------------------------
# The mean row: ordered two-stage column sums.
# ---------------------------------------------------------------------------------------------------------------------
def _rows_per_period(d):
    return 8 // math.gcd(d, 8)          # a period of lcm(d, 8) elements holds whole 16-byte chunks (csrc/smooth.hip)


@pytest.mark.parametrize('d', [4, 260, 768])
@pytest.mark.parametrize('which', ['V5', 'V300', 'two-partials', 'capped-grid'])
def test_vocab_mean_every_column(which, d):
    """Every column of e_bar and b_bar against the fp64 mean under accum_bound for V terms; pad rows of 1e30 behind row V - 1 (and
    behind bias[V - 1]) must not show; two runs give the same bits.  `two-partials`: the smallest V at which the second stage adds
    more than one first-stage partial per (period row, column) - the grid rule gives a second group of periods once the first
    holds 32.  `capped-grid`: the first-stage grid at its cap, every thread on the unrolled loop."""
    from m3p_amd import ops, lib as L
    plan = L.load().m3p_vocab_mean_plan
    if which == 'two-partials':
        V = 32 * _rows_per_period(d) + 1
        assert plan(V, d) == 2 and plan(V - 1, d) == 1
    elif which == 'capped-grid':
        chunks = d // math.gcd(d, 8)
        V = (131072 // chunks) * 32 * _rows_per_period(d) + 5
        assert plan(V, d) == 131072 // chunks and plan(V, d) * 32 < -(-V // _rows_per_period(d))
    else:
        V = int(which[1:])
    g = torch.Generator(device='cuda').manual_seed(V + d)
    pad = 5
    emb = (torch.randn((V + pad, d), device='cuda', generator=g) * 0.3 + 0.05).to(BF16)
    bias = torch.randn((V + pad,), device='cuda', generator=g) * 0.5 + 0.1
    emb[V:] = 1e30
    bias[V:] = 1e30
    out = ops.vocab_mean(emb, bias, V)
    again = ops.vocab_mean(emb, bias, V)
    torch.cuda.synchronize()
    assert out.shape == (d + 1,) and out.dtype == torch.float32
    assert_bits_equal(again, out, 'vocab_mean twice')
    e64, b64 = emb[:V].double(), bias[:V].double()
    w_e, at = accum_bound(out[:d], e64.mean(0), e64.abs().mean(0), V)
    w_b, _ = accum_bound(out[d:], b64.mean().reshape(1), b64.abs().mean().reshape(1), V)
    print('vocab_mean V = %d, d = %d (%d partials): e_bar %.3g, b_bar %.3g of the bound' % (V, d, plan(V, d), w_e, w_b))
    assert w_e <= 1.0, (w_e, at)
    assert w_b <= 1.0, w_b


@pytest.mark.parametrize('n,d', [(7, 64), (4096, 256)])
def test_ordered_column_sums_of_the_rows(n, d):
    """ls_colsum_rows (the same two stages with a caller's scale) against fp64, twice the same bits."""
    from m3p_amd import ops
    g = torch.Generator(device='cuda').manual_seed(n)
    h = torch.randn((n, d), device='cuda', generator=g).to(BF16)
    scale = -0.1 / (n * 1000)
    out, again = ops.ls_colsum_rows(h, scale), ops.ls_colsum_rows(h, scale)
    assert_bits_equal(again, out, 'ls_colsum_rows twice')
    h64 = h.double()
    worst, at = accum_bound(out, scale * h64.sum(0), abs(scale) * h64.abs().sum(0), n)
    assert worst <= 1.0, (worst, at)


# ---------------------------------------------------------------------------------------------------------------------
# The uniform add.
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V,d', [(5, 4), (300, 260), (2100, 1000)])
def test_uniform_add_touches_v_rows_only(V, d):
    """dst[v, :] += g u and dbias[v] += g db for v < V, each element one fp32 multiply-add of exact inputs; the rows from V on
    (in the arena: the head of the bias gradient) and the guard rows around both buffers keep their bits.  [2100, 1000] has more
    16-byte chunks than the capped grid has threads: the grid-stride loop takes a second trip."""
    from m3p_amd import ops, lib as L
    blocks = L.load().m3p_ls_uniform_add_plan(V, d)
    if V == 2100:
        assert V * d // 4 > blocks * 256
    else:
        assert V * d // 4 <= blocks * 256
    extra = 4
    gen = torch.Generator(device='cuda').manual_seed(V)
    buf, dst = guarded(V + extra, d, torch.float32)
    bbuf, db2 = guarded(V + extra, 1, torch.float32)
    dst.copy_(torch.randn((V + extra, d), device='cuda', generator=gen))
    db2.copy_(torch.randn((V + extra, 1), device='cuda', generator=gen))
    dbias = db2.view(-1)
    dst0, dbias0 = dst.clone(), dbias.clone()
    u = torch.randn((d,), device='cuda', generator=gen)
    gup = torch.tensor([0.5], device='cuda')
    dbv = -0.1 / V
    ops.ls_uniform_add(dst, dbias, u, gup, dbv, V)
    torch.cuda.synchronize()
    assert_guards(buf, 'uniform add, matrix')
    assert_guards(bbuf, 'uniform add, bias')
    assert_bits_equal(dst[V:], dst0[V:], 'rows from V on')
    assert_bits_equal(dbias[V:], dbias0[V:], 'bias elements from V on')
    add = 0.5 * u.double()
    ref = dst0[:V].double() + add
    worst, at = gemm_bound(dst[:V], ref, torch.zeros_like(ref), 0, 0.0, F32_OUT * (dst0[:V].double().abs() + add.abs()))
    assert worst <= 1.0, (worst, at)
    refb = dbias0[:V].double() + 0.5 * float(torch.tensor(dbv, dtype=torch.float32))
    errb = (dbias[:V].double() - refb).abs() / (F32_OUT * (dbias0[:V].double().abs() + abs(0.5 * dbv)) + 1e-300)
    assert float(errb.max()) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# The head on every dispatch route.
# ---------------------------------------------------------------------------------------------------------------------
def _reference(H, E, b, y, g, eps, stored):
    """fp64 loss and gradients of the tied projection + mean cross-entropy (label_smoothing = eps) times the upstream gradient g,
    with the sums of absolute values the bounds take: tests/test_mlm_shifted_gpu.py's reference, its sums extended by the
    correction's terms.  stored: the route keeps the logits in bf16 (one more rounding of every logit in the exponent)."""
    from m3p_amd.functional import label_smoothing_ref
    n, d = H.shape
    V = E.shape[0]
    rows = torch.arange(n, device=H.device)
    H64, E64, b64 = H.double(), E.double(), b.double()
    x = H64 @ E64.t() + b64
    ax = H64.abs() @ E64.abs().t() + b64.abs()
    lse = torch.logsumexp(x, 1)
    loss_n = lse - x[rows, y]
    t = x[rows, y]
    P = torch.exp(x - lse[:, None])
    accx = KAPPA * math.sqrt(d) * U32 * ax.max(1).values
    # (the project's bound for dE: every logit perturbed relative to itself, |delta_nv| <= |x_nv|)
    S = (P * x.abs()).sum(1, keepdim=True)
    xG = P * (x.abs() + S) * (abs(g) / n)
    # for dH, element by element, the same first-order model without the slack: a perturbation delta of the logits moves p_v by
    # p_v sum_{w != v} p_w (delta_v - delta_w), here |delta_nv| <= D_nv = BF16_OUT |x_nv| (logits stored in bf16) + the GEMM's
    # element bound; and the fp32 evaluation of the exponent, relative to its operands (the logit, the log-sum-exp or the shift)
    D = accx[:, None] + (BF16_OUT * x.abs() if stored else 0.0)
    SD = (P * D).sum(1, keepdim=True)
    xGt = P * (D * (1.0 - 2.0 * P) + SD).clamp(min=0.0) + P * F32_OUT * (x.abs() + lse.abs()[:, None] + t.abs()[:, None] + SHIFT)
    xGt *= abs(g) / n
    del D
    G = P
    G[rows, y] = torch.expm1(-loss_n)                              # p_y - 1 without cancellation
    G *= g / n
    aE = E64.abs()
    ref = dict(loss=float(loss_n.mean()), t=t, accx=accx, dH=G @ E64, adH=G.abs() @ aE, xdH=xGt @ aE, dE=G.t() @ H64,
               adE=G.abs().t() @ H64.abs(), xdE=xG.t() @ H64.abs(), db=G.sum(0), adb=G.abs().sum(0),
               xdEt=xGt.t() @ H64.abs(), xdbt=xGt.sum(0))
    ref['loss_bound'] = float((BF16_OUT * (1.0 + t.abs()) + 2.0 * accx).mean())
    ref['corr_dH'] = torch.zeros_like(ref['dH'])
    ref['corr_adH'] = torch.zeros_like(ref['dH'])
    if eps > 0:
        c = eps / n
        l_c, dh_c, de_c, db_c = label_smoothing_ref(H, E, b, y, eps, g=g)
        e_bar, a_bar = E64.mean(0), aE.mean(0)
        ref['loss'] += float(l_c)
        # the rows' term in fp32: two depth-d dot products and a few roundings of their difference; the mean row's own error
        aux_abs = ax[rows, y] + H64.abs() @ a_bar + b64.abs().mean()
        ref['loss_bound'] += eps * float((KAPPA * math.sqrt(d) * U32 * aux_abs + F32_OUT * aux_abs +
                                          KAPPA * math.sqrt(V) * U32 * (H64.abs() @ a_bar + b64.abs().mean())).mean())
        ref['corr_dH'] = dh_c
        ref['corr_adH'] = abs(g) * c * (aE[y] + a_bar[None, :])
        ref['dH'] = ref['dH'] + dh_c
        ref['dE'] = ref['dE'] + de_c
        ref['adE'] = ref['adE'] + abs(g) * c * (torch.zeros_like(aE).index_add_(0, y, H64.abs()) + H64.abs().sum(0) / V)
        cnt = torch.bincount(y, minlength=V).double()
        ref['db'] = ref['db'] + db_c
        ref['adb'] = ref['adb'] + abs(g) * c * (cnt + n / V)
    return ref


class _Head:
    """An MLM head of T x B predicted rows over a vocabulary matrix of this test's own (logits of a random row ~ N(0, 1.2^2) +
    bias).  Seven rows of eight are a multiple of their target's embedding row - a model that has learnt something: the target's
    probability is about 0.97 (the multiple is calibrated for it) - the eighth is noise.  Targets include word 0, word V - 1 and
    an id that repeats."""
    G_UP = 0.5

    def __init__(self, d, V, T, B):
        from m3p_amd.model.transformer import TransformerModel
        self.d, self.V, self.T, self.B, self.n = d, V, T, B, T * B
        P = synth.model_params(d, d // 64, 1, V)
        torch.manual_seed(0)
        m = TransformerModel(P, is_encoder=True, with_output=True, is_crossModal=True)
        sd = synth.golden_state_dict(synth.hot_param_shapes(P))
        g = torch.Generator().manual_seed(11)
        E = (torch.randn((V, d), generator=g) * (1.2 / math.sqrt(d))).to(BF16).float()
        b = torch.randn((V,), generator=g) * 0.5
        for k in sd:
            if k in ('embeddings.weight', 'pred_layer.proj.weight'):
                sd[k] = E.clone()
            if k == 'pred_layer.proj.bias':
                sd[k] = b.clone()
        missing, unexpected = m.load_state_dict(sd, strict=False)
        assert not unexpected
        self.m = m.cuda().train()
        self.E, self.b = E.cuda(), b.cuda()
        y = torch.randint(0, V, (self.n,), generator=g)
        y[0], y[1] = 0, V - 1
        y[10:20] = 123
        y[20] = y[21] = V - 1
        self.y = y.cuda()
        noise = torch.randn((self.n, d), generator=g).cuda()
        learnt = (torch.arange(self.n, device='cuda') % 8) != 7
        alpha = self._calibrate(self.E, self.b, self.y[learnt][:128])
        self.alpha = alpha
        self.H = torch.where(learnt[:, None], alpha * self.E[self.y], noise).to(BF16)
        self._refs = {}

    @staticmethod
    def _calibrate(E, b, y, want=0.03):
        """The multiple alpha at which rows alpha E[y] leave their targets a median probability of 1 - want."""
        E64, b64 = E.double(), b.double()
        lo, hi = 1.0, 64.0
        for _ in range(24):
            a = 0.5 * (lo + hi)
            x = a * (E64[y] @ E64.t()) + b64
            miss = -torch.expm1(x[torch.arange(len(y)), y] - torch.logsumexp(x, 1))
            lo, hi = (a, hi) if float(miss.median()) > want else (lo, a)
        return 0.5 * (lo + hi)

    def run(self, scores, eps):
        m = self.m
        m.label_smoothing = eps
        m.train()
        m.arena().zero_grad()
        tensor = self.H.view(self.T, self.B, self.d).clone().requires_grad_(True)
        mask = torch.ones((self.T, self.B), dtype=torch.bool, device='cuda')
        got_scores, loss = m('predict', tensor=tensor, pred_mask=mask, y=self.y, get_scores=scores)
        (loss * self.G_UP).backward()
        torch.cuda.synchronize()
        m.label_smoothing = 0.0
        own = dict(m.named_parameters())
        return dict(loss=float(loss), dH=tensor.grad.view(self.n, self.d).float().clone(), dE=own['embeddings.weight'].grad.clone(),
                    db=own['pred_layer.proj.bias'].grad.clone(), scores=got_scores)

    def reference(self, eps, stored):
        if (eps, stored) not in self._refs:
            self._refs[(eps, stored)] = _reference(self.H, self.E, self.b, self.y, self.G_UP, eps, stored)
        return self._refs[(eps, stored)]


# route -> (d, V, T, B, get_scores).  d = 64 and V = 1000 (V_pad = 1024 > V) wherever the route exists at that size; the stored
# weight gradient (KERN_WGRAD_W4_TILES) needs d % 256 == 0 and more 256 x 256 tiles of the padded matrix than the device has
# compute units, so that route runs at the smallest vocabulary that has them at d = 256
ROUTES = {
    'n40-in-place': (64, 1000, 5, 8, False),
    'n1024-shifted-accumulating': (64, 1000, 4, 256, False),
    'n4096-whole-tile-wgrad': (64, 1000, 16, 256, False),
    'n4096-scores': (64, 1000, 16, 256, True),
    'n4096-stored-wgrad': (256, None, 16, 256, False),
}


@pytest.fixture(scope='module')
def heads():
    """route -> (its head, get_scores): one model per shape, shared by the tests of this file and freed with its fp64
    references when the file is done."""
    from m3p_amd import lib as L
    cache = {}

    def get(route):
        d, V, T, B, scores = ROUTES[route]
        if V is None:
            V = (L.num_cus() + 1) * 256 - 200          # V_pad / 256 tiles > compute units, V_pad - V = 200 pad rows
        key = (d, V, T, B)
        if key not in cache:
            cache[key] = _Head(d, V, T, B)
        return cache[key], scores
    yield get
    for head in cache.values():
        head._refs.clear()
    cache.clear()
    gc.collect()
    torch.cuda.empty_cache()


class _Spy:
    """The launchers a forward / backward of the head went through."""
    NAMES = ('ce_fwd_bwd', 'ce_fwd_bwd_colsum', 'ce_from_block_stats', 'ce_shift_from_block_sums', 'ce_shift_colsum',
             'ce_shift_target_rows', 'ce_shift_dh', 'scale_bf16_dev') + NEW_LAUNCHERS

    def __init__(self, monkeypatch):
        from m3p_amd import ops
        self.calls, self.nt, self.wgrad = [], [], []
        real_nt, real_wg = ops.gemm_nt, ops.gemm_wgrad

        def nt(a, w, epilogue=0, **kw):
            self.nt.append((epilogue, a.shape[0], kw.get('n') or w.shape[0], kw.get('row_ref') is not None))
            return real_nt(a, w, epilogue, **kw)

        def wg(*a, **kw):
            out = real_wg(*a, **kw)
            self.wgrad.append((kw.get('n'), bool(kw.get('dw_is_zero')), kw.get('bias') is not None, out))
            return out

        def named(name, real):
            def f(*a, **kw):
                self.calls.append(name)
                return real(*a, **kw)
            return f
        monkeypatch.setattr(ops, 'gemm_nt', nt)
        monkeypatch.setattr(ops, 'gemm_wgrad', wg)
        for name in self.NAMES:
            monkeypatch.setattr(ops, name, named(name, getattr(ops, name)))

    def count(self, name):
        return self.calls.count(name)


def _assert_route(route, head, spy, scores):
    """The premise that puts the run on its route."""
    from m3p_amd import functional as Fn, lib as L
    assert Fn._CE_FUSED_LSE and Fn._VOCAB_FULL_TILES and Fn._VOCAB_WGRAD_BIAS
    ar = head.m.arena()
    n, V, Vp, d = head.n, head.V, ar.V_pad, head.d
    assert Vp > V
    plan = L.load().m3p_gemm_wgrad_plan(n, Vp, d)
    if route == 'n40-in-place':
        assert spy.nt == [(L.EPI_BIAS, n, V, False)] and spy.count('ce_fwd_bwd') == 1 and spy.wgrad[0][:2] == (V, False)
    elif route == 'n1024-shifted-accumulating':
        assert spy.nt == [(L.EPI_BIAS_LSE, n, Vp, True)] and spy.count('ce_shift_from_block_sums') == 1
        assert spy.wgrad[0][:2] == (V, False)
    elif route == 'n4096-whole-tile-wgrad':
        assert spy.nt == [(L.EPI_BIAS_LSE, n, Vp, True)] and spy.count('ce_shift_from_block_sums') == 1
        assert spy.wgrad[0][:2] == (Vp, True) and plan != L.KERN_WGRAD_W4_TILES
    elif route == 'n4096-scores':
        assert spy.nt == [(L.EPI_BIAS_LSE, n, Vp, False)] and spy.count('ce_from_block_stats') == 1
        assert spy.wgrad[0][:2] == (Vp, True)
    else:
        assert plan == L.KERN_WGRAD_W4_TILES
        assert spy.nt == [(L.EPI_BIAS_LSE, n, Vp, True)] and spy.count('ce_shift_from_block_sums') == 1
        # stored, and the bias gradient's column sums came out of its K loop: no pass over e for them
        assert spy.wgrad[0][:3] == (Vp, True, True) and spy.wgrad[0][3] == (True, True) and ar.vocab_stored
        assert spy.count('ce_shift_colsum') == 0
    assert len(spy.wgrad) == 1


def _distances(head, got, ref, stored, widened):
    """Each output's distance from the fp64 reference in units of its bound (<= 1 passes).
    widened = False: the bounds of tests/test_mlm_shifted_gpu.py::_distances and its caller, as they stand there - the loss,
      the rows of dH (ATTN_CTX_RTOL, ROW_FLOOR), dE (the stored logits' rounding xdE counted where the logits are stored in bf16
      AND fewer than 4096 rows are summed) and db - with the smoothed reference and the correction's terms in the sums of
      absolute values.  Every route that does not store its logits is held to these.
    widened = True, for the two routes that store the logits in bf16 and read them back (one more rounding |delta x| <=
      BF16_OUT |x| in the exponent): that file's logits are ~ N(0, 1.2^2), these rows carry a target logit near 12, and
      test_bf16_logits_force_the_wider_bounds shows with an fp64 restatement of the path that has nothing but its bf16
      roundings that they cannot meet three of those bounds.  Those three count the rounding by the first-order model of
      _reference (xGt: p_v moves by p_v sum_{w != v} p_w (delta_v - delta_w), which keeps the target's own term small on a
      confident row): db gets its column sums (xdbt), dE at 4096 rows its products with |H| (xdEt; below 4096 rows the
      project's own xdE stays), and the rows of dH are held element by element only (xdH), not to 2^-7 of the row.
    dH element by element, on every route:
      one bf16 rounding of the output; the accumulation over V terms; the first operand of the product rounded to bf16 once
      (e, or the gradient rewritten over the logits) and its normaliser summed from rounded values, BF16_OUT sum |G| |E| each;
      what the error of the logits and the fp32 exponent move the softmax by (_reference: xdH); the correction's own fp32
      evaluation, F32_OUT (eps / n)(|E[y]| + |e_bar|), and the mean row's accumulation error over V terms."""
    assert stored or not widened
    below = head.n < 4096
    out = {'loss': abs(got['loss'] - ref['loss']) / ref['loss_bound']}
    if not widened:
        out['dH rows'] = block_bound(got['dH'], ref['dH'], ('row',), ATTN_CTX_RTOL, ROW_FLOOR)[2]
    eps_h = BF16_OUT * 2.0 * ref['adH'] + ref['xdH'] + (F32_OUT + KAPPA * math.sqrt(head.V) * U32) * ref['corr_adH']
    if stored:
        eps_h = eps_h + BF16_OUT * ref['adH']       # (the exponent read back from bf16 is in xdH; the gradient is rounded again)
    out['dH'] = gemm_bound(got['dH'], ref['dH'], ref['adH'] + ref['corr_adH'], head.V, BF16_OUT, eps_h)[0]
    eps_e = BF16_OUT * ref['adE']
    if stored and below:
        eps_e = eps_e + BF16_OUT * ref['xdE']
    elif widened:
        eps_e = eps_e + ref['xdEt']
    out['dE'] = gemm_bound(got['dE'], ref['dE'], ref['adE'], head.n, F32_OUT, eps_e)[0]
    out['db'] = accum_bound(got['db'], ref['db'], ref['adb'], head.n, BF16_OUT * ref['adb'] + (ref['xdbt'] if widened else 0.0))[0]
    # the bound of every element of dH, for the premise below
    out['dH bound'] = (BF16_OUT * ref['dH'].abs() + KAPPA * math.sqrt(head.V) * U32 * (ref['adH'] + ref['corr_adH']) + eps_h)
    return out


def _restated_stored_path(head):
    """The route that stores its logits in bf16, restated in fp64 with nothing but its bf16 roundings (the form of
    tests/test_parity_bounds.py): the logits rounded once, the log-sum-exp and the softmax from the rounded values, the gradient
    (p - onehot) / n rounded into their place, exact products with E and with g H (g = 1/2: exact), dH rounded once."""
    bf = lambda t: t.float().to(BF16).double()                      # noqa: E731
    n = head.n
    rows = torch.arange(n, device='cuda')
    H64, E64, b64, g = head.H.double(), head.E.double(), head.b.double(), head.G_UP
    xb = bf(H64 @ E64.t() + b64)
    lse = torch.logsumexp(xb, 1)
    G = torch.exp(xb - lse[:, None])
    G[rows, head.y] -= 1.0
    Gb = bf(G / n)
    return dict(loss=float((lse - xb[rows, head.y]).mean()), dH=bf(g * (Gb @ E64)), dE=g * (Gb.t() @ H64), db=g * Gb.sum(0))


STORED_ROUTES = ['n40-in-place', 'n4096-scores']


@pytest.mark.parametrize('route', STORED_ROUTES)
def test_bf16_logits_force_the_wider_bounds(route, heads):
    """Why the two routes that store bf16 logits are not held to tests/test_mlm_shifted_gpu.py's bounds on these inputs: the
    fp64 restatement of the path, with its bf16 roundings and no other error, already exceeds the rows-of-dH bound, the db
    bound and - at 4096 rows - the dE bound (asserted).  And the terms that replace them are no wider than that: under the
    widened bounds the same restatement stays within 1 and reaches at least 1/8 of each - a worst-case sum of roundings that each
    reach half their bound on average and partly cancel leaves about that much; a term an order of magnitude too generous would
    not."""
    head, scores = heads(route)
    ref = head.reference(0.0, True)
    got = _restated_stored_path(head)
    plain = _distances(head, got, ref, stored=True, widened=False)
    wide = _distances(head, got, ref, stored=True, widened=True)
    plain.pop('dH bound'), wide.pop('dH bound')
    print('%s restated in fp64 with its bf16 roundings: project bounds %s; widened %s' % (
        route, ', '.join('%s %.3g' % kv for kv in plain.items()), ', '.join('%s %.3g' % kv for kv in wide.items())))
    forced = ['dH rows', 'db'] + (['dE'] if head.n >= 4096 else [])
    for k in forced:
        assert plain[k] > 1.0, (route, k, plain[k])
    for k in ['dH', 'db'] + (['dE'] if head.n >= 4096 else []):
        assert 0.125 <= wide[k] <= 1.0, (route, k, wide[k])


def _assert_pad_region(head, what):
    """The weight gradient's pad rows V .. V_pad - 1 alias the head of the bias gradient (and, at d = 64, what follows it): after
    backward everything in the gradient arena outside the tied matrix and the output bias is exactly zero - the bias gradient
    itself is held to its bound by the caller - so nothing was added to the pad rows."""
    ar = head.m.arena()
    assert ar.stale is None
    o, cnt, _ = ar.offsets['embeddings.weight']
    ob, cntb, _ = ar.offsets['pred_layer.proj.bias']
    assert cnt == head.V * head.d and ob == o + cnt and ar.V_pad > head.V         # the bias gradient IS the pad rows' head
    rest = ar.grad.clone()
    rest[o:o + cnt] = 0
    rest[ob:ob + cntb] = 0
    assert_exact_zero(rest, what + ': the gradient arena outside embeddings.weight and pred_layer.proj.bias')


@pytest.mark.parametrize('eps', [EPS, 0.0], ids=['eps0.1', 'eps0-control'])
@pytest.mark.parametrize('route', list(ROUTES))
def test_head_on_every_route(route, eps, heads, monkeypatch):
    """model.predict forward and backward against the fp64 smoothed cross-entropy, every element of the loss, dH, dE (all V
    rows) and db within the plain head's bound on that route (_distances; the two routes that store bf16 logits under the
    bounds test_bf16_logits_force_the_wider_bounds justifies); eps = 0 is the control that shows the bound is the plain head's.
    Premise of the eps = 0.1 runs: on at least half of dH's elements the correction is more than ten times the element's
    bound - a head that ignores label_smoothing fails."""
    head, scores = heads(route)
    spy = _Spy(monkeypatch)
    got = head.run(scores, eps)
    _assert_route(route, head, spy, scores)
    new = [spy.count(k) for k in NEW_LAUNCHERS]
    if eps == 0:
        assert new == [0] * len(NEW_LAUNCHERS), dict(zip(NEW_LAUNCHERS, new))
    else:
        assert spy.count('ls_row_aux') == spy.count('ce_shift_dh_smooth') == spy.count('ls_uniform_add') == 1
        # (the data gradient's closing pass is the smoothed one; scale_bf16_dev still scales the plain routes' second operand)
        assert spy.count('ce_shift_target_rows') == 1 and spy.count('ce_shift_dh') == 0 and spy.count('scale_bf16_dev') <= 1
    n = head.n
    in_bf16 = scores or n % 256 != 0 or n < 1024         # the logits are stored in bf16 and rewritten into their gradient
    ref = head.reference(eps, in_bf16)
    dist = _distances(head, got, ref, stored=in_bf16, widened=in_bf16)
    assert in_bf16 == (route in STORED_ROUTES)
    bound = dist.pop('dH bound')
    print('%s, eps = %g (alpha %.2f): distance / bound %s' % (route, eps, head.alpha, ', '.join('%s %.3g' % kv for kv in dist.items())))
    if eps > 0:
        frac = float((ref['corr_dH'].abs() > 10.0 * bound).double().mean())
        print('%s: the correction exceeds 10 x the bound on %.1f %% of dH' % (route, 100 * frac))
        assert frac >= 0.5, frac
    for k, v in dist.items():
        assert v <= 1.0, (route, eps, k, v)
    if scores:
        x = head.H.double() @ head.E.double().t() + head.b.double()
        assert got['scores'].shape == (n, head.V)
        assert float((got['scores'].double() - x).abs().max()) <= BF16_OUT * float(x.abs().max()) + 1e-3     # the raw logits
    _assert_pad_region(head, route)


# ---------------------------------------------------------------------------------------------------------------------
# The trainer: eps = 0 launches nothing new, the cached mean row, the logged loss, a one-rank data-parallel world.
# ---------------------------------------------------------------------------------------------------------------------
def _clm_trainer(eps, **over):
    from m3p_amd.trainer import XTrainer
    from tests.test_clm import _model, _step_case
    P, sd, x, lengths, langs, pred_mask, y = _step_case(**over)
    P.label_smoothing = eps
    m = _model(P, sd)
    assert m.label_smoothing == eps
    return XTrainer(m, {}, P), m, (x, lengths, pred_mask, y, 'zh', 1.0), dict(langs=langs)


def _mt_trainer(eps):
    from m3p_amd.trainer import XTrainer
    from tests.test_seq2seq_tiled import _model
    P, sd, x1, len1, x2, len2 = synth.mt_case()
    for k, v in synth.trainer_params(batch_size=int(len1.numel()), langs=['en', 'zh'], mt_steps=[('en', 'zh')]).items():
        setattr(P, k, v)
    P.label_smoothing = eps
    m = _model(P, sd)
    return XTrainer(m, {}, P), m, (x1, len1, x2, len2, 'en', 'zh', 1.0), {}


def _spy_new(monkeypatch, capture=None):
    from m3p_amd import ops
    seen = {k: 0 for k in NEW_LAUNCHERS}
    for name in NEW_LAUNCHERS:
        def f(*a, _real=getattr(ops, name), _name=name, **kw):
            seen[_name] += 1
            out = _real(*a, **kw)
            if capture is not None and _name == 'ls_row_aux':
                capture.append((a[0].clone(), out.clone()))
            return out
        monkeypatch.setattr(ops, name, f)
    return seen


def test_eps_zero_launches_nothing_new(monkeypatch):
    """Over a training step with label_smoothing = 0 none of the new launchers is called; with 0.1 each one is."""
    seen = _spy_new(monkeypatch)
    tr, m, args, kw = _clm_trainer(0.0)
    tr.clm_step_on_batch(*args, **kw)
    torch.cuda.synchronize()
    assert seen == {k: 0 for k in NEW_LAUNCHERS}, seen
    tr, m, args, kw = _clm_trainer(EPS)
    tr.clm_step_on_batch(*args, **kw)
    torch.cuda.synchronize()
    assert all(v == 1 for v in seen.values()), seen


def test_cached_mean_row_follows_the_optimizer(monkeypatch):
    """One mean-row launch per state of the weights: after two optimizer steps the arena's cached row equals a freshly computed
    one bit for bit (and no longer the first step's), and asking again launches nothing."""
    from m3p_amd import ops
    seen = _spy_new(monkeypatch)
    tr, m, args, kw = _clm_trainer(EPS)
    ar = m.arena()
    ar.refresh()
    first = ar.vocab_mean().clone()
    for _ in range(2):
        tr.clm_step_on_batch(*args, **kw)
    torch.cuda.synchronize()
    # (the first step reuses the row computed above; its optimizer step invalidates it and the second step computes its own)
    assert seen['vocab_mean'] == 2, seen
    ar.refresh()
    cached = ar.vocab_mean()
    assert seen['vocab_mean'] == 3 and ar.vocab_mean() is cached and seen['vocab_mean'] == 3
    fresh = ops.vocab_mean(ar.w('embeddings.weight'), ar.p('pred_layer.proj.bias'), m.n_words)
    assert_bits_equal(cached, fresh, 'cached mean row after two optimizer steps')
    assert not torch.equal(cached, first)


def test_evaluation_is_not_smoothed(heads):
    """predict_stats and eval-mode predict give the same bits under label_smoothing = 0.1 and 0."""
    head, _ = heads('n1024-shifted-accumulating')
    m = head.m
    tensor = head.H.view(head.T, head.B, head.d).clone()
    mask = torch.ones((head.T, head.B), dtype=torch.bool, device='cuda')
    res = {}
    try:
        for eps in (EPS, 0.0):
            m.label_smoothing = eps
            m.eval()
            with torch.no_grad():
                stats = m.predict_stats(tensor, mask, head.y)
                scores, loss = m('predict', tensor=tensor, pred_mask=mask, y=head.y, get_scores=True)
            m.train()
            _, train_loss = m('predict', tensor=tensor, pred_mask=mask, y=head.y, get_scores=False)
            res[eps] = (stats[0].clone(), stats[1].clone(), scores.clone(), loss.detach().clone(), float(train_loss))
    finally:
        m.label_smoothing = 0.0
        m.train()
    for k, name in enumerate(('predict_stats loss sum', 'predict_stats hits', 'eval-mode scores', 'eval-mode loss')):
        assert_bits_equal(res[EPS][k].reshape(-1), res[0.0][k].reshape(-1), name)
    assert res[EPS][4] - res[0.0][4] > 0.01          # (training mode on the same rows IS smoothed)


@pytest.mark.parametrize('step', ['clm', 'mt'])
def test_trainer_logs_the_smoothed_loss(step, monkeypatch):
    """Three clm / mt steps at eps = 0.1: finite losses, one statistic each.  On the first step - the same weights and batch as a
    model with eps = 0 - the logged loss minus the plain one is the fp64 aux term of the rows the head was handed: both losses
    are fp32 numbers (a rounding each) and the term carries the fp32 dot products of depth d over |h| (|E[y]| + |e_bar|)."""
    make = _clm_trainer if step == 'clm' else _mt_trainer
    fn = 'clm_step_on_batch' if step == 'clm' else 'mt_step_on_batch'
    tr0, m0, args, kw = make(0.0)
    plain = float(getattr(tr0, fn)(*args, **kw))
    captured = []
    seen = _spy_new(monkeypatch, captured)
    tr, m, args, kw = make(EPS)
    if step == 'clm':
        y = args[3]
    else:
        x2, len2 = args[2], args[3]
        alen = torch.arange(int(len2.max()))
        y = x2[1:].masked_select((alen[:, None] < len2[None] - 1)[:-1])
    ar = m.arena()
    ar.refresh()
    E64, b64 = ar.w('embeddings.weight').double().clone(), ar.p('pred_layer.proj.bias').double().clone()
    losses = [float(getattr(tr, fn)(*args, **kw)) for _ in range(3)]
    torch.cuda.synchronize()
    key = [k for k, v in tr.stats.items() if k.startswith(('CLM-', 'MT-')) and isinstance(v, list) and v]
    assert len(key) == 1 and len(tr.stats[key[0]]) == 3 and all(math.isfinite(v) for v in losses)
    assert [float(v) for v in tr.stats[key[0]]] == losses
    assert seen['ls_row_aux'] == 3 and len(captured) == 3
    from m3p_amd.functional import label_smoothing_ref
    h = captured[0][0]
    n, d = h.shape
    assert n == y.numel()
    yd = y.to(h.device)
    want = float(label_smoothing_ref(h, E64, b64, yd, EPS)[0])
    absum = (h.double().abs() * (E64[yd].abs() + E64.abs().mean(0))).sum(1) + b64[yd].abs() + b64.abs().mean()
    tol = EPS * float(((KAPPA * math.sqrt(d) + KAPPA * math.sqrt(m.n_words)) * U32 * absum + F32_OUT * absum).mean()) \
        + 2 * F32_OUT * (abs(plain) + abs(losses[0]))
    print('%s step: loss %.6f, plain %.6f, difference %.6f against the fp64 aux term %.6f (tolerance %.2e)' % (
        step, losses[0], plain, losses[0] - plain, want, tol))
    assert abs(want) > 10 * tol                      # (the term is told from zero)
    assert abs((losses[0] - plain) - want) <= tol


# ---- a forced one-rank data-parallel world (the pattern of tests/test_clm.py) against the plain step, both at eps = 0.1
def _one_step(multi_gpu):
    tr, m, args, kw = _clm_trainer(EPS, multi_gpu=multi_gpu, is_master=True)
    loss = float(tr.clm_step_on_batch(*args, **kw))
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
        q.put(('ok', loss, m.arena().master.float().cpu().numpy(), wrapped))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        q.put(('err', traceback.format_exc(), None, False))
        raise


def test_smoothed_step_in_a_one_rank_world_matches_the_plain_step():
    """The eps = 0.1 clm step through the data-parallel path (buckets, hooks, mlm_head_done behind the correction) ends in the
    same weights as the single-device step, to that step's own run-to-run noise - measured by running it twice."""
    import torch.multiprocessing as mp
    from tests.test_clm import _free_port
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    proc = ctx.Process(target=_dp_worker, args=(_free_port(), q))
    proc.start()
    status, loss_dp, master_dp, wrapped = q.get(timeout=600)
    proc.join(timeout=120)
    assert status == 'ok', loss_dp
    assert wrapped, 'M3P_DP_FORCE=1 did not put the one-rank world on the data-parallel path'
    runs = []
    for _ in range(2):
        tr, m, loss = _one_step(False)
        runs.append((loss, m.arena().master.float().cpu().clone()))
    noise = rel_l2(runs[1][1], runs[0][1])
    diff = rel_l2(torch.from_numpy(master_dp), runs[0][1])
    print('one-rank world at eps = 0.1: loss %.6f against %.6f, weights differ by %.3e (run-to-run noise %.3e)' % (
        loss_dp, runs[0][0], diff, noise))
    assert abs(loss_dp - runs[0][0]) <= 2 * F32_OUT * abs(runs[0][0]) + abs(runs[1][0] - runs[0][0])
    assert diff <= max(10 * noise, 1e-7), (diff, noise)
