"""The grouped whole-tile weight-gradient launch (m3p_gemm_wgrad_group_bf16: up to twelve products dW_k += alpha dY_k^T X_k over
one M, one workgroup per 256 x 256 output tile over all of M, csrc/gemm_wgrad_w4.hpp), its placement table, and the queue of
the encoder's backward loop that feeds it (functional.WgradQueue).

Every element is held to the accumulation bound of tests/util.py against an fp64 product: one output element is ONE running
fp32 sum of M products (the MFMA accumulator), added once to what dW held - n_terms = M + 1, sum|terms| = |dW0| + |alpha|
|dY|^T |X|.  M = 4096 is the smallest M the four-wave kernel takes (64 K-tiles); M = 4160 = 65 K-tiles ends the K loop, which
is unrolled by two, on its odd tail."""
import pytest
import torch

from m3p_amd import lib as L
from m3p_amd import ops
from tests.util import assert_accum_bound, assert_bits_equal

gpu = pytest.mark.gpu
GUARD = 2            # poisoned rows above and below a dW, and (4 columns = 16 bytes, the alignment the launch asks for) beside it
GCOL = 4


def _randn(shape, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    return torch.randn(shape, generator=g, device='cuda', dtype=torch.float32)


class Product:
    """One item: operands with pitches wider than their widths, a nonzero dW inside a poisoned frame, its fp64 reference."""

    def __init__(self, M, N, K, seed, alpha, operands=None):
        self.N, self.K = N, K
        if operands is None:
            operands = (_randn((M, N + 8), seed).to(torch.bfloat16), _randn((M, K + 16), seed + 1).to(torch.bfloat16))
        self.operands = operands
        self.dy, self.x = operands[0][:, :N], operands[1][:, :K]
        self.frame = torch.empty((N + 2 * GUARD, K + 2 * GCOL), dtype=torch.float32, device='cuda')
        self.frame.untyped_storage().fill_(0xFF)
        self.dw = self.frame[GUARD:GUARD + N, GCOL:GCOL + K]
        self.dw0 = _randn((N, K), seed + 2)
        self.reset()
        y64, x64 = self.dy.double(), self.x.double()
        self.ref64 = self.dw0.double() + alpha * (y64.t() @ x64)
        self.abs64 = self.dw0.double().abs() + abs(alpha) * (y64.abs().t() @ x64.abs())
        self.M = M

    def reset(self):
        self.dw.copy_(self.dw0)
        self.before = self.frame.clone()

    def item(self):
        return (self.dy, self.x, self.dw)

    def check(self, what):
        assert_accum_bound(self.dw, self.ref64, self.abs64, self.M + 1, what=what)
        self.check_frame(what)

    def check_frame(self, what, dw_too=False):
        """Nothing outside dW (or nothing at all) has changed, bit for bit."""
        a, b = self.frame.clone(), self.before.clone()
        if not dw_too:
            a[GUARD:GUARD + self.N, GCOL:GCOL + self.K] = 0
            b[GUARD:GUARD + self.N, GCOL:GCOL + self.K] = 0
        assert_bits_equal(a, b, what + ': the frame around dW' if not dw_too else what + ': dW and its frame')


MIXED = [(768, 768), (256, 256), (512, 768), (256, 256), (768, 512), (256, 512), (512, 256), (512, 512), (256, 768)]   # 34 tiles
ALPHA = 0.375


def _mixed(M):
    return [Product(M, N, K, 100 + 10 * k, ALPHA) for k, (N, K) in enumerate(MIXED)]


@pytest.fixture(scope='module')
def mixed4096():
    return _mixed(4096)


@gpu
@pytest.mark.parametrize('M', [4096, 4160])
def test_mixed_group(M, mixed4096):
    prods = mixed4096 if M == 4096 else _mixed(M)
    for p in prods:
        p.reset()
    assert ops.gemm_wgrad_group([p.item() for p in prods], alpha=ALPHA)
    torch.cuda.synchronize()
    for k, p in enumerate(prods):
        p.check('item %d (%d x %d), M = %d' % (k, p.N, p.K, M))


@gpu
def test_grouped_against_ungrouped_and_twice(mixed4096):
    prods = mixed4096
    runs = []
    for _ in range(2):
        for p in prods:
            p.reset()
        assert ops.gemm_wgrad_group([p.item() for p in prods], alpha=ALPHA)
        torch.cuda.synchronize()
        runs.append([p.dw.clone() for p in prods])
    for k, (a, b) in enumerate(zip(*runs)):
        assert_bits_equal(a, b, 'item %d: two runs of the grouped launch' % k)
    for p in prods:
        p.reset()
    ops.gemm_wgrad_pair(*prods[0].item(), *prods[1].item(), alpha=ALPHA)
    for p in prods[2:]:
        ops.gemm_wgrad(*p.item(), alpha=ALPHA)
    torch.cuda.synchronize()
    for k, p in enumerate(prods):
        p.check('item %d through the per-product calls' % k)      # (the grouped results met the same bound in test_mixed_group)
        # one fp64 product bounds both: they differ from each other by at most twice the bound
        assert_accum_bound(runs[0][k], p.dw.double(), p.abs64, 4 * (p.M + 1), what='item %d grouped against ungrouped' % k)


def _shared(M, shapes, alpha):
    """Products that share their operands where the shapes repeat (the references are computed once per shape)."""
    first, out = {}, []
    for k, (N, K) in enumerate(shapes):
        if (N, K) not in first:
            first[(N, K)] = Product(M, N, K, 300 + 10 * k, alpha)
            out.append(first[(N, K)])
        else:
            f = first[(N, K)]
            p = Product.__new__(Product)
            p.N, p.K, p.M, p.operands, p.dy, p.x = N, K, M, f.operands, f.dy, f.x
            p.frame = f.before.clone()
            p.dw = p.frame[GUARD:GUARD + N, GCOL:GCOL + K]
            p.dw0, p.before, p.ref64, p.abs64 = f.dw0, f.before, f.ref64, f.abs64
            out.append(p)
    return out


def _boundary_shapes(kind):
    ncu = L.num_cus()
    if kind == 'one':
        return [(256, 256)]
    if kind == 'one9':
        return [(768, 768)]
    k = min(ncu // 36, 7)
    shapes = [(3072, 768), (768, 3072)] * 4
    shapes = shapes[:k]
    if kind == 'full':          # exactly one tile per CU: 36-tile products, then one (r x 1)-tile product
        r = ncu - 36 * k
        while r > 0:
            shapes.append((256 * min(r, 32), 256))
            r -= min(r, 32)
    return shapes


@gpu
@pytest.mark.parametrize('kind', ['one', 'one9', 'full', 'spill'])
def test_boundary_groups(kind):
    shapes = _boundary_shapes(kind)
    ncu = L.num_cus()
    tiles = [(N // 256, K // 256) for N, K in shapes]
    n_tiles = sum(a * b for a, b in tiles)
    if kind == 'full':
        assert n_tiles == ncu and len(shapes) <= L.WGRAD_GROUP_MAX
    if kind == 'spill':         # 36 tiles do not fit the 32 CUs of an XCD: every product's remainder lands on another one
        place = ops.wgrad_group_place(tiles, ncu)
        assert all(len({w % 8 for w, p in enumerate(place) if p is not None and p[0] == k}) == 2 for k in range(len(shapes)))
    prods = _shared(4096, shapes, 1.0)
    assert ops.gemm_wgrad_group([p.item() for p in prods])
    torch.cuda.synchronize()
    for k, p in enumerate(prods):
        p.check('%s: item %d (%d x %d)' % (kind, k, p.N, p.K))


def _raw(prods, M, alpha=1.0, n=None, patch=None):
    """The entry point's return code for these products (patch(array) may falsify fields the wrapper would assert on)."""
    n = len(prods) if n is None else n
    arr = (L.WgradItem * n)()
    for k, p in enumerate(prods):
        arr[k] = L.WgradItem(p.dy.data_ptr(), p.x.data_ptr(), p.dw.data_ptr(), p.dy.stride(0), p.x.stride(0), p.dw.stride(0), p.N, p.K)
    if patch:
        patch(arr)
    rc = L.load().m3p_gemm_wgrad_group_bf16(arr, n, M, alpha, L.stream())
    torch.cuda.synchronize()
    return rc


@gpu
def test_rejections_write_nothing():
    ncu = L.num_cus()
    M = 4160         # (the operands have 4160 rows, so that the M = 4100 case below names rows that exist)
    many = _shared(M, [(768, 3072)] * 12 + [(256, 256)], 1.0)
    big, small = many[:12], many[12]
    assert 36 * len(big) > ncu

    def unchanged(prods, what):
        for k, p in enumerate(prods):
            p.check_frame('%s, item %d' % (what, k), dw_too=True)
    assert _raw(big, M) == -2
    unchanged(big, 'more tiles than CUs')
    thirteen = [small] * 13
    assert _raw(thirteen, M) == -1
    unchanged([small], '13 items')
    assert _raw([], M, n=0) == -1

    def misalign(arr):
        arr[0].dW += 4          # one float on: 4-byte aligned, inside the frame (GCOL columns of room)
    assert _raw([big[0], small], M, patch=misalign) == -2
    unchanged([big[0], small], 'a misaligned dW')

    def narrow(arr):
        arr[1].lddw = small.K - 4
    assert _raw([big[0], small], M, patch=narrow) == -2
    unchanged([big[0], small], 'lddw < K')
    assert _raw([big[0], small], 4100) == -2
    unchanged([big[0], small], 'M not a multiple of 64')
    # ... and the same two products are taken as they are
    assert _raw([big[0], small], M) == 0
    big[0].check('accepted after the rejections: item 0')
    small.check('accepted after the rejections: item 1')


# ---------------------------------------------------------------------------------------------------------------------
# Placement (host only: no GPU)
# ---------------------------------------------------------------------------------------------------------------------
def _check_place(tiles, ncu):
    place = ops.wgrad_group_place(tiles, ncu)
    assert len(place) == ncu
    seen = [p for p in place if p is not None]
    want = [(k, i, j) for k, (ti, tj) in enumerate(tiles) for i in range(ti) for j in range(tj)]
    assert sorted(seen) == want, 'every tile exactly once'
    per_xcd = [sum(1 for w, p in enumerate(place) if p is not None and w % 8 == x) for x in range(8)]
    assert max(per_xcd) <= ncu // 8, per_xcd
    return place, [sorted({w % 8 for w, p in enumerate(place) if p is not None and p[0] == k}) for k in range(len(tiles))]


def test_placement_seven_products_of_36_tiles():
    place, xcds = _check_place([(3, 12), (12, 3)] * 3 + [(3, 12)], 256)
    for k, xs in enumerate(xcds):
        assert len(xs) <= 2, (k, xs)
        # 32 tiles of product k fill one XCD, the other four sit with the other products' remainders
        counts = sorted(sum(1 for w, p in enumerate(place) if p is not None and p[0] == k and w % 8 == x) for x in xs)
        assert counts == [4, 32], (k, counts)
    home = [max(xs, key=lambda x: sum(1 for w, p in enumerate(place) if p is not None and p[0] == k and w % 8 == x))
            for k, xs in enumerate(xcds)]
    assert len(set(home)) == 7, home                # seven XCDs hold one product's 32 tiles each
    # neighbouring workgroups of an XCD hold neighbouring tiles of a row panel
    x0 = [place[w] for w in range(xcds[0][0], 256, 8)]
    assert x0[:12] == [(0, 0, j) for j in range(12)]


def test_placement_of_the_layer_loop_and_other_grids():
    layer = [(3, 12), (12, 3), (9, 3), (3, 3)]
    place, xcds = _check_place((layer * 3)[:9], 256)            # lin2, lin1, q/k/v, out_lin, ... : 252 tiles, 9 items
    assert all(len(xs) <= 2 for xs in xcds), xcds
    _check_place((layer[2:] + layer * 2), 256)                   # a group that starts with the attention pair: 10 items
    _check_place([(3, 12)] * 6, 224)                             # a reduced persistent grid: 28 CUs per XCD
    _check_place([(1, 1)], 8)
    _check_place([(1, 1)] * 12, 256)
    _check_place([(16, 16)], 256)                                # one product on all eight XCDs
    gen = torch.Generator().manual_seed(5)
    for _ in range(200):
        n = int(torch.randint(1, 13, (1,), generator=gen))
        tiles = [(int(torch.randint(1, 7, (1,), generator=gen)), int(torch.randint(1, 7, (1,), generator=gen))) for _ in range(n)]
        ncu = 8 * int(torch.randint(1, 33, (1,), generator=gen))
        if sum(a * b for a, b in tiles) <= ncu:
            _check_place(tiles, ncu)
        else:
            with pytest.raises(L.M3PError):
                ops.wgrad_group_place(tiles, ncu)


# ---------------------------------------------------------------------------------------------------------------------
# The queue of the encoder's backward loop
# ---------------------------------------------------------------------------------------------------------------------
# three layers of cfg2's width at M = B * (T + R) = 4096: nine 36-tile units - seven fill one grouped launch, two are left
QUEUE_CFG = dict(emb_dim=768, n_heads=12, n_layers=3, n_words=5000, T=92, R=36, B=32, n_pred=8)
SMALL_CFG = dict(emb_dim=768, n_heads=12, n_layers=2, n_words=5000, T=40, R=36, B=6, n_pred=6)      # M = 456: nothing qualifies


def _backward(m, cfg, batch, monkeypatch, capacity):
    """One backward pass with the queue at `capacity` tiles -> (the layer products' (dy, x, dw) as the loop handed them over,
    the tile counts of the grouped launches, a copy of the whole gradient arena)."""
    from m3p_amd import functional as F
    from tests.test_model_parity import _losses
    products, groups = [], []
    real_add, real_group = F.WgradQueue.add, ops.gemm_wgrad_group

    def add(self, *unit):
        products.extend(unit)
        return real_add(self, *unit)

    def group(items, alpha=1.0):
        ok = real_group(items, alpha)
        if ok:
            groups.append(sum((dy.shape[1] // 256) * (x.shape[1] // 256) for dy, x, _ in items))
        return ok
    with monkeypatch.context() as mp:
        mp.setattr(F, 'WGRAD_QUEUE_TILES', capacity)
        mp.setattr(F.WgradQueue, 'add', add)
        mp.setattr(ops, 'gemm_wgrad_group', group)
        m.arena().zero_grad()
        out, mlm, rel, bce = _losses(m, batch, cfg['R'])
        (mlm + bce).backward()
        torch.cuda.synchronize()
    return products, groups, m.arena().grad.clone()


@gpu
def test_queue_in_the_layer_loop(monkeypatch):
    from m3p_amd import synth
    from tests.test_model_parity import _build
    cfg = QUEUE_CFG
    m, P, sd = _build(cfg)
    m.train()
    batch = synth.make_batch(cfg['T'], cfg['R'], cfg['B'], cfg['n_words'], cfg['n_pred'], seed=7)
    ncu = L.num_cus()
    for name, cap in (('default', None), ('one unit', 36)):
        products, groups, grad = _backward(m, cfg, batch, monkeypatch, cap)
        assert len(products) == 4 * cfg['n_layers']
        if cap == 36:
            assert groups == [36] * (3 * cfg['n_layers']), groups
        elif ncu == 256:
            assert groups == [252], groups
        # every layer weight gradient against the fp64 product of the very operands the loop handed over (the gradients were
        # zero before: one product each)
        for k, (dy, x, dw) in enumerate(products):
            y64, x64 = dy.double(), x.double()
            assert_accum_bound(dw, y64.t() @ x64, y64.abs().t() @ x64.abs(), dy.shape[0] + 1,
                               what='%s capacity: product %d (%d x %d)' % (name, k, dy.shape[1], x.shape[1]))


@gpu
def test_queue_leaves_small_products_alone(monkeypatch):
    from m3p_amd import synth
    from tests.test_model_parity import _build
    cfg = SMALL_CFG
    m, P, sd = _build(cfg)
    m.train()
    batch = synth.make_batch(cfg['T'], cfg['R'], cfg['B'], cfg['n_words'], cfg['n_pred'], seed=7)
    calls = []
    real_wg, real_pair = ops.gemm_wgrad, ops.gemm_wgrad_pair

    def wg(dy, x, dw, *a, **kw):
        calls[-1].append(('one', tuple(dy.shape), tuple(x.shape)))
        return real_wg(dy, x, dw, *a, **kw)

    def pair(dya, xa, dwa, dyb, xb, dwb, *a, **kw):
        calls[-1].append(('pair', tuple(dya.shape), tuple(xa.shape), tuple(dyb.shape), tuple(xb.shape)))
        return real_pair(dya, xa, dwa, dyb, xb, dwb, *a, **kw)
    monkeypatch.setattr(ops, 'gemm_wgrad', wg)
    monkeypatch.setattr(ops, 'gemm_wgrad_pair', pair)
    for cap in (None, 36, 0):           # (0: the queue switched off - the launches of the loop as they were)
        calls.append([])
        products, groups, grad = _backward(m, cfg, batch, monkeypatch, cap)
        assert len(products) == 4 * cfg['n_layers'] and groups == []
        for k, (dy, x, dw) in enumerate(products):
            y64, x64 = dy.double(), x.double()
            assert_accum_bound(dw, y64.t() @ x64, y64.abs().t() @ x64.abs(), dy.shape[0] + 1,
                               what='capacity %r: product %d (%d x %d)' % (cap, k, dy.shape[1], x.shape[1]))
    # the same launches in the same order, whatever the capacity: the products went out where the loop stands
    assert calls[0] == calls[2] and calls[1] == calls[2] and len(calls[2]) >= 3 * cfg['n_layers']
