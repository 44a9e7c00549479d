"""The whole-tile weight gradient that also sums the output-bias gradient's columns (m3p_gemm_wgrad_bias_bf16: the BIAS
instantiation of gemm_wgrad_w4_kernel) and MLMHeadFn on top of it.

The kernel sums bsum[v] = sum_n w[n] e[n, v] from the fragments its K loop holds, with the weights rounded to bf16.  It is
held, element by element, to the bound tests/test_mlm_shifted_gpu.py derives for the bias gradient (_distances: n addends
gathered in any order, each rounded to bf16 once - here the rounding is the weight's) against the fp64 product of the same
operands; the weights span six decades across the rows, so a weight representation that is too short for the small ones (a
fixed-point one, a flushed denormal) shows.  The product itself must not notice:
dE is compared bit for bit with the existing entry points' on the same operands, stored and accumulated.

The whole-tile schedule needs more output tiles than workgroups: the persistent grid is narrowed (tests.util.gemm_schedule, as
in tests/test_gemm_schedules.py) so that 20 row tiles make every workgroup take more than one tile and the last round a partial
one; n = 4096 is the smallest row count of the dispatch band (64 K-tiles)."""
import pytest
import torch

from m3p_amd import functional as F
from m3p_amd import lib as L
from m3p_amd import ops
from tests import test_mlm_shifted_gpu as TSH
from tests.util import BF16_OUT, KAPPA, U32, accum_bound, assert_exact_zero, gemm_schedule

pytestmark = pytest.mark.gpu

N_ROWS, V_PAD, V = 4096, 20 * 256, 20 * 256 - 110
GRID = {256: 8, 768: 32, 1024: 32}          # 20 / 60 / 80 tiles: rounds of 8 + 8 + 4, 32 + 28, 32 + 32 + 16
GUARD = 64
_OPERANDS = {}


def _operands():
    """e (positive, a few decades wide, exact-zero pad columns), the weights and the fp64 sums: made once, never written."""
    if not _OPERANDS:
        g = torch.Generator().manual_seed(23)
        e = torch.exp(2.0 * torch.randn((N_ROWS, V_PAD), generator=g) - 3.0).to(torch.bfloat16)
        e[:, V:] = 0
        w = 10.0 ** (-6.0 * torch.rand((N_ROWS,), generator=g))              # 1e-6 .. 1 across the rows
        w[0], w[1] = 1.0, 1e-6
        ref = e.double().t() @ w.double()
        _OPERANDS.update(e=e.cuda(), w=w.cuda(), ref=ref, absref=ref.clone(), hs={})         # (positive terms: their own absolute sum)
    return _OPERANDS


def _hs(d):
    c = _operands()
    if d not in c['hs']:
        g = torch.Generator().manual_seed(100 + d)
        c['hs'][d] = (torch.randn((N_ROWS, d), generator=g) * 0.05).to(torch.bfloat16).cuda()
    return c['hs'][d]


def _guarded_bsum():
    buf = torch.full((GUARD + V_PAD + GUARD,), 12345.0, dtype=torch.float32, device='cuda')
    buf[GUARD:GUARD + V_PAD] = float('nan')
    return buf, buf[GUARD:GUARD + V_PAD]


@pytest.mark.parametrize('store', [True, False], ids=['store', 'accumulate'])
@pytest.mark.parametrize('d', [768, 256, 1024])
def test_bias_sums_beside_a_bit_identical_product(d, store):
    c = _operands()
    e, w, hs = c['e'], c['w'], _hs(d)
    g = torch.Generator().manual_seed(7)
    dw0 = torch.randn((V_PAD, d), generator=g).cuda() if not store else torch.zeros((V_PAD, d), device='cuda')
    with gemm_schedule(grid=GRID[d]):
        assert L.load().m3p_gemm_wgrad_plan(N_ROWS, V_PAD, d) == L.KERN_WGRAD_W4_TILES
        want = dw0.clone()
        stored = ops.gemm_wgrad(e, hs, want, n=V_PAD, k=d, dw_is_zero=store, report_store=True)
        assert stored == store
        got = dw0.clone() if not store else torch.full((V_PAD, d), float('nan'), device='cuda')
        buf, bsum = _guarded_bsum()
        assert ops.gemm_wgrad_bias(e, hs, got, w, bsum, n=V_PAD, k=d, store=store)
        torch.cuda.synchronize()
    assert torch.equal(got, want), 'dE differs from the launch without the bias sums'
    assert bool((buf[:GUARD] == 12345.0).all()) and bool((buf[GUARD + V_PAD:] == 12345.0).all()), 'guard words overwritten'
    assert not bool(torch.isnan(bsum).any()), 'entries of bsum left unwritten'
    assert_exact_zero(bsum[V:], 'bsum of the pad columns')
    worst, at = accum_bound(bsum.cpu(), c['ref'], c['absref'], N_ROWS, BF16_OUT * c['absref'])
    print('d = %d, %s: bsum reaches %.3g x its bound (column %s); largest relative error %.3g' % (
        d, 'store' if store else 'accumulate', worst, at, float(((bsum.cpu().double() - c['ref']).abs()[:V] / c['ref'][:V]).max())))
    assert worst <= 1.0


def test_declines_without_writing():
    c = _operands()
    e, w, hs = c['e'], c['w'], _hs(768)
    dw = torch.full((V_PAD, 768), float('nan'), device='cuda')
    buf, bsum = _guarded_bsum()
    # fewer tiles than workgroups: the full grid gives every tile a workgroup of its own and splits M instead
    if 60 <= L.num_cus():
        assert L.load().m3p_gemm_wgrad_plan(N_ROWS, V_PAD, 768) != L.KERN_WGRAD_W4_TILES
        assert not ops.gemm_wgrad_bias(e, hs, dw, w, bsum, n=V_PAD, k=768, store=True)
    with gemm_schedule(grid=32):
        # first operand off the 16-byte boundary its transfers need
        flat = torch.zeros((N_ROWS * V_PAD + 8,), dtype=torch.bfloat16, device='cuda')
        e_off = flat[1:1 + N_ROWS * V_PAD].view(N_ROWS, V_PAD)
        assert not ops.gemm_wgrad_bias(e_off, hs, dw, w, bsum, n=V_PAD, k=768, store=True)
        # more rows than the weights' part of the LDS holds is not tried here: 8256 rows of operands for one return code
        torch.cuda.synchronize()
    assert bool(torch.isnan(dw).all()) and bool(torch.isnan(bsum).all()) and bool((buf[:GUARD] == 12345.0).all())


@pytest.fixture(scope='module')
def head():
    return TSH._Head()                       # d = 256, V = 5000 -> V_pad = 5120, 4096 predicted rows


def _spy(mp, counts):
    real_wgrad, real_colsum = ops.gemm_wgrad, ops.ce_shift_colsum

    def wgrad(*a, **k):
        res = real_wgrad(*a, **k)
        if k.get('bias') is not None:
            counts['bias'] += int(res[1])              # (result, whether the launch wrote the sums)
        return res

    def colsum(*a, **k):
        counts['colsum'] += 1
        return real_colsum(*a, **k)

    mp.setattr(ops, 'gemm_wgrad', wgrad)
    mp.setattr(ops, 'ce_shift_colsum', colsum)


def test_mlm_head_takes_the_bias_gradient_from_the_weight_gradient(head):
    """Forward skips the column-sum pass, backward gets the sums from the launch; against the same call with the skip off, and
    with the entry that hands the launch its operands made to decline (backward then runs the pass itself): the bias gradient within its bound, all else equal."""
    ref = head.reference('plain', head.H, head.y)
    runs = {}
    with gemm_schedule(grid=8):
        assert L.load().m3p_gemm_wgrad_plan(head.n, V_PAD, head.d) == L.KERN_WGRAD_W4_TILES
        for what in ('new', 'pass in forward', 'declined'):
            counts = {'bias': 0, 'colsum': 0}
            with pytest.MonkeyPatch.context() as mp:
                _spy(mp, counts)
                if what == 'pass in forward':
                    mp.setattr(F, '_VOCAB_WGRAD_BIAS', False)
                if what == 'declined':
                    mp.setattr(L.load(), 'm3p_gemm_wgrad_bias_arm', lambda *a: -2)
                runs[what] = head.run(head.H, head.y, False)
            assert (counts['bias'], counts['colsum']) == {'new': (1, 0), 'pass in forward': (0, 1), 'declined': (0, 1)}[what], (what, counts)
    for what, got in runs.items():
        dist = TSH._distances(head, got, ref)
        print('%-16s distance / bound: %s' % (what, ', '.join('%s %.3g' % kv for kv in sorted(dist.items()))))
        for k, v in dist.items():
            assert v <= 1.0, (what, k, v)
    # bit for bit, but for the words that are the target of several rows: their rows of dE and entries of db also gather those
    # rows' terms with fp32 atomics, in an order that differs from run to run (held to the bounds above)
    once = (torch.bincount(head.y, minlength=head.V) <= 1)
    base = runs['pass in forward']
    for what in ('new', 'declined'):
        loss, dH, dE, db = runs[what]
        assert loss == base[0] and torch.equal(dH, base[1]) and torch.equal(dE[once], base[2][once]), what
    # (the bias gradient of the declined launch comes from the same pass, run one call later: its partial sums are folded in an
    #  order of their own, so twice the accumulation term of the bound)
    err = (runs['declined'][3].double() - base[3].double()).abs().cpu()
    assert bool((err <= 2 * KAPPA * head.n ** 0.5 * U32 * ref['adb'].cpu() + 1e-300).all())
