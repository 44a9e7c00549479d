"""LayerNorm forward and backward on every launch path of csrc/layernorm.hip (GPU): the grid-stride loops of the three
kernels, every NI instantiation with a partly filled last chunk, the half-wave backward with 16-byte accesses and with the
8-byte ones it takes when a pointer is only 8-byte aligned, the dropout branch of both, and the entry points' refusals.

The convention of tests/test_stream_kernels.py: the launchers' caps are copied below beside the line they come from, and each
case asserts the premise that puts it on the path it names before the kernel runs, so a later change of a cap makes the test
say that it no longer covers the loop.  y and dx are held row by row, mean and rstd element by element, as in
tests/test_layernorm.py; dgamma, dbeta and dbias_drop column by column with the accumulation bound of tests/util.py
(ln_colsum_bounds, ln_dbias_bound), shown on the CPU in tests/test_parity_bounds.py to accept the fp32 restatement of the
kernels and to reject a lost term, a misplaced column and the rows of a lost second trip."""
import numpy as np
import pytest
import torch

from tests import util as U
from tests.util import (F32_OUT, ROW_FLOOR, ROW_RTOL_BF16, assert_bits_equal, assert_exact_zero, block_bound, gemm_bound,
                        poisoned_outputs, randn_bf16, randn_f32)

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16

# --- the launchers' rules (m3p_amd/csrc/layernorm.hip) ---------------------------------------------------------------------
LN_ROWS_PER_BLOCK = 4             # ln_fwd_kernel / ln_bwd_kernel: one wave per row, __launch_bounds__(256)
LN_FWD_MAXBLK = 4096              # m3p_layernorm_fwd: blocks = min((rows + 3) / 4, 4096)
LN_BWD_MAXBLK = 512               # m3p_layernorm_bwd_rows: blocks = min((rows + 3) / 4, 512)
LN_BWD_BLOCKS = 512               # LN_BWD_BLOCKS: blocks_hw = min((rows + 7) / 8, LN_BWD_BLOCKS)
LN_HW_ROWS_PER_BLOCK = 8          # ln_bwd_hw_kernel: half a wave per row, 8 half-waves per block
LN_HW_WIDTHS = (768, 1024)        # m3p_layernorm_bwd_rows: d == 768 || d == 1024; 16-byte accesses if every bf16 pointer is 16-byte aligned
LN_MAX_D = 2048                   # both entry points: d % 4 == 0 && d <= 2048
M3P_EINVAL = -1                   # include/m3p_hip.h

WORST = {}                        # kernel, path and quantity -> the largest normalised error seen


def _note(kernel, what, worst):
    key = '%-28s %s' % (kernel, what)
    WORST[key] = max(WORST.get(key, 0.0), float(worst))


def ln_ni(d):
    """layernorm.hip ln_ni and the switches on it: NI = ceil(d / 256), and 8 for everything above 4."""
    ni = (d + 255) // 256
    return ni if ni <= 4 else 8


def fwd_kernel(rows, d):
    return 'ln_fwd_kernel<%d>%s' % (ln_ni(d), ' loop' if rows > LN_FWD_MAXBLK * LN_ROWS_PER_BLOCK else '')


def bwd_kernel(rows, d, *ptrs):
    """The kernel m3p_layernorm_bwd_rows launches for these x, dy_a, dx, dy_b, dx_drop (None = a null pointer)."""
    if d in LN_HW_WIDTHS:
        a16 = all(t is None or t.data_ptr() % 16 == 0 for t in ptrs)
        return 'ln_bwd_hw_kernel<%d%s>%s' % (d // 256, '' if a16 else ', 8-byte', ' loop' if rows > LN_BWD_BLOCKS * LN_HW_ROWS_PER_BLOCK else '')
    return 'ln_bwd_kernel<%d>%s' % (ln_ni(d), ' loop' if rows > LN_BWD_MAXBLK * LN_ROWS_PER_BLOCK else '')


def _at8(t):
    """A copy of t at an address that is 8 but not 16 bytes aligned: carved out of a larger buffer at an element offset of 4."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    buf.view(torch.int16).fill_(-1)
    v = buf[4:4 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 8 and v.is_contiguous()
    return v


def _inputs(rows, d, masked, misalign=()):
    x, _ = randn_bf16((rows, d), 1, 2.0)
    dya, _ = randn_bf16((rows, d), 5)
    dyb, _ = randn_bf16((rows, d), 6)
    g, _ = randn_f32((d,), 2, 0.5)
    g += 1.0
    b, _ = randn_f32((d,), 3, 0.5)
    rm = None
    if masked:
        rm = torch.from_numpy((np.random.RandomState(4).rand(rows) > 0.3).astype(np.uint8)).cuda()
    t = {'x': x, 'dy_a': dya, 'dy_b': dyb}
    for name in misalign:
        if name in t:
            t[name] = _at8(t[name])
    return t['x'], t['dy_a'], t['dy_b'], g, b, rm


class _Ref:
    """fp64 on the device from the kernel's own bf16 / fp32 inputs."""

    def __init__(self, x, g, b, rm):
        self.x, self.g, self.b = x.double(), g.double(), b.double()
        self.mu = self.x.mean(-1)
        self.rs = 1.0 / torch.sqrt((self.x - self.mu[:, None]).pow(2).mean(-1) + 1e-12)
        self.xhat = (self.x - self.mu[:, None]) * self.rs[:, None]
        self.keep = torch.ones(x.shape[0], 1, dtype=torch.float64, device=x.device) if rm is None else rm.double()[:, None]
        self.off = None if rm is None else rm == 0

    def check_fwd(self, kernel, y, mean, rstd):
        d = self.x.shape[1]
        w, at, _ = block_bound(y, (self.xhat * self.g + self.b) * self.keep, ('row',), ROW_RTOL_BF16, ROW_FLOOR)
        assert w <= ROW_RTOL_BF16, '%s y: row %s has relative error %.3g > %.3g' % (kernel, at, w, ROW_RTOL_BF16)
        _note(kernel, 'y / ROW_RTOL_BF16', w / ROW_RTOL_BF16)
        for name, got, ref, absref in (('mean', mean, self.mu, self.x.abs().mean(-1)), ('rstd', rstd, self.rs, self.rs)):
            w, at = gemm_bound(got, ref, absref, d, F32_OUT)
            assert w <= 1.0, '%s %s: the error reaches %.3g x the elementwise bound at row %d' % (kernel, name, w, at['row'])
            _note(kernel, name, w)
        if self.off is not None:
            assert_exact_zero(y[self.off], kernel + ' y of masked rows')

    def check_bwd(self, kernel, dya, dyb, dx, dg, db):
        dy = dya.double() if dyb is None else dya.double() + dyb.double()
        gdy = dy * self.g
        dx64 = self.rs[:, None] * (gdy - gdy.mean(-1, keepdim=True) - self.xhat * (gdy * self.xhat).mean(-1, keepdim=True)) * self.keep
        w, at, _ = block_bound(dx, dx64, ('row',), ROW_RTOL_BF16, ROW_FLOOR)
        assert w <= ROW_RTOL_BF16, '%s dx: row %s has relative error %.3g > %.3g' % (kernel, at, w, ROW_RTOL_BF16)
        _note(kernel, 'dx / ROW_RTOL_BF16', w / ROW_RTOL_BF16)
        if self.off is not None:
            assert_exact_zero(dx[self.off], kernel + ' dx of masked rows')
        (wg, ag), (wb, ab) = U.ln_colsum_bounds(dg, db, dy * self.keep, self.x, self.mu, self.rs)
        print('%s [%d x %d]: dgamma %.3g, dbeta %.3g of the column bound' % ((kernel,) + tuple(self.x.shape) + (wg, wb)))
        assert wg <= 1.0, '%s dgamma: the error reaches %.3g x the accumulation bound at column %d' % (kernel, wg, ag['row'])
        assert wb <= 1.0, '%s dbeta: the error reaches %.3g x the accumulation bound at column %d' % (kernel, wb, ab['row'])
        _note(kernel, 'dgamma', wg)
        _note(kernel, 'dbeta', wb)

    def check_dbias(self, kernel, dbias, stored):
        w, at = U.ln_dbias_bound(dbias, stored)
        assert w <= 1.0, '%s dbias_drop: the error reaches %.3g x the accumulation bound at column %d' % (kernel, w, at['row'])
        _note(kernel, 'dbias_drop', w)


def _bwd(x, dya, dyb, g, mean, rstd, rm, dbias=True, dx_at8=False, **kw):
    """ops.layernorm_bwd on poisoned outputs and zeroed column sums -> dx, dx_drop, dgamma, dbeta, dbias_drop.  dx_at8: the
    library entry point itself with a poisoned dx at an 8-mod-16 address (ops.layernorm_bwd allocates dx itself), and the
    elements before and behind it untouched."""
    from m3p_amd import ops, lib as L
    rows, d = x.shape
    dg, db = torch.zeros(d, device='cuda'), torch.zeros(d, device='cuda')
    dbt = torch.zeros(d, device='cuda') if dbias else None
    if not dx_at8:
        with poisoned_outputs():
            dx, dxd = ops.layernorm_bwd(dya, dyb, x, g, mean, rstd, rm, dg, db, dbias_drop=dbt, **kw)
        return dx, dxd, dg, db, dbt
    assert not kw
    buf = torch.empty(rows * d + 8, dtype=BF16, device='cuda')
    buf.view(torch.int16).fill_(-1)
    dx = buf[4:4 + rows * d].view(rows, d)
    assert dx.data_ptr() % 16 == 8
    rc = L.load().m3p_layernorm_bwd_rows(dya.data_ptr(), L.ptr(dyb), x.data_ptr(), g.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                         L.ptr(rm), dx.data_ptr(), None, dg.data_ptr(), db.data_ptr(), L.ptr(dbt), rows, d, 0, 0,
                                         1.0, None, L.stream())
    L.check(rc, 'm3p_layernorm_bwd_rows')
    edge = torch.cat((buf[:4], buf[-4:])).view(torch.int16)
    assert bool((edge == -1).all()), 'the elements around an 8-mod-16 dx were written'
    return dx, None, dg, db, dbt


def _fwd_bwd(rows, d, masked, misalign=(), dx_at8=False):
    """Forward, then backward with dy_a + dy_b and dbias_drop (no dropout), all checked -> (kernel that ran backward, dx)."""
    from m3p_amd import ops
    x, dya, dyb, g, b, rm = _inputs(rows, d, masked, misalign)
    with poisoned_outputs():
        y, mean, rstd = ops.layernorm_fwd(x, g, b, rm)
    ref = _Ref(x, g, b, rm)
    ref.check_fwd(fwd_kernel(rows, d), y, mean, rstd)
    dx, dxd, dg, db, dbias = _bwd(x, dya, dyb, g, mean, rstd, rm, dx_at8=dx_at8)
    assert dxd is None
    kernel = bwd_kernel(rows, d, x, dya, dx, dyb, None)
    ref.check_bwd(kernel, dya, dyb, dx, dg, db)
    ref.check_dbias(kernel, dbias, dx)                   # no dropout: the column sums of the bf16 dx it wrote
    return kernel, dx


# (path, rows, d, the kernels it must run forward and backward)
PATHS = [
    ('forward loop', 16390, 128, 'ln_fwd_kernel<1> loop', 'ln_bwd_kernel<1> loop'),
    ('generic backward loop, full chunks', 2051, 128, 'ln_fwd_kernel<1>', 'ln_bwd_kernel<1> loop'),
    ('generic backward loop, ragged NI = 1', 2051, 36, 'ln_fwd_kernel<1>', 'ln_bwd_kernel<1> loop'),
    ('generic backward loop, ragged NI = 2', 2051, 260, 'ln_fwd_kernel<2>', 'ln_bwd_kernel<2> loop'),
    ('generic backward loop, ragged NI = 3', 2051, 516, 'ln_fwd_kernel<3>', 'ln_bwd_kernel<3> loop'),
    ('generic backward loop, ragged NI = 4', 2051, 772, 'ln_fwd_kernel<4>', 'ln_bwd_kernel<4> loop'),
    ('NI = 8 below 2048', 70, 1028, 'ln_fwd_kernel<8>', 'ln_bwd_kernel<8>'),
    ('NI = 8 below 2048', 70, 1540, 'ln_fwd_kernel<8>', 'ln_bwd_kernel<8>'),
    ('NI = 8 below 2048, backward loop', 2051, 1284, 'ln_fwd_kernel<8>', 'ln_bwd_kernel<8> loop'),
    ('half-wave loop', 4101, 768, 'ln_fwd_kernel<3>', 'ln_bwd_hw_kernel<3> loop'),
    ('half-wave loop', 4101, 1024, 'ln_fwd_kernel<4>', 'ln_bwd_hw_kernel<4> loop'),
    ('fewer rows than a block', 1, 768, 'ln_fwd_kernel<3>', 'ln_bwd_hw_kernel<3>'),
    ('fewer rows than a block', 7, 768, 'ln_fwd_kernel<3>', 'ln_bwd_hw_kernel<3>'),
    ('an odd row count over two blocks', 9, 1024, 'ln_fwd_kernel<4>', 'ln_bwd_hw_kernel<4>'),
    ('one chunk in one lane', 3, 4, 'ln_fwd_kernel<1>', 'ln_bwd_kernel<1>'),
]


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('path,rows,d,fwd,bwd', PATHS, ids=['%dx%d' % (p[1], p[2]) for p in PATHS])
def test_layernorm_paths(path, rows, d, fwd, bwd, masked):
    # the premises, from the launchers' rules
    assert fwd_kernel(rows, d) == fwd, (path, fwd_kernel(rows, d))
    if path == 'forward loop':
        assert rows > LN_FWD_MAXBLK * LN_ROWS_PER_BLOCK
    if 'backward loop' in path:
        assert rows > LN_BWD_MAXBLK * LN_ROWS_PER_BLOCK and d not in LN_HW_WIDTHS
    if 'ragged' in path:
        assert d % 256 != 0 and (d + 255) // 256 == ln_ni(d)
    if 'NI = 8' in path:
        assert (d + 255) // 256 >= 5 and d < LN_MAX_D and ln_ni(d) == 8
    if path == 'half-wave loop':
        assert rows > LN_BWD_BLOCKS * LN_HW_ROWS_PER_BLOCK and d in LN_HW_WIDTHS
    kernel, _ = _fwd_bwd(rows, d, masked)
    assert kernel == bwd, (path, kernel)         # (the half-wave kernel: every pointer 16-byte aligned, dx included)


@pytest.mark.parametrize('which', ['x', 'dy_a', 'dy_b', 'dx'])
@pytest.mark.parametrize('d', LN_HW_WIDTHS)
def test_layernorm_bwd_alignment_fallback(d, which):
    """d = 768 / 1024 with one of x, dy_a, dy_b, dx at an 8-mod-16 address (the premise: data_ptr() % 16 == 8 of that one
    pointer, asserted where it is carved out) takes the 8-byte form of the half-wave kernel, ln_bwd_hw_kernel<NC, false>.  Every
    output passes the fp64 bounds, and dx equals the aligned launch's bit for bit: the arithmetic is the same kernel's, only
    the width of the memory accesses differs.  (ln_bwd_kernel<3 / 4>, which served these calls before, adds the row sums c1 and
    c2 in another order - a lane's four elements pairwise and 64 lanes, against eight elements one after the other and 32
    lanes - and its dx differed from the half-wave kernel's by one bf16 step in 8 of 230400 elements at d = 768 and 3 of 307200
    at d = 1024: what a call computed depended on where the allocator had put its tensors.)"""
    rows = 300
    k_hw, dx_hw = _fwd_bwd(rows, d, False)
    assert k_hw == 'ln_bwd_hw_kernel<%d>' % (d // 256)
    k_fb, dx_fb = _fwd_bwd(rows, d, False, misalign=(which,), dx_at8=which == 'dx')
    assert k_fb == 'ln_bwd_hw_kernel<%d, 8-byte>' % (d // 256), (which, k_fb)
    assert_bits_equal(dx_fb.contiguous(), dx_hw, 'dx behind an 8-mod-16 %s against the aligned launch (d = %d)' % (which, d))


# (rows, d, dy_b and a row mask, dx_drop wanted, rows of the full tensor for rng_rows or 0[, the input at 8 mod 16])
DROP = [
    (2051, 128, False, True, 0), (2051, 260, False, True, 0), (4101, 768, False, True, 0),      # generic <1>, <2> ragged, half-wave: loops
    (2051, 128, True, True, 0), (4101, 768, True, True, 0), (2051, 260, True, True, 0),           # with dy_b and a row mask
    (2051, 128, False, False, 0), (4101, 768, True, False, 0),                                    # dbias_drop alone: dx_drop == nullptr
    (300, 128, False, True, 1000), (300, 768, True, True, 1000), (2051, 128, True, False, 5000),  # rng_rows
    (4101, 768, True, True, 0, 'dy_b'), (300, 1024, False, True, 0, 'x'),                         # the half-wave kernel's 8-byte form
]


@pytest.mark.parametrize('case', DROP, ids=['-'.join(str(v) for v in c) for c in DROP])
def test_layernorm_bwd_dropout_paths(case):
    """The dropout branch (p = 0.1) against the host twin of the device RNG: dx_drop = bf16(dx keep / (1 - p)) of the dx the
    kernel stored, dbias_drop = the column sums of those bf16 values whether they are stored or not; the keep element of
    (r, c) is r d + c, or rng_rows[r] d + c."""
    from m3p_amd import ops, rng
    (rows, d, both, want_drop, full), at8 = case[:5], case[5:]
    p, seed = 0.1, 12345
    x, dya, dyb, g, b, rm = _inputs(rows, d, both, misalign=at8)
    if not both:
        dyb = None
    y, mean, rstd = ops.layernorm_fwd(x, g, b, rm)
    rr = None
    if full:
        pick = np.sort(np.random.RandomState(8).choice(full, size=rows, replace=False))      # a subset, in increasing order
        assert (np.diff(pick) > 0).all() and pick[-1] > rows
        rr = torch.from_numpy(pick.astype(np.int32)).cuda()
    dx, dxd, dg, db, dbias = _bwd(x, dya, dyb, g, mean, rstd, rm, want_drop=want_drop, seed=seed, p_drop=p, rng_rows=rr)
    kernel = bwd_kernel(rows, d, x, dya, dx, dyb, dxd)
    if d in LN_HW_WIDTHS:
        assert kernel.startswith('ln_bwd_hw_kernel') and ('8-byte' in kernel) == bool(at8), kernel
    if rows > 2048:
        assert kernel.endswith(' loop'), kernel
    assert (dxd is not None) == want_drop
    kernel += ' drop'
    ref = _Ref(x, g, b, rm)
    ref.check_bwd(kernel, dya, dyb, dx, dg, db)
    keep = rng.keep_mask((full or rows) * d, seed, p, (full or rows, d))
    keep = torch.from_numpy(keep[pick] if full else keep)
    assert abs(float(keep.float().mean()) - (1 - p)) < 5e-3
    exp = (dx.float().cpu() * keep / (1 - p)).to(BF16)
    if want_drop:
        assert torch.equal(dxd.cpu(), exp), '%s dx_drop: %d elements differ' % (kernel, int((dxd.cpu() != exp).sum()))
        if ref.off is not None:
            assert_exact_zero(dxd[ref.off], kernel + ' dx_drop of masked rows')
    ref.check_dbias(kernel, dbias, dxd if want_drop else exp.cuda())


def test_layernorm_entry_points_refuse_bad_shapes_and_pointers():
    """M3P_EINVAL and nothing launched: d % 4 != 0, d > 2048, rows = 0, a pointer that is 4 but not 8 bytes aligned."""
    from m3p_amd import lib as L
    lib = L.load()
    rows, d = 8, 2048 + 8
    n = rows * d
    poison = lambda *s, dt=BF16: torch.full(s, float('nan'), dtype=dt, device='cuda')      # noqa: E731
    x, _ = randn_bf16((n + 8,), 1)
    dy, _ = randn_bf16((n + 8,), 2)
    g, b = torch.ones(d, device='cuda'), torch.zeros(d, device='cuda')
    mean, rstd = torch.zeros(rows, device='cuda'), torch.ones(rows, device='cuda')
    y, dx = poison(n + 8), poison(n + 8)
    st, dg, db = poison(2 * rows, dt=torch.float32), poison(d, dt=torch.float32), poison(d, dt=torch.float32)
    assert x[2:].data_ptr() % 8 == 4

    def fwd(r, dd, xin=x, out=y):
        return lib.m3p_layernorm_fwd(xin.data_ptr(), g.data_ptr(), b.data_ptr(), None, out.data_ptr(), st.data_ptr(),
                                     st[rows:].data_ptr(), r, dd, 1e-12, L.stream())

    def bwd(r, dd, xin=x, dyin=dy, out=dx):
        return lib.m3p_layernorm_bwd_rows(dyin.data_ptr(), None, xin.data_ptr(), g.data_ptr(), mean.data_ptr(), rstd.data_ptr(), None,
                                          out.data_ptr(), None, dg.data_ptr(), db.data_ptr(), None, r, dd, 0, 0, 1.0, None, L.stream())

    for what, r, dd in (('d % 4 != 0', rows, 770), ('d % 4 != 0', rows, 6), ('d > 2048', rows, LN_MAX_D + 4), ('rows = 0', 0, 768),
                        ('rows < 0', -1, 768), ('d = 0', rows, 0)):
        assert fwd(r, dd) == M3P_EINVAL, 'm3p_layernorm_fwd: ' + what
        assert bwd(r, dd) == M3P_EINVAL, 'm3p_layernorm_bwd_rows: ' + what
    assert fwd(rows, 768, xin=x[2:]) == M3P_EINVAL and fwd(rows, 768, out=y[2:]) == M3P_EINVAL
    assert bwd(rows, 768, xin=x[2:]) == M3P_EINVAL and bwd(rows, 768, dyin=dy[2:]) == M3P_EINVAL and bwd(rows, 768, out=dx[2:]) == M3P_EINVAL
    torch.cuda.synchronize()
    for t in (y, dx, st, dg, db):
        assert bool(torch.isnan(t).all()), 'a refused call wrote an output'
    assert fwd(rows, 768) == 0 and bwd(rows, 768) == 0             # the same buffers are taken once the arguments are right
    torch.cuda.synchronize()
    assert not bool(torch.isnan(y[:rows * 768]).any()) and not bool(torch.isnan(dx[:rows * 768]).any())


def test_zz_report_layernorm_paths():
    """Not a check: the largest normalised error (1 = the bound) each kernel and path reached in this module's tests."""
    for key in sorted(WORST):
        print('layernorm  %s  %.3g' % (key, WORST[key]))
