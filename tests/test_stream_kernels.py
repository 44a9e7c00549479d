"""The streaming and glue kernels (optimizer, sum of squares, GELU passes, 8-bit quantisation, casts, gathers and scatters,
embedding assembly) at the sizes where their grid-stride loops and batch splits run, against fp64 references (GPU).

Almost every one of these launchers caps its grid and walks the rest in a loop, or changes its work split with the batch
size.  Each test derives its sizes from the launcher's rule - constants copied below beside the line they come from - and
asserts the premise that puts it on the path it names, so a later change of a cap makes the test say that it no longer
covers the loop.  The bounds are those of tests/util.py, shown on the CPU in tests/test_parity_bounds.py to accept an fp32
restatement of each kernel and to reject single wrong quads and rows."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import util as U
from tests.util import (BF16_OUT, EMBED_DE_RTOL, EPS_DGELU, EPS_ERF, ROW_FLOOR, ROW_RTOL_BF16, _dgelu64, _gelu64, assert_accum_bound,
                        assert_adam_bound, assert_bits_equal, assert_block_bound, assert_exact_zero, assert_gemm_bound,
                        assert_sumsq_bound, poisoned_outputs)

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16

# --- the launchers' grid rules (m3p_amd/csrc) ---------------------------------------------------------------------------
THREADS = 256                     # every kernel here: __launch_bounds__(256)
ADAM_MAXBLK = 4096                # optim.hip m3p_adam_step: blocks = min(ceil(n4 / 256), 4096); ADAM_MAXBLK of the ranged form
ADAM_Q = 2                        # optim.hip adam_kernel / ADAM_Q: quads per thread and trip
ADAM_MAX_RANGES = 32              # optim.hip ADAM_MAX_RANGES: pieces per launch
SUMSQ_MAXBLK = 2048               # optim.hip m3p_sumsq_f32: blocks = clamp(ceil(n4 / 1024), 1, 2048)
SUMSQ_QUADS_PER_BLOCK = 1024
SUMSQ_UNROLL = 4                  # optim.hip sumsq_kernel: four quads per thread and trip of the unrolled loop
SUMSQ_MAX_RANGES = 32             # optim.hip SUMSQ_MAX_RANGES
GELU_MAXBLK = 8192                # optim.hip m3p_gelu_fwd / m3p_gelu_bwd / m3p_gelu_fwd_q8: 8 elements per thread and trip
QUANT_MAXBLK = 4096               # optim.hip m3p_quant_fp8: 8 elements per thread and trip
CAST_MAXBLK = 4096                # embed.hip m3p_cast_f32_bf16: 4 elements per thread and trip
ROWS_MAXBLK = 2048                # heads.hip m3p_gather_rows / m3p_scatter_add_rows: 4 elements per thread and trip
TOKROWS_MAXBLK = 4096             # heads.hip m3p_scatter_add_token_rows: 4 rows (waves) per block
EMBED_FWD_MAXBLK = 4096           # embed.hip launch_embed_fwd: 4 rows (waves) per block
EMB_BWD_BLOCKS = 512              # embed.hip EMB_BWD_BLOCKS

ADAM_FULL = ADAM_MAXBLK * THREADS                   # quads one trip of the full grid covers with its first quad
SUMSQ_FULL = SUMSQ_MAXBLK * THREADS * SUMSQ_UNROLL  # quads one trip of the full grid's unrolled loop covers
GUARD = 1024                                        # floats of guard band before and after an updated range

WORST = {}                        # kernel -> the largest normalised error seen, printed by the last test of the module


def _note(name, worst):
    WORST[name] = max(WORST.get(name, 0.0), float(worst))


def _gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


# =====================================================================================================================
# Adam
# =====================================================================================================================
def _adam_arena(n, seed):
    """p, g, m, v (fp32) and w16 (bf16) of n floats: gradient scales 1e-4 .. 30, second moments 1e-10 .. 1 (log-uniform per
    element), zero g / m / v entries."""
    gen = _gen(seed)
    gscale = torch.pow(10.0, torch.empty(n, device='cuda').uniform_(-4.0, math.log10(30.0), generator=gen))
    p = torch.randn(n, device='cuda', generator=gen)
    g = gscale * torch.randn(n, device='cuda', generator=gen)
    m = 0.5 * gscale * torch.randn(n, device='cuda', generator=gen)
    v = torch.pow(10.0, torch.empty(n, device='cuda').uniform_(-10.0, 0.0, generator=gen))
    del gscale
    for k, t in enumerate((g, m, v)):
        t[torch.randint(0, n, (max(n // 64, 1),), device='cuda', generator=gen)] = 0
    w16 = torch.randn(n, device='cuda', generator=gen).to(BF16)
    return p, g, m, v, w16


def _hp(step=3, wd=0.01, max_norm=0.0, grad_scale=1.0, gnorm_sq=None, step_size=None):
    lr, b1, b2 = 1e-2, 0.9, 0.98
    return dict(lr=lr, beta1=b1, beta2=b2, eps=1e-8, weight_decay=wd, max_norm=max_norm, grad_scale=grad_scale, gnorm_sq=gnorm_sq,
                step_size=lr * math.sqrt(1 - b2 ** step) / (1 - b1 ** step) if step_size is None else step_size)


def _check_adam_piece(after, before, a, b, hp, zero, what):
    """Elements [a, b) of the arenas after one update with hp: the bound on p, m, v; w16 = bf16(p) bitwise; g zeroed or
    bit-identical.  Then the piece is put back as it was, so the caller can compare whole arenas for everything else."""
    (p, g, m, v, w16), (p0, g0, m0, v0, w0) = after, before
    worst = assert_adam_bound((p[a:b], m[a:b], v[a:b]), (p0[a:b], g0[a:b], m0[a:b], v0[a:b]), hp, what=what, start=a)
    if w16 is not None:
        assert_bits_equal(w16[a:b], p[a:b].to(BF16), what + ': bf16 copy')
        w16[a:b] = w0[a:b]
    if zero:
        assert_bits_equal(g[a:b], torch.zeros_like(g[a:b]), what + ': zeroed gradient')      # (+0, not -0)
        g[a:b] = g0[a:b]
    for t, t0 in ((p, p0), (m, m0), (v, v0)):
        t[a:b] = t0[a:b]
    return worst


def _check_untouched(after, before, what):
    for name, t, t0 in zip(('p', 'g', 'm', 'v', 'w16'), after, before):
        if t is not None:
            assert_bits_equal(t, t0, '%s: %s outside the updated ranges' % (what, name))


ADAM_SIZES = [1, ADAM_FULL, ADAM_FULL + 1, 2 * ADAM_FULL + 77, 3 * ADAM_FULL + 77]      # quads


def _adam_plain(n4, variant, seed, steps=1):
    from m3p_amd import ops
    n = 4 * n4
    arena = _adam_arena(n + 2 * GUARD, seed)
    lo, hi = GUARD, GUARD + n
    gn = torch.zeros(1, dtype=torch.float64, device='cuda')
    for step in range(1, steps + 1):
        if step > 1:        # fresh gradients on moments that are no longer what the arena started with
            arena[1][lo:hi] = torch.randn(n, device='cuda', generator=_gen(seed + step)) * 0.3
        before = tuple(t.clone() for t in arena)
        gn.copy_((arena[1][lo:hi].double() ** 2).sum())
        norm = math.sqrt(float(gn))
        hp = _hp(step=step, wd=variant.get('wd', 0.01), grad_scale=variant.get('grad_scale', 1.0))
        clip = variant.get('clip', 'active')
        gs = hp['grad_scale'] or 1.0
        hp['max_norm'] = {'active': 0.5 * norm * gs, 'inactive': 2.0 * norm * gs, 'off': 0.0, 'no_norm': 0.5 * norm * gs}[clip]
        hp['gnorm_sq'] = None if clip == 'no_norm' else float(gn)       # (read from the device scalar the kernel is handed)
        if clip == 'active':
            assert math.sqrt(hp['gnorm_sq']) * gs > hp['max_norm'] > 0
        zero = variant.get('zero_grad', True)
        w16 = arena[4] if variant.get('w16', True) else None
        ops.adam_step(arena[0][lo:hi], arena[1][lo:hi], arena[2][lo:hi], arena[3][lo:hi], None if w16 is None else w16[lo:hi],
                      hp['lr'], hp['beta1'], hp['beta2'], hp['eps'], hp['weight_decay'], hp['step_size'],
                      gnorm_sq=None if clip == 'no_norm' else gn, max_norm=hp['max_norm'], grad_scale=hp['grad_scale'], zero_grad=zero)
        torch.cuda.synchronize()
        what = 'adam_step n4=%d %r step %d' % (n4, variant, step)
        after = arena[:4] + (w16,)
        result = [None if t is None else t.clone() for t in after]           # (the checks put the piece back as it was)
        worst = _check_adam_piece(after, before, lo, hi, hp, zero, what)
        for k, w in worst.items():
            _note('adam_kernel ' + k, w)
        _check_untouched(after, before, what)
        for t, r in zip(after, result):                                      # the next step goes on from what this one left
            if t is not None:
                t.copy_(r)
        if zero:
            assert_exact_zero(arena[1][lo:hi], what + ': gradient')


@pytest.mark.parametrize('n4', ADAM_SIZES)
def test_adam_step_sizes(n4):
    """One quad; the last size whose grid needs no loop; one quad more (block 0's thread 0 alone takes a second quad); a
    second trip in which only 77 threads have a first quad and none a second (``two`` false); a second trip with 77 second
    quads."""
    blocks = min(-(-n4 // THREADS), ADAM_MAXBLK)
    stride = blocks * THREADS
    if n4 > ADAM_FULL:
        assert blocks == ADAM_MAXBLK and n4 > stride                     # some thread takes a second quad
    if n4 > 2 * ADAM_FULL:
        assert n4 > ADAM_Q * stride and (n4 - ADAM_Q * stride) % stride == 77          # a second trip, ragged
    _adam_plain(n4, dict(clip='active', wd=0.01), seed=n4 % 997)


@pytest.mark.parametrize('variant', [
    dict(clip='inactive', wd=0.0), dict(clip='off', wd=0.01, zero_grad=False), dict(clip='no_norm', wd=0.0, w16=False),
    dict(clip='active', wd=0.0, grad_scale=0.5, zero_grad=False), dict(clip='active', wd=0.01, grad_scale=0.0),
    dict(clip='inactive', wd=0.01, grad_scale=0.5, w16=False)], ids=lambda v: '-'.join('%s=%s' % kv for kv in sorted(v.items())))
def test_adam_step_variants_at_the_largest_size(variant):
    n4 = ADAM_SIZES[-1]
    assert n4 > ADAM_Q * ADAM_MAXBLK * THREADS
    _adam_plain(n4, variant, seed=41)


def test_adam_step_three_steps_on_one_state():
    n4 = ADAM_SIZES[-2]
    assert n4 > ADAM_Q * ADAM_MAXBLK * THREADS
    _adam_plain(n4, dict(clip='active', wd=0.01), seed=43, steps=3)


def _adam_step_ranges_raw(arena, pieces, hp, gn):
    """m3p_adam_step_ranges with the pieces as given: ops.adam_step_ranges drops the empty ones before the launcher sees them,
    and the launcher's own handling of them is part of what is tested."""
    from m3p_amd import lib as L
    n = len(pieces)
    starts = (C.c_longlong * n)(*[int(a) for a, _, _, _ in pieces])
    counts = (C.c_longlong * n)(*[int(b - a) for a, b, _, _ in pieces])
    steps = (C.c_float * n)(*[float(st) for _, _, st, _ in pieces])
    zeros = (C.c_int * n)(*[int(bool(z)) for _, _, _, z in pieces])
    p, g, m, v, w16 = arena
    L.check(L.load().m3p_adam_step_ranges(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), L.ptr(w16), starts, counts, steps,
                                          zeros, n, hp['lr'], hp['beta1'], hp['beta2'], hp['eps'], hp['weight_decay'], L.ptr(gn),
                                          hp['max_norm'], hp['grad_scale'], L.stream()), 'm3p_adam_step_ranges')


def _range_shares(counts4, maxblk, quads_per_block, max_ranges):
    """Blocks the ranged launchers deal to the non-empty pieces of each launch (optim.hip m3p_adam_step_ranges and
    m3p_sumsq_ranges_f32: want = clamp(ceil(total4 / quads_per_block), pieces, maxblk); share = max(1, floor(n4 / total4 *
    want))), launch by launch of at most max_ranges non-empty pieces.  -> [(n4, share)] and the number of launches."""
    live = [c for c in counts4 if c > 0]
    out, launches = [], 0
    for k in range(0, len(live), max_ranges):
        grp = live[k:k + max_ranges]
        total = sum(grp)
        want = max(min(-(-total // quads_per_block), maxblk), len(grp))
        out += [(c, max(1, int(float(c) / float(total) * float(want)))) for c in grp]
        launches += 1
    return out, launches


def _piece_patterns(name):
    """[(start, end, step_size, zero_grad)] in floats and the arena size.  Step sizes and zero flags differ from piece to
    piece, pieces keep a guard band between them unless the pattern is about touching."""
    st = lambda k: 1e-3 * (1 + k % 5)             # noqa: E731
    if name == 'big_and_31_tiny':
        big = 8 << 20
        pieces = [(GUARD, GUARD + big, 2e-3, True)]
        pieces += [(GUARD + big + 64 * (k + 1), GUARD + big + 64 * (k + 1) + 4, st(k), k % 2 == 0) for k in range(31)]
    elif name in ('33_with_empties', '65_with_empties'):
        n_live = int(name[:2])
        pieces, at = [(GUARD, GUARD, 1e-3, True)], GUARD                       # an empty piece first
        for k in range(n_live):
            size = 4 * (1 + (k * 7919) % 3000) if k % 9 else 4 * 300_000
            pieces.append((at, at + size, st(k), k % 3 != 1))
            at += size + 64
            if k % 4 == 2:
                pieces.append((at, at, st(k), True))                            # empty ones interleaved
        pieces.append((at, at, 1e-3, False))                                    # and last
    elif name == 'touching':
        cuts = [GUARD, GUARD + 4, GUARD + 4 + 4 * 70_001, GUARD + 4 + 4 * 70_001 + 4 * 513, GUARD + 4 * 300_000, GUARD + 4 * 300_001]
        pieces = [(a, b, st(k), k % 2 == 0) for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:]))]
    elif name == 'above_2_28':
        base = (1 << 28) + 4 * 12_345
        pieces = [(GUARD, GUARD + 4 * 5000, 1e-3, True), (base, base + 4 * 600_001, 3e-3, False), (base + 4 * 600_001 + 64, base + 4 * 600_001 + 64 + 4, 2e-3, True)]
        assert pieces[1][0] > 2 ** 28
    size = max(b for _, b, _, _ in pieces) + GUARD
    return pieces, size


ADAM_PATTERNS = ['big_and_31_tiny', '33_with_empties', '65_with_empties', 'touching', 'above_2_28']


@pytest.mark.parametrize('pattern', ADAM_PATTERNS)
def test_adam_step_ranges_against_fp64(pattern):
    pieces, size = _piece_patterns(pattern)
    shares, launches = _range_shares([(b - a) // 4 for a, b, _, _ in pieces], ADAM_MAXBLK, THREADS, ADAM_MAX_RANGES)
    if pattern == 'big_and_31_tiny':
        n4, share = shares[0]
        assert launches == 1 and n4 > share * THREADS * ADAM_Q               # the big piece loops
        assert all(s == 1 and c == 1 for c, s in shares[1:])                  # the tiny ones: the forced single block
    elif pattern == '33_with_empties':
        assert launches == 2 and pieces[0][0] == pieces[0][1] and pieces[-1][0] == pieces[-1][1]
    elif pattern == '65_with_empties':
        assert launches == 3
    elif pattern == 'touching':
        assert all(a[1] == b[0] and a[2] != b[2] and a[3] != b[3] for a, b in zip(pieces[:-1], pieces[1:]))
    arena = _adam_arena(size, 50 + len(pieces))
    before = tuple(t.clone() for t in arena)
    live = [q for q in pieces if q[1] > q[0]]
    gn = torch.zeros(1, dtype=torch.float64, device='cuda')
    gn.copy_(sum((arena[1][a:b].double() ** 2).sum() for a, b, _, _ in live))
    hp = _hp(wd=0.01, grad_scale=0.5, gnorm_sq=float(gn))
    hp['max_norm'] = 0.5 * math.sqrt(hp['gnorm_sq']) * 0.5
    _adam_step_ranges_raw(arena, pieces, hp, gn)
    torch.cuda.synchronize()
    for k, (a, b, step_size, zero) in enumerate(live):
        worst = _check_adam_piece(arena, before, a, b, dict(hp, step_size=step_size), zero, 'adam_step_ranges %s piece %d [%d, %d)' % (pattern, k, a, b))
        for key, w in worst.items():
            _note('adam_ranges_kernel ' + key, w)
    _check_untouched(arena, before, 'adam_step_ranges ' + pattern)


# =====================================================================================================================
# Sum of squares
# =====================================================================================================================
def _sum64(x):
    return float(sum((x[i:i + U._CHUNK].double() ** 2).sum() for i in range(0, x.numel(), U._CHUNK)))


SUMSQ_BIG = 75_000_000 + 77           # quads: 300 M floats, the order of the largest configuration's gradient arena


@pytest.mark.parametrize('n4', [1, SUMSQ_FULL, SUMSQ_FULL + 1, 3 * SUMSQ_FULL + 77, SUMSQ_BIG])
def test_sumsq_sizes(n4):
    from m3p_amd import ops
    blocks = min(max(-(-n4 // SUMSQ_QUADS_PER_BLOCK), 1), SUMSQ_MAXBLK)
    threads = blocks * THREADS
    t = -(-n4 // threads)
    if n4 >= SUMSQ_FULL:
        assert blocks == SUMSQ_MAXBLK and n4 >= SUMSQ_UNROLL * threads       # the unrolled loop at the full grid
    if n4 > 3 * SUMSQ_FULL:
        assert n4 % (SUMSQ_UNROLL * threads) % threads == 77 or n4 == SUMSQ_BIG   # unrolled trips, then a ragged tail loop
    if n4 == SUMSQ_BIG:
        assert 4 * n4 >= 300_000_000 and t > 100
    g = torch.randn(4 * n4 + 8, device='cuda', generator=_gen(n4 % 991))[4:4 * n4 + 4] * 3.0
    g[-1] = 1e3                                                             # the very last element counts
    pre = 123.456
    out = torch.full((1,), pre, dtype=torch.float64, device='cuda')          # the kernel adds to what is there
    ops.sumsq(g, out)
    ref = _sum64(g)
    _note('sumsq_kernel', assert_sumsq_bound(float(out) - pre, ref, t, 'sumsq n4=%d' % n4))


def _sumsq_ranges_raw(buf, ranges, out):
    from m3p_amd import lib as L
    n = len(ranges)
    starts = (C.c_longlong * n)(*[int(a) for a, _ in ranges])
    counts = (C.c_longlong * n)(*[int(b - a) for a, b in ranges])
    L.check(L.load().m3p_sumsq_ranges_f32(buf.data_ptr(), starts, counts, n, out.data_ptr(), L.stream()), 'm3p_sumsq_ranges_f32')


@pytest.mark.parametrize('pattern', ADAM_PATTERNS)
def test_sumsq_ranges_against_fp64(pattern):
    pieces, size = _piece_patterns(pattern)
    ranges = [(a, b) for a, b, _, _ in pieces]
    shares, launches = _range_shares([(b - a) // 4 for a, b in ranges], SUMSQ_MAXBLK, SUMSQ_QUADS_PER_BLOCK, SUMSQ_MAX_RANGES)
    t = max(-(-c // (s * THREADS)) for c, s in shares)
    if pattern == 'big_and_31_tiny':
        assert shares[0][0] >= SUMSQ_UNROLL * shares[0][1] * THREADS         # the big piece runs the unrolled loop
    assert launches == {'33_with_empties': 2, '65_with_empties': 3}.get(pattern, 1)
    buf = torch.randn(size, device='cuda', generator=_gen(7)) * 2.0
    for a, b in ranges:
        if b > a:
            buf[b - 1] = 50.0                                               # the last element of every piece counts
    buf[[b for a, b in ranges if b + 1 < size]] = 1e4                       # and the one after it must not
    pre = -7.25
    out = torch.full((1,), pre, dtype=torch.float64, device='cuda')
    _sumsq_ranges_raw(buf, ranges, out)
    ref = sum(_sum64(buf[a:b]) for a, b in ranges if b > a)
    _note('sumsq_ranges_kernel', assert_sumsq_bound(float(out) - pre, ref, t, 'sumsq_ranges ' + pattern))


# =====================================================================================================================
# GELU passes, 8-bit quantisation, casts
# =====================================================================================================================
SPECIALS = [0.0, -0.0, 2.0 ** -20, -2.0 ** -20, 8.0, -8.0, 40.0, -40.0]
BF16_MAX = 3.3895313892515355e38
GELU_FULL = GELU_MAXBLK * THREADS * 8                # elements one trip of the full grid covers


def _assert_grid_loops(n, per_thread, maxblk):
    """More elements than one trip of the capped grid covers: some threads run their grid-stride loop again."""
    assert -(-n // (per_thread * THREADS)) > maxblk, (n, per_thread, maxblk)


def _gelu_input(shape, seed):
    u = (torch.randn(shape, device='cuda', generator=_gen(seed)) * 2.0).to(BF16)
    flat = u.view(-1)
    sp = torch.tensor(SPECIALS, device='cuda').to(BF16)
    flat[:8] = sp
    flat[-8:] = sp.flip(0)
    flat[8], flat[9], flat[-9], flat[-10] = BF16_MAX, -BF16_MAX, BF16_MAX, -BF16_MAX
    return u


def _elementwise(got, ref_fn, eps_fn, inputs, what, name):
    """assert_gemm_bound with depth 0 over a flat bf16 output in chunks: |got - ref| <= BF16_OUT |ref| + eps."""
    got = got.reshape(-1)
    flat = [x.reshape(-1) for x in inputs]
    for i0 in range(0, got.numel(), U._CHUNK):
        sl = slice(i0, i0 + U._CHUNK)
        xs = [x[sl].double() for x in flat]
        ref = ref_fn(*xs)
        w = assert_gemm_bound(got[sl].view(-1, 8), ref.view(-1, 8), torch.zeros_like(ref).view(-1, 8), 0, BF16_OUT, eps_fn(*xs).view(-1, 8),
                              what=what + ' (rows of 8 elements)', row0=i0 // 8)
        _note(name, w)


GELU_SHAPES = [(41984, 3072), (GELU_FULL - 8,), (GELU_FULL + 8,)]


@pytest.mark.parametrize('shape', GELU_SHAPES, ids=str)
def test_gelu_fwd_and_derivative(shape):
    from m3p_amd import ops
    if int(np.prod(shape)) > GELU_FULL:
        _assert_grid_loops(int(np.prod(shape)), 8, GELU_MAXBLK)
    u = _gelu_input(shape, 1)
    with poisoned_outputs():
        h = ops.gelu_fwd(u)
    _elementwise(h, _gelu64, lambda x: 2 * EPS_ERF * x.abs(), [u], 'gelu_fwd %s' % (shape,), 'gelu_fwd_kernel<false>')
    u2 = u.clone()
    with poisoned_outputs():
        h2 = ops.gelu_fwd(u2, grad_inplace=True)
    assert_bits_equal(h2, h, 'gelu_fwd(grad_inplace) h')
    _elementwise(u2, _dgelu64, lambda x: torch.full_like(x, EPS_DGELU), [u], 'gelu_fwd derivative %s' % (shape,), 'gelu_fwd_kernel<true> dh')


@pytest.mark.parametrize('shape', GELU_SHAPES, ids=str)
def test_gelu_bwd(shape):
    from m3p_amd import ops
    if int(np.prod(shape)) > GELU_FULL:
        _assert_grid_loops(int(np.prod(shape)), 8, GELU_MAXBLK)
    u = _gelu_input(shape, 2)
    dy = torch.randn(shape, device='cuda', generator=_gen(3)).to(BF16)
    dy.view(-1)[-8:] = torch.tensor([1.0, -1.0, 0.0, -0.0, 2.0 ** -20, 3.0, -5.0, 0.5], device='cuda').to(BF16)
    with poisoned_outputs():
        du = ops.gelu_bwd(dy, u)
    _elementwise(du, lambda g, x: g * _dgelu64(x), lambda g, x: EPS_DGELU * g.abs(), [dy, u], 'gelu_bwd %s' % (shape,), 'gelu_bwd_kernel')


def _fp8_ref(x, scale, bf8):
    """The 8-bit codes of torch's saturating cast of x * scale, in row chunks."""
    dt, lim = (torch.float8_e5m2, 57344.0) if bf8 else (torch.float8_e4m3fn, 448.0)
    flat = x.reshape(-1)
    out = torch.empty(flat.numel(), dtype=torch.uint8, device=x.device)
    for i0 in range(0, flat.numel(), 1 << 26):
        out[i0:i0 + (1 << 26)] = (flat[i0:i0 + (1 << 26)].float() * scale).clamp(-lim, lim).to(dt).view(torch.uint8)
    return out.view(x.shape)


QUANT_FULL = QUANT_MAXBLK * THREADS * 8
QUANT_EDGE = [0.0, -0.0, 1e-4, -2e-3, 500.0, -1000.0, 447.9, 60000.0]      # the values of test_fp8.py: signed zeros, saturation


@pytest.mark.parametrize('bf8', [False, True])
@pytest.mark.parametrize('shape', [(22784, 4096), (1, QUANT_FULL - 8), (1, QUANT_FULL + 8)], ids=str)
def test_quant_fp8_exact(shape, bf8):
    from m3p_amd import ops
    n = shape[0] * shape[1]
    if n > QUANT_FULL:
        _assert_grid_loops(n, 8, QUANT_MAXBLK)
    x = (torch.randn(shape, device='cuda', generator=_gen(5)) * 3.0).to(BF16)
    x[-1, -8:] = torch.tensor(QUANT_EDGE, device='cuda').to(BF16)
    x[-1, -16:-8] = -torch.tensor(QUANT_EDGE, device='cuda').to(BF16)
    x[0, 3] = 70000.0                                                       # the largest |x|: amax
    scale = torch.tensor([0.75], device='cuda')
    amax = torch.zeros(1, device='cuda')
    q = ops.quant_fp8(x, scale=scale, amax=amax, bf8=bf8)
    assert_bits_equal(q, _fp8_ref(x, 0.75, bf8), 'quant_fp8 %s bf8=%s' % (shape, bf8))
    assert float(amax) == float(x.float().abs().max())


@pytest.mark.parametrize('shape', [(41984, 3072), (GELU_FULL - 8,), (GELU_FULL + 8,)], ids=str)
def test_gelu_fwd_q8_is_gelu_then_quant(shape):
    """gelu_fwd_q8 = gelu_fwd then quant_fp8, bit for bit; gelu_fwd and quant_fp8 are held to their references at these sizes
    above, so the chain ends at one."""
    from m3p_amd import ops
    if int(np.prod(shape)) > GELU_FULL:
        _assert_grid_loops(int(np.prod(shape)), 8, GELU_MAXBLK)
    u = _gelu_input(shape, 6)
    scale = torch.tensor([3.0], device='cuda')
    amax = torch.zeros(1, device='cuda')
    with poisoned_outputs():
        h, h8 = ops.gelu_fwd_q8(u, scale, amax)
        href = ops.gelu_fwd(u)
    assert_bits_equal(h, href, 'gelu_fwd_q8 h')
    h2 = href.view(-1, 8)
    assert_bits_equal(h8.view(-1, 8), ops.quant_fp8(h2, scale=scale), 'gelu_fwd_q8 h8 against quant_fp8')
    assert_bits_equal(h8.view(-1, 8), _fp8_ref(h2, 3.0, False), 'gelu_fwd_q8 h8 against the torch cast')
    assert float(amax) == float(href.float().abs().max())


CAST_FULL = CAST_MAXBLK * THREADS * 4


@pytest.mark.parametrize('n', [CAST_FULL - 4, CAST_FULL + 4, 3 * CAST_FULL + 4 * 77])
def test_cast_f32_bf16_exact(n):
    from m3p_amd import ops
    if n > CAST_FULL:
        _assert_grid_loops(n, 4, CAST_MAXBLK)
    x = torch.randn(n, device='cuda', generator=_gen(8))
    x[-4:] = torch.tensor([0.0, -0.0, 1.00390625, -3.3895313892515355e38], device='cuda')     # a tie (to even), the largest bf16
    with poisoned_outputs():
        y = ops.cast_bf16(x)
    assert_bits_equal(y, x.to(BF16), 'cast_bf16 n=%d' % n)
    dst = torch.zeros(n + 8, dtype=BF16, device='cuda')
    ops.cast_f32_bf16_into(x, dst[4:n + 4])
    assert_bits_equal(dst[4:n + 4], x.to(BF16), 'cast_f32_bf16_into')
    assert_exact_zero(torch.cat([dst[:4], dst[n + 4:]]).float(), 'around the destination of cast_f32_bf16_into')


# =====================================================================================================================
# Gather / scatter
# =====================================================================================================================
@pytest.mark.parametrize('n,d', [(6298, 768), (41984, 1024)])
def test_gather_and_scatter_add_rows_exact(n, d):
    from m3p_amd import ops
    _assert_grid_loops(n * d, 4, ROWS_MAXBLK)
    rows = n + n // 3
    src = torch.randn((rows, d), device='cuda', generator=_gen(9)).to(BF16)
    idx = torch.randperm(rows, device='cuda', generator=_gen(10))[:n].to(torch.int32)
    with poisoned_outputs():
        out = ops.gather_rows(src, idx, n, d)
    assert_bits_equal(out, src[idx.long()], 'gather_rows')
    dst = torch.randn((rows, d), device='cuda', generator=_gen(11)).to(BF16)
    dst0 = dst.clone()
    ops.scatter_add_rows(out, idx, dst, n, d)
    ref = dst0.clone()
    ref[idx.long()] = (dst0[idx.long()].float() + out.float()).to(BF16)      # one bf16 add per element
    assert_bits_equal(dst, ref, 'scatter_add_rows')                          # (rows outside idx: bit-identical)


def test_scatter_add_token_rows_with_repeats_and_padding():
    from m3p_amd import ops
    n, V, d, ld, pad = 32768 + 3, 1000, 768, 768 + 64, 1
    assert -(-n // 4) > TOKROWS_MAXBLK
    buf = torch.randn((n, ld), device='cuda', generator=_gen(12)).to(BF16)
    rows = buf[:, :d]
    assert rows.stride(0) > d
    ids = torch.randint(0, V, (n,), device='cuda', generator=_gen(13))
    ids[::7] = pad
    ids[-1] = V - 1                                                         # the last row, looped to by the last wave
    dst = torch.randn((V, d), device='cuda', generator=_gen(14))
    dst0 = dst.clone()
    ops.scatter_add_token_rows(rows, ids, dst, pad)
    live = ids != pad
    r64 = rows.double() * live[:, None]
    ref = dst0.double().index_add(0, ids, r64)
    absref = dst0.double().abs().index_add(0, ids, r64.abs())
    cnt = 1 + torch.bincount(ids[live], minlength=V).double()
    _note('scatter_add_token_rows_kernel', assert_accum_bound(dst, ref, absref, cnt[:, None], what='scatter_add_token_rows'))
    assert_bits_equal(dst[pad], dst0[pad], 'scatter_add_token_rows: the padding row')


# =====================================================================================================================
# Embedding assembly
# =====================================================================================================================
def _keep_dev(n, seed, p, shape):
    """m3p_amd/rng.py keep_mask on the device (fp64 0 / 1): 32 M elements of integer hashing are slow on the host.  Its first
    elements are compared with the NumPy twin on every call."""
    from m3p_amd import rng
    if p == 0:
        return torch.ones(shape, dtype=torch.float64, device='cuda')
    idx = torch.arange(n, dtype=torch.int64, device='cuda')
    m32, m24 = 0xFFFFFFFF, 0xFFFFFF
    h = ((idx >> 1) + (int(seed) & m32)) & m32
    for k in (0x9E3779, 0x85EBCB, 0xC2B2AF):
        h ^= h >> 16
        h = (h + (h & m24) * k) & m32
    h ^= h >> 16
    half = torch.where((idx & 1) != 0, h >> 16, h & 0xFFFF)
    keep = half >= (int(round(float(p) * (1 << 24))) >> 8)
    k0 = min(n, 8192)
    assert np.array_equal(keep[:k0].cpu().numpy(), rng.keep_mask(k0, seed, p))
    return keep.double().view(shape)


def _ln64(x, eps=1e-12):
    mu = x.mean(-1, keepdim=True)
    rs = 1.0 / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + eps)
    return mu, rs, (x - mu) * rs


def _ln_bwd64(dy, g, xh, rs):
    """LayerNorm backward of one row set in fp64 and the same expression over absolute values (every fp32 operation of the
    kernel rounds relative to its operands)."""
    gd = dy * g
    c1, c2 = gd.mean(-1, keepdim=True), (gd * xh).mean(-1, keepdim=True)
    a1, a2 = gd.abs().mean(-1, keepdim=True), (gd * xh).abs().mean(-1, keepdim=True)      # (the means round relative to these)
    return (gd - c1 - xh * c2) * rs, (gd.abs() + a1 + xh.abs() * a2) * rs


def _bsplit(B, S):
    """embed.hip m3p_embed_assemble_bwd: the batch is split until about EMB_BWD_BLOCKS blocks are in flight."""
    bsplit = 1
    while bsplit < 16 and S * bsplit < EMB_BWD_BLOCKS and B // (4 * bsplit) >= 8:
        bsplit *= 2
    return bsplit


# Two bf16 roundings lie between de and exact inputs: dz (the gradient of the LayerNorm input, which the row kernel stores
# for the image kernel) and de itself.  One rounding moves an element by at most 2^-8 of itself, so a row by at most
# ROW_RTOL_BF16 of its norm, and the LayerNorm backward between the two removes two directions of a d-dimensional row and
# scales the rest alike, so the rounding of dz reaches de with the same relative size.  Over a row of d >= 512 elements the
# two are independent and add in quadrature: sqrt(2) ROW_RTOL_BF16 (util.EMBED_DE_RTOL; the restatement of
# tests/test_parity_bounds.py reaches 0.48 of ROW_RTOL_BF16 with one rounding and 0.68 with two).  h, z and e are each one
# rounding away from the saved bf16 tensor before them and are compared with fp64 of that tensor.
EMBED_CASES = [  # B, T, R, d, NI, bsplit, forward grid loops
    (256, 128, 36, 768, 3, 4, True), (32, 128, 36, 1024, 4, 2, False), (512, 24, 8, 512, 2, 16, False), (67, 24, 36, 768, 3, 4, False),
    (256, 128, 0, 768, 3, 4, True)]


@pytest.mark.parametrize('p_drop', [0.0, 0.1])
@pytest.mark.parametrize('B,T,R,d,ni,bsplit,fwd_loops', EMBED_CASES)
def test_embed_assemble_at_the_sizes_that_split_the_batch(B, T, R, d, ni, bsplit, fwd_loops, p_drop):
    from m3p_amd import ops
    V, S, pad = 1000, R + T, 1
    assert (d + 255) // 256 == ni and _bsplit(B, S) == bsplit
    assert (-(-B * S // 4) > EMBED_FWD_MAXBLK) == fwd_loops
    if (B, R) == (67, 36):
        assert B % (4 * bsplit) != 0                                        # the last slice of the batch is ragged
    gen = _gen(B + d)
    rnd = lambda *shape, scale=1.0: torch.randn(shape, device='cuda', generator=gen) * scale       # noqa: E731
    lens = torch.randint(1, T + 1, (B,), device='cuda', generator=gen)
    lens[0], lens[1] = 1, T                                                 # a single token; the full length
    tok = torch.randint(2, V - 50, (T, B), device='cuda', generator=gen)    # V - 50 .. V - 1 never occur
    tok[torch.arange(T, device='cuda')[:, None] >= lens[None, :]] = pad
    tok[0, 5] = pad                                                         # a padding token inside a sequence
    totlen = (lens + R).int()
    emb16 = rnd(V, d, scale=0.5).to(BF16)
    pos = rnd(S + 3, d, scale=0.1)
    w_loc, b_loc = rnd(d, 5, scale=0.3), rnd(d, scale=0.1)
    g_img, be_img, g_emb, be_emb = 1 + rnd(d, scale=0.1), rnd(d, scale=0.1), 1 + rnd(d, scale=0.1), rnd(d, scale=0.1)
    img_proj = loc = None
    if R:
        img_proj, loc = rnd(R * B, d).to(BF16), rnd(R, B, 5)
    seed_i, seed_e = 111, 222
    what = 'embed (B, T, R, d) = %s p_drop = %s' % ((B, T, R, d), p_drop)
    with poisoned_outputs():
        h, saved = ops.embed_assemble_fwd(tok, emb16, pos, img_proj, loc, w_loc, b_loc, g_img, be_img, g_emb, be_emb, totlen, B, T, R, d,
                                          seed_img=seed_i, seed_emb=seed_e, p_drop=p_drop)
    z_s, e_s = saved[0].double().view(B, S, d), saved[3].double()
    ik = 1.0 / (1.0 - p_drop)
    keep_e = _keep_dev(B * S * d, seed_e, p_drop, (B, S, d))
    keep_i = _keep_dev(R * B * d, seed_i, p_drop, (R, B, d)) if R else None
    mask = (torch.arange(S, device='cuda')[None, :] < totlen[:, None]).double()[..., None]
    D = lambda t: t.double()                                                # noqa: E731
    # --- forward, stage by stage: each saved bf16 tensor against fp64 of the exact inputs before it
    z_ref = torch.empty((B, S, d), dtype=torch.float64, device='cuda')
    if R:
        e_ref = D(img_proj).view(R, B, d) + D(b_loc) + D(loc) @ D(w_loc).t()
        _note('embed_fwd e', assert_block_bound(e_s.view(R * B, d), e_ref.view(R * B, d), ('row',), ROW_RTOL_BF16, ROW_FLOOR, what + ': e') / ROW_RTOL_BF16)
        mu_i, rs_i, xh_i = _ln64(e_s.view(R, B, d))
        z_ref[:, :R] = ((xh_i * D(g_img) + D(be_img)) * keep_i * ik).transpose(0, 1) + D(pos[:R])
    z_ref[:, R:] = D(emb16)[tok.t()] + D(pos[R:S])
    z_ref *= mask
    _note('embed_fwd z', assert_block_bound(z_s, z_ref, ('b', 's'), ROW_RTOL_BF16, ROW_FLOOR, what + ': z') / ROW_RTOL_BF16)
    assert_exact_zero(saved[0].view(B, S, d)[mask[..., 0] == 0], what + ': z past totlen')
    mu, rs, xh = _ln64(z_s)
    h_ref = (xh * D(g_emb) + D(be_emb)) * keep_e * ik                       # (rows past totlen: the bias under the mask)
    _note('embed_fwd h', assert_block_bound(h.view(B, S, d), h_ref, ('b', 's'), ROW_RTOL_BF16, ROW_FLOOR, what + ': h') / ROW_RTOL_BF16)
    del z_ref, h_ref
    # --- backward reference from the saved z, e and dh
    dh = rnd(B * S, d).to(BF16)
    dy = D(dh).view(B, S, d) * keep_e * ik
    o, abs_o = _ln_bwd64(dy, D(g_emb), xh, rs)
    o, abs_o = o * mask, abs_o * mask
    ref, absr, nterms, extra = {}, {}, {}, {}
    ref['d_g_emb'], absr['d_g_emb'], nterms['d_g_emb'] = (dy * xh).sum((0, 1)), (dy.abs() * (z_s.abs() + mu.abs()) * rs).sum((0, 1)), B * S
    ref['d_be_emb'], absr['d_be_emb'], nterms['d_be_emb'] = dy.sum((0, 1)), dy.abs().sum((0, 1)), B * S
    tail = torch.zeros((3, d), dtype=torch.float64, device='cuda')           # the table has rows past S: nothing is added there
    ref['d_pos'], absr['d_pos'], nterms['d_pos'] = torch.cat([o.sum(0), tail]), torch.cat([abs_o.sum(0), tail]), B
    ids = tok.t().reshape(-1)
    live = ((ids != pad)[:, None] * mask[:, R:, 0].reshape(-1, 1))
    o_tok = o[:, R:].reshape(-1, d) * live
    ref['d_emb'] = torch.zeros((V, d), dtype=torch.float64, device='cuda').index_add(0, ids, o_tok)
    absr['d_emb'] = torch.zeros((V, d), dtype=torch.float64, device='cuda').index_add(0, ids, abs_o[:, R:].reshape(-1, d) * live)
    count = torch.bincount(ids[live[:, 0] != 0], minlength=V)
    nterms['d_emb'] = count.double()[:, None]
    assert int((count == 0).sum()) >= 50 and int(count.max()) > 1           # rows that never occur, rows that repeat
    if B * T >= 8 * V:
        assert int((count > 1).sum()) > (V - 52) // 2                       # most repeat
    if R:
        dyi = o[:, :R].transpose(0, 1) * keep_i * ik
        abs_dyi = abs_o[:, :R].transpose(0, 1) * keep_i * ik
        de_ref, _ = _ln_bwd64(dyi, D(g_img), xh_i, rs_i)
        e3 = e_s.view(R, B, d)
        half = 2.0 ** -9                      # the bf16 rounding of dz: at most 2^-8 of a term, of random sign term by term
        ref['d_g_img'], absr['d_g_img'], nterms['d_g_img'] = (dyi * xh_i).sum((0, 1)), (abs_dyi * (e3.abs() + mu_i.abs()) * rs_i).sum((0, 1)), R * B
        extra['d_g_img'] = U.KAPPA * half * (dyi * xh_i).pow(2).sum((0, 1)).sqrt()
        ref['d_be_img'], absr['d_be_img'], nterms['d_be_img'] = dyi.sum((0, 1)), abs_dyi.sum((0, 1)), R * B
        extra['d_be_img'] = U.KAPPA * half * dyi.pow(2).sum((0, 1)).sqrt()
    used_pos = int(totlen.max())

    def fresh():
        return {k: torch.zeros(s, device='cuda') for k, s in dict(
            d_g_emb=(d,), d_be_emb=(d,), d_pos=(S + 3, d), d_emb=(V, d), d_g_img=(d,), d_be_img=(d,), d_b_img=(d,), d_b_loc=(d,),
            d_w_loc=(d, 5)).items()}

    def check(grads, de, route, tok_rows=None):
        """Rows first (a failure names the sequence), then the sums."""
        w = '%s, %s' % (what, route)
        if R:
            _note('embed_bwd de', assert_block_bound(de.view(R, B, d), de_ref, ('r', 'b'), EMBED_DE_RTOL, ROW_FLOOR, w + ': de') / EMBED_DE_RTOL)
        for k in ('d_pos', 'd_emb', 'd_g_emb', 'd_be_emb', 'd_g_img', 'd_be_img'):
            if (k == 'd_emb' and tok_rows is not None) or k not in ref:
                continue
            _note('embed_bwd ' + k, assert_accum_bound(grads[k], ref[k], absr[k], nterms[k], extra.get(k, 0.0), what='%s: %s' % (w, k)))
        assert_exact_zero(grads['d_pos'][used_pos:], w + ': d_pos past the longest sequence and past S')
        if tok_rows is None:
            assert_exact_zero(grads['d_emb'][count == 0], w + ': d_emb rows of tokens that never occur')
            assert_exact_zero(grads['d_emb'][pad], w + ': d_emb padding row')
        if R:
            # the sums over de are sums of the rounded values the kernel stored: exact up to their fp32 accumulation
            de64 = D(de)
            loc2 = D(loc).view(R * B, 5)
            for k in ('d_b_img', 'd_b_loc'):
                _note('embed_bwd ' + k, assert_accum_bound(grads[k], de64.sum(0), de64.abs().sum(0), R * B, what='%s: %s' % (w, k)))
            _note('embed_bwd d_w_loc', assert_accum_bound(grads['d_w_loc'], de64.t() @ loc2, de64.abs().t() @ loc2.abs(), R * B, what=w + ': d_w_loc'))

    args = (dh, saved, g_emb, g_img, tok, totlen, loc)
    kw = dict(seed_img=seed_i, seed_emb=seed_e, p_drop=p_drop)
    grads = fresh()
    with poisoned_outputs():
        de = ops.embed_assemble_bwd(*args, grads, B, T, R, d, pad, **kw)
    check(grads, de, 'one call')
    if R:       # the two-phase route with an identity between the halves: the same results against the same reference
        grads = fresh()
        with poisoned_outputs():
            de = ops.embed_assemble_bwd(*args, grads, B, T, R, d, pad, img_rows_bwd=lambda t: t, **kw)
        check(grads, de, 'phases 1 and 2')
    # token rows handed out instead of scattered
    grads = fresh()
    grads['d_emb'].fill_(3.25)
    rows = torch.full((T * B, d), float('nan'), dtype=BF16, device='cuda')
    with poisoned_outputs():
        de = ops.embed_assemble_bwd(*args, grads, B, T, R, d, pad, tok_rows=rows, **kw)
    check(grads, de, 'tok_rows', tok_rows=rows)
    rows_ref = o_tok.view(B, T, d).transpose(0, 1)
    _note('embed_bwd tok_rows', assert_block_bound(rows.view(T, B, d), rows_ref, ('t', 'b'), ROW_RTOL_BF16, ROW_FLOOR, what + ': tok_rows') / ROW_RTOL_BF16)
    assert_exact_zero(rows.view(T, B, d)[live.view(B, T).t() == 0], what + ': tok_rows of padding and masked tokens')
    assert_bits_equal(grads['d_emb'], torch.full_like(grads['d_emb'], 3.25), what + ': d_emb with tok_rows')


def test_zz_report_worst_normalised_errors():
    """Not a check: prints what the bounds above were reached by (run with -s or -rP)."""
    for k in sorted(WORST):
        print('worst normalised error  %-28s %.3f' % (k, WORST[k]))
