"""The persistent GEMMs under the two process-wide schedule switches (include/m3p_hip.h): the per-XCD tile queues of the
eight-wave NT kernel (m3p_set_tile_queue -> gemm_nt_w8_kernel<EPI, true>) and a reduced persistent grid
(m3p_set_persistent_grid), which every launcher of csrc/gemm.hip that sizes its grid by the CU count follows.  The rest of
the suite runs one schedule only: the full grid with static tile dealing.

Nothing here has a bound of its own.  Queued launches are held to the elementwise bounds of tests/test_gemm.py
(_check_epilogues) and, bit for bit, to the same call under the default schedule - a tile's arithmetic does not depend on
which workgroup computes it.  The reduced-grid cases are the bodies of the existing tests, called inside
tests.util.gemm_schedule; the NT products among them are again bit-equal to the full-grid launch.  The products that split the
contraction (weight gradients, the NN product on the weight-gradient kernel, stream-K) are not: their segment boundaries and
the order of their partial sums follow the grid, so they are held to the bounds alone.

No test can pass by running the default schedule: every queued launch asserts KERN_NT_W8_QUEUE and the counters its slot
must hold afterwards, every reduced-grid test first asserts a dispatch answer that only the reduced grid gives."""
import contextlib

import pytest
import torch

from m3p_amd import lib as L
from m3p_amd import ops
from tests import test_fp8 as TF8
from tests import test_gemm as TG
from tests import test_mlm_shifted_gpu as TSH
from tests import test_wgrad_group as TWG
from tests.test_gemm import _check_epilogues, _keep_rows_dev, _prod64
from tests.util import (F32_OUT, assert_bits_equal, assert_gemm_bound, gemm_schedule, poisoned_outputs, randn_bf16, randn_f32,
                        rel_l2)

pytestmark = pytest.mark.gpu

SEED, P_DROP = 99, 0.1
GUARD_COLS = 8                  # behind the N columns of the NONE / BIAS outputs (a pitch that keeps the 16-byte row stores)
QUEUE_EPIS = ('none', 'bias', 'gelu', 'drop_res', 'res')
EPI = {'none': L.EPI_NONE, 'bias': L.EPI_BIAS, 'gelu': L.EPI_BIAS_GELU, 'drop_res': L.EPI_BIAS_DROP_RES, 'res': L.EPI_RES}
A_SHAPE, B_SHAPE = (1024, 768, 512), (1024, 768, 576)       # 12 tiles each; 8 and 9 K-tiles


def _grid(g):
    """'full' = one workgroup per CU; 'reserve8' = what M3P_DP_RESERVE_CUS=8 sets."""
    return L.num_cus() if g == 'full' else L.num_cus() - 8 if g == 'reserve8' else g


def _set(g):
    """The argument of m3p_set_persistent_grid for grid g (0 = the default)."""
    return 0 if g == 'full' else _grid(g)


def _nt_plan(M, N, K, epi):
    return L.load().m3p_gemm_nt_plan(M, N, K, epi)


def _wgrad_plan(M, N, K):
    return L.load().m3p_gemm_wgrad_plan(M, N, K)


def _xcd_tiles(ntiles, nwg):
    """Tiles of each XCD's queue: position p of XCD x is tile (p // per_xcd) * nwg + x * per_xcd + p % per_xcd (csrc/gemm.hip,
    gemm_nt_w8_kernel), i.e. XCD x holds the tiles t with (t % nwg) // per_xcd == x."""
    per_xcd = nwg // 8
    return [sum(1 for t in range(ntiles) if (t % nwg) // per_xcd == x) for x in range(8)]


# ---------------------------------------------------------------------------------------------------------------------
# Operands, fp64 products and the default schedule's outputs of one shape: made once, shared by every test that launches it
# ---------------------------------------------------------------------------------------------------------------------
_CASES = {}


def _launch(c, name):
    """One epilogue of case c as the parity tests launch it -> the tensors it wrote (compared bit for bit, guards included)."""
    M, N, K = c['shape']
    a, w, bias, r = c['a'], c['w'], c['bias'], c['r']
    with poisoned_outputs():
        if name in ('none', 'bias'):
            buf = torch.empty((M, N + GUARD_COLS), dtype=torch.bfloat16, device='cuda')
            buf.untyped_storage().fill_(0xFF)
            if name == 'none':
                ops.gemm_nt(a, w, L.EPI_NONE, out=buf, n=N)
            else:
                ops.gemm_nt(a, w, L.EPI_BIAS, bias=bias, scale_cols=N // 3, scale=0.125, out=buf, n=N)
            return (buf,)
        if name == 'gelu':
            u = torch.empty((M, N), dtype=torch.bfloat16, device='cuda')
            u.untyped_storage().fill_(0xFF)
            h = ops.gemm_nt(a, w, L.EPI_BIAS_GELU, bias=bias, out2=u)
            return (u, h)
        if name == 'drop_res':
            return (ops.gemm_nt(a, w, L.EPI_BIAS_DROP_RES, bias=bias, aux=r, seed=SEED, p_drop=P_DROP),)
        assert name == 'res'
        return (ops.gemm_nt(a, w, L.EPI_RES, aux=r, alpha=0.5),)


def _case(M, N, K):
    """Call it under the default schedule only: the first call launches the static twins."""
    c = _CASES.get((M, N, K))
    if c is None:
        assert torch.cuda.current_device() not in ops._TILE_QUEUE
        c = {'shape': (M, N, K)}
        c['a'], c['w'] = randn_bf16((M, K), 1)[0], randn_bf16((N, K), 2, 0.05)[0]
        c['bias'], c['r'] = randn_f32((N,), 3)[0], randn_bf16((M, N), 4)[0]
        c['p64'], c['ap64'] = _prod64(c['a'], c['w'])
        c['keep'] = _keep_rows_dev(0, M, N, SEED, P_DROP)
        assert L.load().m3p_set_persistent_grid(0) == 0
        c['static'] = {name: _launch(c, name) for name in QUEUE_EPIS}
        # the eight-wave kernel's static schedule where the default table picks the four-wave kernel (K >= 2048, unarmed)
        if _nt_plan(M, N, K, L.EPI_NONE) != L.KERN_NT_W8:
            torch.cuda.synchronize()
            L.load().m3p_debug_set_variant(6)
            try:
                c['static_w8'] = {name: _launch(c, name) for name in QUEUE_EPIS}
                torch.cuda.synchronize()
            finally:
                L.load().m3p_debug_set_variant(1)
        torch.cuda.synchronize()
        _CASES[(M, N, K)] = c
    return c


def _verify(c, name, got, what):
    """Every element of one epilogue's outputs within the bounds of tests/test_gemm.py, the guard columns untouched, and all of
    it bit for bit what the default schedule left."""
    M, N, K = c['shape']
    if name in ('none', 'bias'):
        buf = got[0]
        assert bool((buf[:, N:].contiguous().view(torch.int16) == -1).all()), '%s %s: wrote behind column N' % (what, name)
        outs = {'none': buf[:, :N]} if name == 'none' else {'bias': (buf[:, :N], N // 3)}
    elif name == 'gelu':
        outs = {'gelu': got}
    elif name == 'drop_res':
        outs = {'drop_res': (got[0], c['keep'], P_DROP)}
    else:
        outs = {'res': got[0]}
    _check_epilogues(K, c['p64'], c['ap64'], c['bias'], c['r'], outs)
    for k, (g, s) in enumerate(zip(got, c['static'][name])):
        assert_bits_equal(g, s, '%s %s: output %d against the default schedule' % (what, name, k))
    if 'static_w8' in c:
        for k, (g, s) in enumerate(zip(got, c['static_w8'][name])):
            assert_bits_equal(g, s, '%s %s: output %d against the eight-wave kernel\'s static schedule' % (what, name, k))


def _queued(pool, k, c, name, nwg, launch=None):
    """The k-th queued launch since the queue was armed.  Its slot - eight counters, one per XCD - is clear before it (as is
    every later slot) and holds the tile counts of the XCDs' queues afterwards:
      every workgroup pops once per tile it loads (at K-tile 3 of that tile), the pop that finds no tile included;
      the pops of an XCD return consecutive positions, so they hand out every tile of its queue exactly once;
      hence pops = tiles loaded = the tiles of the queue, whichever workgroup took them (_xcd_tiles; none is 0: a queued
      launch has more tiles than workgroups).
    A skipped or doubled tile, a slot that was not clear or a launch that took the static schedule all show here."""
    M, N, K = c['shape']
    assert _nt_plan(M, N, K, EPI[name]) == L.KERN_NT_W8_QUEUE, (c['shape'], name)
    slots = pool.view(-1, 8)
    torch.cuda.synchronize()
    assert not bool(slots[k:].any()), 'slots %d.. must be clear before queued launch %d' % (k, k)
    out = launch() if launch else _launch(c, name)
    torch.cuda.synchronize()
    want = _xcd_tiles((M // 256) * (N // 256), nwg)
    assert min(want) > 0 and slots[k].tolist() == want, (k, slots[k].tolist(), want)
    assert not bool(slots[k + 1:].any()), 'queued launch %d touched a later slot' % k
    return out


def _reduced(g):
    """Dispatch answers that only a persistent grid of g gives - 256 x 256 tiles: g + 8 of them are more than the workgroups
    (whole tiles round-robin; under the default grid they are not), g of them are not (one segment per workgroup; under a
    smaller grid they are.  8 is the smallest grid, and 8 tiles are too few for either mode)."""
    ncu, g = L.num_cus(), _grid(g)
    assert 8 <= g <= ncu - 8 and g % 8 == 0
    above = _wgrad_plan(4096, 256 * (g // 8 + 1), 2048) == L.KERN_WGRAD_W4_TILES
    return above and (g == 8 or _wgrad_plan(4096, 256 * (g // 8), 2048) == L.KERN_WGRAD_W4_CHUNKS)


def _defaults_hold():
    assert torch.cuda.current_device() not in ops._TILE_QUEUE
    assert _nt_plan(1024, 768, 512, L.EPI_BIAS) == L.KERN_NT_W8
    assert _nt_plan(4352, 4096, 512, L.EPI_BIAS) == L.KERN_NT_W8
    assert _nt_plan(1024, 768, 3072, L.EPI_BIAS) == L.KERN_NT_W4
    assert _wgrad_plan(4096, 1536, 1536) == L.KERN_WGRAD_W4_CHUNKS
    assert not any(_reduced(g) for g in (8, 64, 'reserve8'))


# ---------------------------------------------------------------------------------------------------------------------
# A. The dispatch table under the switches
# ---------------------------------------------------------------------------------------------------------------------
ALL_EPIS = (L.EPI_NONE, L.EPI_BIAS, L.EPI_BIAS_GELU, L.EPI_BIAS_DROP_RES, L.EPI_RES, L.EPI_DGELU, L.EPI_MUL, L.EPI_MULQ,
            L.EPI_BIAS_GELUQ, L.EPI_BIAS_LSE)
WHOLE = [(M, N, K) for M in (1024, 1280, 2304, 4352) for N in (512, 768, 2304, 4096) for K in (448, 512, 576, 3072)]
RAGGED = [(1000, 768, 512), (1024, 640, 512), (768, 768, 512), (1024, 256, 512), (2048 + 40, 1000, 128)]


def _all_plans():
    return {(s, e): _nt_plan(*s, e) for s in WHOLE + RAGGED for e in ALL_EPIS}


def test_plan_table_under_the_switches():
    lib = L.load()
    _defaults_hold()
    before = _all_plans()
    assert L.KERN_NT_W8_QUEUE not in before.values()
    for g in (8, 16, 'full'):
        nwg = _grid(g)
        with gemm_schedule(grid=_set(g), queue_slots=4):
            for (M, N, K) in WHOLE:
                ntiles = (M // 256) * (N // 256)
                grid = nwg if ntiles >= nwg else (ntiles + 7) // 8 * 8            # persistent_grid(ntiles)
                for e in ALL_EPIS:
                    queued = e in EPI.values() and K >= 512 and ntiles > grid
                    assert _nt_plan(M, N, K, e) == (L.KERN_NT_W8_QUEUE if queued else L.KERN_NT_W8), (g, M, N, K, e)
            for s in RAGGED:            # nothing but whole tiles is queued, and arming moves nothing else
                for e in ALL_EPIS:
                    assert _nt_plan(*s, e) == before[(s, e)], (g, s, e)
            # the rule's clauses one by one, on the production shape (272 tiles)
            for e in (L.EPI_DGELU, L.EPI_MUL, L.EPI_MULQ, L.EPI_BIAS_GELUQ, L.EPI_BIAS_LSE):
                assert _nt_plan(4352, 4096, 512, e) == L.KERN_NT_W8
            assert _nt_plan(4352, 4096, 448, L.EPI_BIAS) == L.KERN_NT_W8
            assert _nt_plan(1024, 512, 512, L.EPI_BIAS) == L.KERN_NT_W8            # 8 tiles: never more than the grid
            assert before[((1024, 768, 3072), L.EPI_BIAS)] == L.KERN_NT_W4
            assert _nt_plan(1024, 768, 3072, L.EPI_BIAS) == (L.KERN_NT_W8_QUEUE if nwg < 12 else L.KERN_NT_W8)
            assert _nt_plan(4352, 4096, 3072, L.EPI_RES) == L.KERN_NT_W8_QUEUE and before[((4352, 4096, 3072), L.EPI_RES)] == L.KERN_NT_W4
        assert _all_plans() == before, 'grid %s: the answers after the context' % (g,)
    # the grid setter: multiples of 8 only, a refused value changes nothing, a taken one moves the weight-gradient table
    with gemm_schedule(grid=8):
        assert _wgrad_plan(4096, 1536, 1536) == L.KERN_WGRAD_W4_TILES
        assert lib.m3p_set_persistent_grid(12) == -1 and lib.m3p_set_persistent_grid(-8) == -1
        assert _wgrad_plan(4096, 1536, 1536) == L.KERN_WGRAD_W4_TILES
        assert _wgrad_plan(8192, 768, 768) == L.KERN_WGRAD_W4_TILES             # 9 tiles on 8 workgroups
        assert all(_reduced(g) == (g == 8) for g in (8, 64, 'reserve8'))
    _defaults_hold()


# ---------------------------------------------------------------------------------------------------------------------
# B. The queue instantiation, every epilogue it has
# ---------------------------------------------------------------------------------------------------------------------
QUEUE_CASES = [(8, A_SHAPE),                    # per_xcd = 1; 12 tiles: four XCDs pop a tile, four find none; nk = 8, the shortest K that queues
               (8, B_SHAPE),                    # odd nk
               (16, (1280, 1024, 768)),         # per_xcd = 2; 20 tiles: uneven queues
               (16, (2304, 2304, 768)),         # tiles_n = 9: the strip walk of split_tile; 81 tiles
               (64, (2304, 2304, 768)),
               (8, (1024, 768, 3072)),          # K >= 2048: the four-wave kernel's product while the queue is off (12 tiles: a
                                                #  grid of 16 would give each its own workgroup and queue nothing)
               ('full', (4352, 4096, 512))]     # more tiles (272) than CUs: the production per_xcd


def _queue_case(g, shape, slots=8):
    c = _case(*shape)
    with gemm_schedule(grid=_set(g), queue_slots=slots) as pool:
        if g != 'full':
            assert _reduced(g)
        got = {name: _queued(pool, k, c, name, _grid(g)) for k, name in enumerate(QUEUE_EPIS)}
    for name in QUEUE_EPIS:
        _verify(c, name, got[name], 'grid %s, %s' % (g, shape))


@pytest.mark.parametrize('g,shape', QUEUE_CASES)
def test_queued_launches_against_fp64_and_the_static_schedule(g, shape):
    if shape[2] >= 2048:
        assert _nt_plan(*shape, L.EPI_BIAS) == L.KERN_NT_W4
    _queue_case(g, shape)


# ---------------------------------------------------------------------------------------------------------------------
# C. The slot ring, streams, launches the queue does not take
# ---------------------------------------------------------------------------------------------------------------------
def test_slot_hand_out():
    c = _case(*A_SHAPE)
    with gemm_schedule(grid=8, queue_slots=4) as pool:
        assert _reduced(8) and pool.numel() == 32 and not bool(pool.any())
        for k, name in enumerate(('bias', 'res', 'none')):
            _verify(c, name, _queued(pool, k, c, name, 8), 'slot %d' % k)


def test_ring_wrap_clears_the_slots():
    """Twelve queued launches back to back through a ring of three slots: without the memset in front of a reused slot its
    counters start at the previous launch's counts and the workgroups skip those tiles (NaN out of the poisoned outputs)."""
    cs = [_case(*A_SHAPE), _case(*B_SHAPE)]
    names = ('drop_res', 'bias', 'gelu')
    with gemm_schedule(grid=8, queue_slots=3) as pool:
        assert _reduced(8)
        runs = []
        for i in range(12):
            c, name = cs[i % 2], names[i % 3]
            assert _nt_plan(*c['shape'], EPI[name]) == L.KERN_NT_W8_QUEUE
            runs.append((c, name, _launch(c, name)))
        torch.cuda.synchronize()
        # launches 9, 10, 11 were the last to take slots 0, 1, 2, cleared in front of launch 9: one launch's counts each
        want = _xcd_tiles(12, 8)
        assert pool.view(-1, 8).tolist() == [want] * 3, pool.view(-1, 8).tolist()
    for i, (c, name, got) in enumerate(runs):
        for k, (g, s) in enumerate(zip(got, c['static'][name])):
            assert_bits_equal(g, s, 'launch %d (%s), output %d' % (i, name, k))


def test_launches_the_queue_does_not_take_leave_the_pool_alone():
    c = _case(*A_SHAPE)
    M, N, K = A_SHAPE
    a448, w448 = c['a'][:, :448], c['w'][:, :448]                 # K = 448: seven K-tiles
    a8, w8 = c['a'], c['w'][:512]                                 # N = 512: 8 tiles on 8 workgroups
    with gemm_schedule(grid=8, queue_slots=4) as pool:
        assert _reduced(8)
        _queued(pool, 0, c, 'bias', 8)
        snap = pool.clone()
        assert _nt_plan(M, N, K, L.EPI_DGELU) == L.KERN_NT_W8 and _nt_plan(M, N, 448, L.EPI_BIAS) == L.KERN_NT_W8
        assert _nt_plan(M, 512, K, L.EPI_BIAS) == L.KERN_NT_W8
        with poisoned_outputs():
            dg = ops.gemm_nt(c['a'], c['w'], L.EPI_DGELU, aux=c['r'], colsum=torch.zeros(N, device='cuda'))
            short = ops.gemm_nt(a448, w448, L.EPI_BIAS, bias=c['bias'], scale_cols=N // 3, scale=0.125)
            few = ops.gemm_nt(a8, w8, L.EPI_BIAS, bias=c['bias'][:512], scale_cols=512 // 3, scale=0.125)
        torch.cuda.synchronize()
        assert_bits_equal(pool, snap, 'the pool after three launches the queue does not take')
        _queued(pool, 1, c, 'res', 8)                             # ... and none of them took a slot
    _check_epilogues(K, c['p64'], c['ap64'], None, c['r'], {'dgelu': dg})
    p64, ap64 = _prod64(a448, w448)
    _check_epilogues(448, p64, ap64, c['bias'], None, {'bias': (short, N // 3)})
    _check_epilogues(K, c['p64'][:, :512], c['ap64'][:, :512], c['bias'][:512], None, {'bias': (few, 512 // 3)})


def _on(stream, c, name):
    """The launch on another stream, ordered behind the current one; both are idle afterwards."""
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        got = _launch(c, name)
    stream.synchronize()
    torch.cuda.current_stream().synchronize()
    return got


def test_a_foreign_stream_takes_the_static_schedule():
    c = _case(*A_SHAPE)
    other = torch.cuda.Stream()
    with gemm_schedule(grid=8, queue_slots=4) as pool:
        assert _reduced(8)
        _verify(c, 'gelu', _queued(pool, 0, c, 'gelu', 8), 'the stream the ring binds to')
        snap = pool.clone()
        foreign = _on(other, c, 'gelu')
        assert_bits_equal(pool, snap, 'the pool after a launch on another stream')
        _verify(c, 'gelu', foreign, 'another stream')
        _verify(c, 'gelu', _queued(pool, 1, c, 'gelu', 8), 'the first stream again')


def test_arming_again_starts_at_slot_0_on_the_stream_of_that_time():
    c = _case(*B_SHAPE)
    other = torch.cuda.Stream()
    with gemm_schedule(grid=8, queue_slots=4) as pool:
        assert _reduced(8)
        _queued(pool, 0, c, 'res', 8)
        _queued(pool, 1, c, 'res', 8)
    with gemm_schedule(grid=8, queue_slots=4) as pool:
        assert _reduced(8) and not bool(pool.any())
        first = _queued(pool, 0, c, 'drop_res', 8, launch=lambda: _on(other, c, 'drop_res'))      # binds the ring to `other`
        snap = pool.clone()
        here = _launch(c, 'drop_res')                             # the default stream is the foreign one now
        torch.cuda.synchronize()
        assert_bits_equal(pool, snap, 'the pool after a launch on the stream the first ring was bound to')
        second = _queued(pool, 1, c, 'drop_res', 8, launch=lambda: _on(other, c, 'drop_res'))
    for what, got in (('first', first), ('default stream', here), ('second', second)):
        _verify(c, 'drop_res', got, what)


# ---------------------------------------------------------------------------------------------------------------------
# D. Every persistent GEMM family under a reduced grid, the queue off: the bodies of the existing tests
# ---------------------------------------------------------------------------------------------------------------------
GRIDS = (8, 64, 'reserve8')


@contextlib.contextmanager
def _recorded(log):
    """Copies of what every ops.gemm_nt / gemm_nt_fp8 call of the block returned (and of out2), in call order."""
    real = {'gemm_nt': ops.gemm_nt, 'gemm_nt_fp8': ops.gemm_nt_fp8}

    def wrap(fn):
        def call(*args, **kw):
            out = fn(*args, **kw)
            log.append(out.clone())
            if kw.get('out2') is not None:
                log.append(kw['out2'].clone())
            return out
        return call
    with pytest.MonkeyPatch.context() as mp:
        for name, fn in real.items():
            mp.setattr(ops, name, wrap(fn))
        yield


NT_BODIES = {
    'four-wave, ragged 1280x640x64': (lambda: TG.test_gemm_nt_256x256_kernels(1280, 640, 64, 2), True),
    'eight-wave, ragged 1280x640x64': (lambda: TG.test_gemm_nt_256x256_kernels(1280, 640, 64, 6), True),
    'four-wave, ragged 1064x1000x128': (lambda: TG.test_gemm_nt_256x256_kernels(1024 + 40, 1000, 128, 2), True),
    'eight-wave, ragged 1064x1000x128': (lambda: TG.test_gemm_nt_256x256_kernels(1024 + 40, 1000, 128, 6), True),
    'four-wave 1024x768x3072': (lambda: TG.test_gemm_nt_256x256_kernels(1024, 768, 3072, 2), True),
    'eight-wave 1024x768x3072': (lambda: TG.test_gemm_nt_256x256_kernels(1024, 768, 3072, 6), True),
    'ring 2088x1000x128': (lambda: TG.test_gemm_nt_none_and_bias(2048 + 40, 1000, 128), False),
    'byte derivative and its dgrad': (lambda: TG.test_gelu_byte_derivative_and_its_dgrad(1024, 512, 64), True),
    'block statistics': (lambda: TG.test_projection_with_block_statistics_and_the_cross_entropy_from_them(1024, 1280, 1217, 128), False),
    '8-bit copies': (lambda: TF8.test_byte_epilogues_leave_the_8bit_copy_of_their_output(1024, 512, 64), False),
    'shifted exponential': (lambda: TSH.test_shifted_exponential_epilogue_every_element(1024, 512, 512, 64), False),
    'fp8 product 1024x768x768': (lambda: TF8.test_gemm_nt_fp8_vs_fp32_product_of_the_same_operands(1024, 768, 768, False), True),
}
_FULL_GRID = {}                 # body -> what its NT launches leave under the default schedule


def _run_nt_body(key):
    body, poisoned = NT_BODIES[key]            # (poisoned: the original runs under the poison_outputs fixture)
    log = []
    torch.manual_seed(1234)                    # (some bodies draw operands from the global generator: the same ones every run)
    with (poisoned_outputs() if poisoned else contextlib.nullcontext()), _recorded(log):
        body()
    torch.cuda.synchronize()
    return log


@pytest.mark.parametrize('g', GRIDS)
@pytest.mark.parametrize('key', list(NT_BODIES))
def test_nt_families_under_a_reduced_grid(key, g):
    """The existing test's own assertions with the grid reduced, and every NT output of it bit for bit what the full grid
    leaves (column sums and running maxima are gathered with atomics and are not compared)."""
    if key not in _FULL_GRID:
        _defaults_hold()
        _FULL_GRID[key] = _run_nt_body(key)
    with gemm_schedule(grid=_grid(g)):
        assert _reduced(g)
        got = _run_nt_body(key)
    want = _FULL_GRID[key]
    assert len(got) == len(want) and len(got) > 0
    for k, (a, b) in enumerate(zip(got, want)):
        assert_bits_equal(a, b, '%s at grid %s: output %d against the full grid' % (key, g, k))


def _tiles_plan(M, N, K, nwg):
    """The weight-gradient table (csrc/gemm.hip, wgrad_plan) for 16-byte aligned operands."""
    ntile = (N // 256) * (K // 256)
    if M % 64 == 0 and M >= 4096 and N % 256 == 0 and K % 256 == 0 and ntile >= 9:
        return L.KERN_WGRAD_W4_TILES if ntile > nwg else L.KERN_WGRAD_W4_CHUNKS
    return L.KERN_WGRAD_RING if M % 64 == 0 and M >= 4096 else L.KERN_WGRAD_128


WGRAD_SHAPES = [(8192, 768, 768),           # 9 tiles on 8 workgroups at grid 8
                (4160, 1024, 1024),         # 65 K-tiles: segments of unequal length
                (4288, 2304, 768),
                (4096, 1000, 72),           # the stream-K ring kernel
                (4096, 1536, 1536)]         # 36 tiles: whole tiles round-robin at grid 8


@pytest.mark.parametrize('g', GRIDS)
@pytest.mark.parametrize('M,N,K', WGRAD_SHAPES)
def test_wgrad_under_a_reduced_grid(M, N, K, g):
    """tests/test_gemm.py::test_gemm_wgrad with the grid reduced.  (With the switch to whole tiles at four tiles per workgroup,
    as it was first written, the one-segment-per-workgroup mode ran with more tiles than workgroups and left the tiles past
    the grid out: at grid 8 the ninth tile of 768 x 768 and tiles 8 .. 15 of 1024 x 1024 came back with a relative error
    of 1, the others at 6e-7.)"""
    with gemm_schedule(grid=_grid(g)):
        assert _reduced(g)
        assert _wgrad_plan(M, N, K) == _tiles_plan(M, N, K, _grid(g))
        if g == 8 and (M, N, K) in ((8192, 768, 768), (4096, 1536, 1536)):
            assert _wgrad_plan(M, N, K) == L.KERN_WGRAD_W4_TILES
        TG.test_gemm_wgrad(M, N, K)


SPLIT_BODIES = {
    'NN four-wave 256x256x4096': lambda: TG.test_gemm_nn_on_the_four_wave_kernel(256, 256, 4096),
    'NN stream-K 1000x130x640': lambda: TG.test_gemm_nn_streamk(1000, 130, 640, 601),
    'NT stream-K 1000x130x640': lambda: TG.test_gemm_nt_streamk(1000, 130, 640),
    'wgrad pair': lambda: TG.test_gemm_wgrad_pair(8192, 768, 768, 256, 512),
}


@pytest.mark.parametrize('g', GRIDS)
@pytest.mark.parametrize('key', list(SPLIT_BODIES))
def test_contraction_split_families_under_a_reduced_grid(key, g):
    """Bounds only: these split the contraction over the workgroups (workspace partials summed in slot order, or fp32 atomics),
    so the order of an element's partial sums follows the grid - like the weight gradients, also for the NN products."""
    with gemm_schedule(grid=_grid(g)):
        assert _reduced(g)
        SPLIT_BODIES[key]()


def _stored_into_zero(shapes):
    """The body of tests/test_gemm.py::test_gemm_wgrad_stored_into_a_zero_gradient at shapes of the caller's choice: a shape
    that plans whole tiles is stored (NaN underneath must not be read), any other quietly accumulates into zeros."""
    for M, N, K in shapes:
        stores = _wgrad_plan(M, N, K) == L.KERN_WGRAD_W4_TILES
        g = torch.Generator(device='cuda').manual_seed(N + K)
        dy = (torch.randn((M, N), device='cuda', generator=g) * 0.1).to(torch.bfloat16)
        x = torch.randn((M, K), device='cuda', generator=g).to(torch.bfloat16)
        stored = torch.full((N, K), float('nan'), device='cuda') if stores else torch.zeros((N, K), device='cuda')
        assert ops.gemm_wgrad(dy, x, stored, alpha=0.5, dw_is_zero=True, report_store=True) == stores
        added = torch.zeros((N, K), device='cuda')
        ops.gemm_wgrad(dy, x, added, alpha=0.5)
        assert torch.isfinite(stored).all()
        assert rel_l2(stored.double(), added.double()) < 1e-6
        ref = 0.5 * (dy.double().t() @ x.double())
        assert rel_l2(stored.double(), ref) < 1e-5
        assert_gemm_bound(stored, ref, 0.5 * (dy.double().abs().t() @ x.double().abs()), M, F32_OUT, what='wgrad stored into zero')


@pytest.mark.parametrize('g', GRIDS)
def test_wgrad_stored_into_a_zero_gradient_under_a_reduced_grid(g):
    """At the grid of eight reserved CUs the existing body as it is (its 1024-tile matrix is stored, 768 x 768 accumulates).  On 8
    and 64 workgroups that matrix would take tens of seconds: the same body at the smallest shapes those grids store - more
    tiles than workgroups - beside a four-tile shape, which no grid stores."""
    nwg = _grid(g)
    with gemm_schedule(grid=nwg):
        assert _reduced(g)
        if g == 'reserve8':
            assert _wgrad_plan(4096, 16384, 4096) == L.KERN_WGRAD_W4_TILES and _wgrad_plan(4096, 768, 768) == L.KERN_WGRAD_W4_CHUNKS
            TG.test_gemm_wgrad_stored_into_a_zero_gradient()
        else:
            big = (4096, 768, 768) if g == 8 else (4096, 2304, 2048)          # 9 tiles on 8 workgroups; 72 on 64
            assert _wgrad_plan(*big) == L.KERN_WGRAD_W4_TILES and _wgrad_plan(4096, 512, 512) == L.KERN_WGRAD_RING
            _stored_into_zero([big, (4096, 512, 512)])


@pytest.mark.parametrize('g', GRIDS)
def test_wgrad_group_under_a_reduced_grid(g):
    """The grouped launch places its tiles on the reduced grid's workgroups (tests/test_wgrad_group.py: its products, its
    placement check, its bound); a group of more tiles than workgroups is declined and writes nothing."""
    nwg = _grid(g)
    shapes = [(256, 256), (512, 768)]                         # 7 tiles: they fit a grid of 8
    tiles = [(N // 256, K // 256) for N, K in shapes]
    prods = TWG._shared(4096, shapes + [(768, 768)], 1.0)
    small, nine = prods[:2], prods[2]
    with gemm_schedule(grid=nwg):
        assert _reduced(g)
        TWG._check_place(tiles, nwg)
        assert ops.gemm_wgrad_group([p.item() for p in small])
        torch.cuda.synchronize()
        for k, p in enumerate(small):
            p.check('grid %d: item %d (%d x %d)' % (nwg, k, p.N, p.K))
        fits = nwg >= 9
        assert ops.gemm_wgrad_group([nine.item()]) == fits
        torch.cuda.synchronize()
        if fits:
            nine.check('grid %d: nine tiles' % nwg)
        else:
            nine.check_frame('nine tiles on eight workgroups: declined', dw_too=True)


# ---------------------------------------------------------------------------------------------------------------------
# E. Both switches, as data parallelism sets them with M3P_DP_RESERVE_CUS=8 and M3P_DP_TILE_QUEUE=1
# ---------------------------------------------------------------------------------------------------------------------
def test_queue_on_the_grid_that_leaves_eight_cus_free():
    _queue_case('reserve8', (4352, 4096, 512))


def test_the_switches_are_back_at_their_defaults():
    """Keep this the last test of the module: nothing above leaves a switch set."""
    _defaults_hold()
