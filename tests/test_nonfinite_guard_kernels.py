"""Kernels of the non-finite guard (csrc/optim.hip; the contract in include/m3p_hip.h): m3p_step_guard's decision, rings and
counters, and the _guarded forms of the Adam and LAMB launches - on a skipped step nothing but the flagged gradient pieces
changes by a bit (sentinels between the pieces included), with skip = 0 or NULL every output is bit-equal to the existing
entry point's.  Non-finite values sit in gradients and in the reduced sums only: arithmetic on them, no control flow."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from m3p_amd import lib as L, ops

from tests.test_lamb_kernels import CLASSES, HP, PLAIN, Synthetic
from tests.util import assert_bits_equal, assert_exact_zero

pytestmark = pytest.mark.gpu

INF, NAN = float('inf'), float('nan')


# ---- m3p_step_guard ------------------------------------------------------------------------------------------------
def _scalar(x):
    return torch.tensor([x], dtype=torch.float64, device='cuda')


def _attempt(guard, sums, attempt, grad_scale=0.5):
    ops.step_guard([_scalar(s) for s in sums], grad_scale, attempt, guard)
    torch.cuda.synchronize()
    counters, norms, ring = guard.read()
    return int(guard.skip.item()), counters, norms, ring


def _norm_ok(got, sums, grad_scale=0.5):
    ref = math.sqrt(sum(sums)) * grad_scale
    return got == ref or abs(got - ref) <= 2.0 ** -51 * ref        # two roundings of a double (root, product)


@pytest.mark.parametrize('s, skip', [(0.0, 0), (1.0, 0), (1e80, 0), (INF, 1), (-INF, 1), (NAN, 1)])
def test_guard_decides_on_one_sum(s, skip):
    guard = ops.StepGuard('cuda')
    got, counters, norms, ring = _attempt(guard, [s], 0)
    assert got == skip and ring[0] == skip and counters == [1, skip, skip]
    if skip:
        assert not math.isfinite(norms[0])
    else:
        assert _norm_ok(norms[0], [s]), (norms[0], s)
    assert ring[1:] == [0] * 63 and norms[1:] == [0.0] * 63


@pytest.mark.parametrize('sums, skip', [([2.0, 7.0], 0), ([2.0, NAN], 1), ([INF, 7.0], 1), ([1e300, 1e300], 0), ([3.0] * 8, 0)])
def test_guard_decides_on_several_sums(sums, skip):
    """One bad sum of several skips.  Two finite sums whose total overflows do NOT skip (the rule reads the sums, each finite
    as a double) - the reported norm is then infinite."""
    guard = ops.StepGuard('cuda')
    got, counters, norms, ring = _attempt(guard, sums, 5)
    assert got == skip and ring[5] == skip and counters == [1, skip, skip]
    if skip == 0 and math.isfinite(sum(sums)):
        assert _norm_ok(norms[5], sums)
    else:
        assert not math.isfinite(norms[5])


def test_guard_takes_a_fixed_number_of_arenas():
    guard = ops.StepGuard('cuda')
    with pytest.raises(L.M3PError, match='M3P_ENOTIMPL'):
        ops.step_guard([_scalar(1.0)] * (ops.StepGuard.MAX_ARENAS + 1), 1.0, 0, guard)
    with pytest.raises(L.M3PError, match='M3P_EINVAL'):
        ops.step_guard([], 1.0, 0, guard)
    torch.cuda.synchronize()
    assert guard.read()[0] == [0, 0, 0]


def test_guard_ring_wraps_at_64():
    guard = ops.StepGuard('cuda')
    _attempt(guard, [NAN], 0)
    got, counters, norms, ring = _attempt(guard, [4.0], 63, grad_scale=1.0)
    assert ring[0] == 1 and ring[63] == 0 and norms[63] == 2.0 and counters == [2, 1, 0]
    got, counters, norms, ring = _attempt(guard, [9.0], 64, grad_scale=1.0)         # slot 0 again
    assert got == 0 and ring[0] == 0 and norms[0] == 3.0 and ring[63] == 0 and norms[63] == 2.0 and counters == [3, 1, 0]


def test_guard_counts_ok_bad_bad_ok():
    guard = ops.StepGuard('cuda')
    seen = []
    for attempt, s in enumerate([16.0, INF, NAN, 25.0]):
        got, counters, norms, ring = _attempt(guard, [s], attempt, grad_scale=1.0)
        seen.append((got, counters))
    assert seen == [(0, [1, 0, 0]), (1, [2, 1, 1]), (1, [3, 2, 2]), (0, [4, 2, 0])]
    assert ring[:5] == [0, 1, 1, 0, 0]
    assert norms[0] == 4.0 and norms[1] == INF and math.isnan(norms[2]) and norms[3] == 5.0


# ---- guarded Adam --------------------------------------------------------------------------------------------------
GAP = 64
ADAM_HP = dict(lr=1e-3, beta1=0.9, beta2=0.98, eps=1e-8, weight_decay=0.01, max_norm=1.0, grad_scale=0.5)
# 4 elements; 2052 = one quad past 256 threads x 2 quads; ~1 M at a start that is no multiple of 1024: several workgroups
SIZES = (4, 2052, (1 << 20) + 12)


class AdamArena:
    def __init__(self, zero_flags, seed=3):
        rs = np.random.RandomState(seed)
        self.pieces, off = [], GAP
        for n, z, step in zip(SIZES, zero_flags, (1e-3, 2e-3, 5e-4)):
            self.pieces.append((off, off + n, step, z))
            off += n + GAP
        assert self.pieces[2][0] % 1024 != 0
        self.total = off
        host = {k: rs.standard_normal(off).astype(np.float32) for k in 'pgm'}
        host['v'] = rs.standard_normal(off).astype(np.float32) ** 2
        inside = torch.zeros(off, dtype=torch.bool)
        for a, b, _, _ in self.pieces:
            inside[a:b] = True
            for k, val in ((0, NAN), (1, INF), (b - a - 1, -INF), ((b - a) // 2, NAN)):
                host['g'][a + k] = val
        self.inside = inside.cuda()
        self.before = {k: torch.from_numpy(x).cuda() for k, x in host.items()}
        nanbits = torch.tensor(0x7fc12345, dtype=torch.int32, device='cuda')              # a NaN with a payload of its own
        self.before['g'].view(torch.int32)[self.pieces[1][0] + 8] = nanbits
        for x in self.before.values():
            x.view(torch.int32)[~self.inside] = -1
        self.before['w'] = torch.full((off,), NAN, dtype=torch.bfloat16, device='cuda')
        self.gnorm = _scalar(9.0)

    def run(self, how, skip=None, w16=True):
        """how = 'plain': the existing entry point; 'guarded': m3p_adam_step_ranges_guarded with `skip` (a tensor, or None = NULL)."""
        s = {k: x.clone() for k, x in self.before.items()}
        n = len(self.pieces)
        args = [s['p'].data_ptr(), s['g'].data_ptr(), s['m'].data_ptr(), s['v'].data_ptr(), s['w'].data_ptr() if w16 else None,
                (C.c_longlong * n)(*[a for a, _, _, _ in self.pieces]), (C.c_longlong * n)(*[b - a for a, b, _, _ in self.pieces]),
                (C.c_float * n)(*[st for _, _, st, _ in self.pieces]), (C.c_int * n)(*[z for _, _, _, z in self.pieces]), n,
                ADAM_HP['lr'], ADAM_HP['beta1'], ADAM_HP['beta2'], ADAM_HP['eps'], ADAM_HP['weight_decay'], self.gnorm.data_ptr(),
                ADAM_HP['max_norm'], ADAM_HP['grad_scale']]
        if how == 'plain':
            L.check(L.load().m3p_adam_step_ranges(*args, L.stream()), 'm3p_adam_step_ranges')
        else:
            L.check(L.load().m3p_adam_step_ranges_guarded(*args, None if skip is None else skip.data_ptr(), L.stream()), 'guarded')
        torch.cuda.synchronize()
        return s


def _flag(v):
    return torch.tensor([v], dtype=torch.int32, device='cuda')


@pytest.fixture(scope='module', params=[(1, 0, 1), (0, 1, 0)], ids=['zero-keep-zero', 'keep-zero-keep'])
def adam_arena(request):
    return AdamArena(request.param)


@pytest.mark.parametrize('w16', [True, False], ids=['w16', 'no-w16'])
def test_adam_skipped_step_changes_only_the_flagged_gradients(adam_arena, w16):
    ar = adam_arena
    after = ar.run('guarded', _flag(1), w16=w16)
    for c in 'pmvw':
        assert_bits_equal(after[c], ar.before[c], 'skipped step: ' + c)
    keep = torch.ones(ar.total, dtype=torch.bool, device='cuda')
    for a, b, _, z in ar.pieces:
        if z:
            assert_exact_zero(after['g'][a:b], 'gradient of the flagged piece [%d, %d)' % (a, b))
            keep[a:b] = False
    assert_bits_equal(after['g'][keep], ar.before['g'][keep], 'gradients outside the flagged pieces (NaN payloads included)')
    assert bool(torch.isnan(after['g'][keep]).any()) == (not all(z for *_, z in ar.pieces))


@pytest.mark.parametrize('w16', [True, False], ids=['w16', 'no-w16'])
@pytest.mark.parametrize('skip', ['zero', 'null'])
def test_adam_unskipped_step_is_the_existing_entry_point_bit_for_bit(adam_arena, skip, w16):
    ar = adam_arena
    ref = ar.run('plain', w16=w16)
    got = ar.run('guarded', _flag(0) if skip == 'zero' else None, w16=w16)
    for c in 'pgmvw':
        assert_bits_equal(got[c], ref[c], 'skip = %s: %s' % (skip, c))
    out = ~ar.inside
    for c in 'pgmvw':
        assert_bits_equal(ref[c][out], ar.before[c][out], 'sentinels of ' + c)
    a, b, _, _ = ar.pieces[2]
    moved = ref['p'][a + 2:b - 1] != ar.before['p'][a + 2:b - 1]
    assert int(moved.sum()) > (b - a) // 2, 'the reference run did not update the big piece'
    if not w16:
        assert_bits_equal(ref['w'], ar.before['w'], 'w16 = NULL: the bf16 copy')


def test_adam_guarded_refuses_a_misaligned_skip(adam_arena):
    ar = adam_arena
    two = torch.zeros(8, dtype=torch.uint8, device='cuda')
    with pytest.raises(L.M3PError, match='M3P_EINVAL'):
        ar.run('guarded', two[1:5])


# ---- guarded LAMB --------------------------------------------------------------------------------------------------
class LambRun:
    """tests.test_lamb_kernels.Synthetic (40-odd tensors: 1-d excluded ones, single-workgroup ones, one over several
    workgroups, pieces that keep r) driven through either set of entry points."""

    def __init__(self):
        self.syn = Synthetic()
        self.poisoned = {k: x.clone() for k, x in self.syn.before.items()}
        for a, b, *_ in self.syn.pieces:                   # non-finite gradients in every piece
            self.poisoned['g'][a] = NAN
            self.poisoned['g'][b - 1] = INF

    def launch(self, s, which, skip, guarded=True):
        syn, t = self.syn, self.syn.table
        lib = L.load()
        sk = () if not guarded else (None if skip is None else skip.data_ptr(),)
        rbc1, rbc2, wd, adapt = ops._lamb_classes(CLASSES, t.n_classes)
        if which == 'update':
            f = lib.m3p_lamb_update_guarded if guarded else lib.m3p_lamb_update
            rc = f(s['p'].data_ptr(), s['g'].data_ptr(), s['m'].data_ptr(), s['v'].data_ptr(), t.dev_pieces.data_ptr(), t.n_pieces, t.n_blocks,
                   rbc1, rbc2, wd, adapt, t.n_classes, HP['beta1'], HP['beta2'], HP['eps'], syn.gnorm.data_ptr(), HP['max_norm'],
                   HP['grad_scale'], t.partials.data_ptr(), *sk, L.stream())
        elif which == 'norms':
            f = lib.m3p_lamb_norms_guarded if guarded else lib.m3p_lamb_norms
            rc = f(t.partials.data_ptr(), t.dev_tblk.data_ptr(), t.n_tensors, t.norms.data_ptr(), *sk, L.stream())
        else:
            f = lib.m3p_lamb_apply_guarded if guarded else lib.m3p_lamb_apply
            rc = f(s['p'].data_ptr(), s['g'].data_ptr(), s['w'].data_ptr(), t.dev_pieces.data_ptr(), t.n_pieces, t.n_blocks,
                   t.norms.data_ptr(), adapt, t.n_classes, HP['lr'], *sk, L.stream())
        L.check(rc, which)

    def step(self, before, skip, guarded=True):
        s = {k: x.clone() for k, x in before.items()}
        for which in ('update', 'norms', 'apply'):
            self.launch(s, which, skip, guarded)
        torch.cuda.synchronize()
        s['norms'] = self.syn.table.norms.clone()
        return s


@pytest.fixture(scope='module')
def lamb():
    return LambRun()


def test_lamb_table_has_the_cases(lamb):
    syn = lamb.syn
    assert len(syn.tensors) >= 3 and any(t['cls'] == PLAIN and t['n'] < 256 for t in syn.tensors)
    t = syn.table
    per_piece = [b1 - b0 for b0, b1 in zip(t.blk0, t.blk0[1:])]
    assert min(per_piece) == 1 and max(per_piece) >= 8
    assert {z for *_, z, _ in syn.pieces} == {0, 1}


def test_lamb_skipped_step_changes_only_the_flagged_gradients(lamb):
    syn, t = lamb.syn, lamb.syn.table
    t.partials.fill_(-3.0)
    t.norms.fill_(-5.0)
    after = lamb.step(lamb.poisoned, _flag(1))
    for c in 'pmvw':
        assert_bits_equal(after[c], lamb.poisoned[c], 'skipped step: ' + c)
    assert bool((t.partials == -3.0).all()) and bool((after['norms'] == -5.0).all()), 'a skipped step wrote partials or norms'
    keep = torch.ones(syn.total, dtype=torch.bool, device='cuda')
    for a, b, _, z, _ in syn.pieces:
        if z:
            assert_exact_zero(after['g'][a:b], 'gradient of the flagged piece [%d, %d)' % (a, b))
            keep[a:b] = False
    assert_bits_equal(after['g'][keep], lamb.poisoned['g'][keep], 'gradients outside the flagged pieces')
    assert bool(torch.isnan(after['g'][keep & syn.inside]).any())


@pytest.mark.parametrize('which', ['update', 'norms', 'apply'])
def test_lamb_each_launch_alone_leaves_the_arenas(lamb, which):
    """Whichever of the three launches the flag reaches: master, moments and the bf16 copy stay; update and norms store nothing
    at all, apply the zeros."""
    syn, t = lamb.syn, lamb.syn.table
    t.partials.fill_(-3.0)
    t.norms.fill_(-5.0)
    s = {k: x.clone() for k, x in lamb.poisoned.items()}
    lamb.launch(s, which, _flag(1))
    torch.cuda.synchronize()
    for c in 'pmvw' + ('' if which == 'apply' else 'g'):
        assert_bits_equal(s[c], lamb.poisoned[c], '%s alone, skipped: %s' % (which, c))
    assert bool((t.partials == -3.0).all()) and bool((t.norms == -5.0).all())
    if which == 'apply':
        for a, b, _, z, _ in syn.pieces:
            if z:
                assert_exact_zero(s['g'][a:b], 'piece [%d, %d)' % (a, b))
            else:
                assert_bits_equal(s['g'][a:b], lamb.poisoned['g'][a:b], 'kept piece [%d, %d)' % (a, b))


@pytest.mark.parametrize('skip', ['zero', 'null'])
def test_lamb_unskipped_step_is_the_existing_entry_points_bit_for_bit(lamb, skip):
    syn = lamb.syn
    ref = lamb.step(syn.before, None, guarded=False)
    flag = _flag(0) if skip == 'zero' else None
    got = lamb.step(syn.before, flag)
    again = lamb.step(syn.before, flag)
    for c in ('p', 'g', 'm', 'v', 'w', 'norms'):
        assert_bits_equal(got[c], ref[c], 'skip = %s: %s' % (skip, c))
        assert_bits_equal(again[c], ref[c], 'skip = %s, repeated: %s' % (skip, c))
    assert bool((ref['p'][syn.inside] != syn.before['p'][syn.inside]).any())
    # and on the poisoned gradients: the same NaNs in the same places
    ref = lamb.step(lamb.poisoned, None, guarded=False)
    got = lamb.step(lamb.poisoned, flag)
    for c in ('p', 'g', 'm', 'v', 'w', 'norms'):
        assert_bits_equal(got[c], ref[c], 'poisoned gradients, skip = %s: %s' % (skip, c))
