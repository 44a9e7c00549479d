"""LAMB and the cosine schedule on the host: the optimizer spec names, the schedule against values recorded from the
reference's own class, the torch loop that steps parameters outside any arena against an fp64 restatement of the rule in
include/m3p_hip.h, and the host half of the kernels' piece table (no GPU here)."""
import math
import os

import numpy as np
import pytest
import torch

from m3p_amd import optim as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 2.0 ** -24


def _params():
    return [torch.nn.Parameter(torch.zeros(4, 3)), torch.nn.Parameter(torch.zeros(5))]


# ---- get_optimizer ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('spec,cls', [
    ('lamb,lr=0.002,weight_decay=0.01', 'Lamb'),
    ('lamb_inverse_sqrt,lr=0.002,weight_decay=0.01,beta1=0.9,beta2=0.98,warmup_updates=10', 'LambInverseSqrtWithWarmup'),
    ('lamb_cosine,lr=0.002,weight_decay=0.01,init_period=100,period_mult=2', 'LambCosineWithWarmup'),
    ('adam_cosine,lr=0.0001,beta1=0.9,beta2=0.98,init_period=100', 'AdamCosineWithWarmup'),
])
def test_spec_names_the_new_classes(spec, cls):
    opt = O.get_optimizer(_params(), spec)
    assert type(opt) is getattr(O, cls)
    assert isinstance(opt, O.Adam) and isinstance(opt, O.Lamb) == cls.startswith('Lamb')
    if 'beta2=0.98' in spec:
        assert opt.param_groups[0]['betas'] == (0.9, 0.98)
    if cls != 'Lamb':
        # built at the floor rate, one counted update per step, lr moved along the curve: what reload_checkpoint relies on
        g = opt.param_groups[0]
        assert g['num_updates'] == 0 and g['lr'] == 1e-7 == opt.get_lr_for_step(0)
        opt.step()
        assert g['num_updates'] == 1 and g['lr'] == opt.get_lr_for_step(1)
    else:
        assert opt.param_groups[0]['lr'] == 0.002 and opt.param_groups[0]['weight_decay'] == 0.01


def test_lamb_defaults_and_exclude_1d_option():
    opt = O.get_optimizer(_params(), 'lamb')
    g = opt.param_groups[0]
    assert (g['eps'], g['weight_decay'], opt.exclude_1d) == (1e-6, 0.01, True)
    assert O.get_optimizer(_params(), 'lamb,exclude_1d=0').exclude_1d is False
    assert O.get_optimizer(_params(), 'lamb_cosine,exclude_1d=1').exclude_1d is True


def test_unknown_lamb_option_raises():
    with pytest.raises(Exception, match='Unexpected parameters'):
        O.get_optimizer(_params(), 'lamb,foo=1')
    with pytest.raises(Exception, match='Unexpected parameters'):
        O.get_optimizer(_params(), 'lamb,exp_factor=0.5')          # a schedule's option on the unscheduled class
    with pytest.raises(Exception, match='Unknown optimization method'):
        O.get_optimizer(_params(), 'lars,lr=0.1')


def test_inverse_sqrt_class_keeps_its_attributes():
    opt = O.AdamInverseSqrtWithWarmup(_params(), lr=1e-4, warmup_updates=10)
    assert opt.schedule == dict(peak_lr=1e-4, warmup=10, floor_lr=1e-7, power=0.5)
    assert opt.get_lr_for_step(10) == 1e-4 and opt.get_lr_for_step(40) == 1e-4 * 0.5
    lamb = O.LambInverseSqrtWithWarmup(_params(), lr=1e-4, warmup_updates=10)
    assert [lamb.get_lr_for_step(t) for t in (0, 3, 10, 40)] == [opt.get_lr_for_step(t) for t in (0, 3, 10, 40)]


# ---- the cosine schedule ---------------------------------------------------------------------------------------------
def test_cosine_schedule_matches_the_reference_class():
    """tests/golden/adam_cosine_lr.npz holds update counts and the rates the reference's AdamCosineWithWarmup
    (M3P/src/optim.py:142-209) returns for them, for two settings (a: period_mult = 1; b: period_mult = 2, lr_shrink = 0.75):
    below warm-up, at warm-up, at mid-period, around the period borders and three periods in.  Recorded once with
        o = AdamCosineWithWarmup([torch.nn.Parameter(torch.zeros(3))], **settings);  [o.get_lr_for_step(s) for s in steps]
    on a CPU parameter.  The schedule here walks the periods instead of inverting their geometric sum; both evaluate one
    cosine of the same argument in double precision and differ by a few ulps (1e-16 relative) at most: rtol 1e-12."""
    gold = np.load(os.path.join(ROOT, 'tests', 'golden', 'adam_cosine_lr.npz'))
    for tag in 'ab':
        kw = {k: float(gold['%s_%s' % (k, tag)]) for k in ('lr', 'warmup_updates', 'warmup_init_lr', 'min_lr', 'init_period',
                                                           'period_mult', 'lr_shrink')}
        steps, rates = gold['steps_' + tag], gold['rates_' + tag]
        assert len(steps) >= 10 and steps[0] < kw['warmup_updates'] < steps[-1]
        for cls in (O.AdamCosineWithWarmup, O.LambCosineWithWarmup):
            opt = cls(_params(), **kw)
            got = np.array([opt.get_lr_for_step(int(s)) for s in steps])
            np.testing.assert_allclose(got, rates, rtol=1e-12, atol=0, err_msg='%s, setting %s' % (cls.__name__, tag))
    # a period border is where the rate jumps back up, shrunk: the recorded points straddle one
    a = dict(zip(gold['steps_a'].tolist(), gold['rates_a'].tolist()))
    assert a[1099] < 1e-8 and abs(a[1100] - 0.75e-3) < 1e-12
    # many equal periods in: one division, not a walk; periods that shrink would end after finitely many updates
    far = O.AdamCosineWithWarmup(_params(), lr=1e-3, warmup_updates=10, init_period=7, lr_shrink=1.0)
    assert abs(far.get_lr_for_step(10 + 7 * 10 ** 9) - 1e-3) < 1e-15
    with pytest.raises(ValueError, match='period_mult'):
        O.AdamCosineWithWarmup(_params(), period_mult=0.5)


# ---- the torch loop against the rule in fp64 ----------------------------------------------------------------------------
def _lamb_numpy(state, grads, hp, steps, max_norm):
    """Section "LAMB on the flat arenas" of include/m3p_hip.h in NumPy fp64.  state: name -> dict(p, m, v, step, ndim)."""
    b1, b2, eps, lr, wd = hp['beta1'], hp['beta2'], hp['eps'], hp['lr'], hp['weight_decay']
    for _ in range(steps):
        live = [n for n in state if grads[n] is not None]
        coef = 1.0
        if max_norm > 0:
            norm = math.sqrt(sum(float((grads[n] ** 2).sum()) for n in live))
            coef = min(1.0, max_norm / (norm + 1e-6))
        for n in live:
            s = state[n]
            g = coef * grads[n]
            s['step'] += 1
            s['m'] = b1 * s['m'] + (1 - b1) * g
            s['v'] = b2 * s['v'] + (1 - b2) * g * g
            plain = hp['exclude_1d'] and s['ndim'] < 2
            r = (s['m'] / (1 - b1 ** s['step'])) / (np.sqrt(s['v'] / (1 - b2 ** s['step'])) + eps) + (0.0 if plain else wd) * s['p']
            pn, rn = np.sqrt((s['p'] ** 2).sum()), np.sqrt((r ** 2).sum())
            phi = pn / rn if (not plain and pn > 0 and rn > 0) else 1.0
            s['phi'] = phi
            s['p'] = s['p'] - lr * phi * r


@pytest.mark.parametrize('exclude_1d', [True, False])
@pytest.mark.parametrize('max_norm', [0.0, 0.5])
def test_torch_loop_follows_the_rule(exclude_1d, max_norm):
    rs = np.random.RandomState(5)
    shapes = dict(w=(12, 7), b=(9,), z=(6, 5), idle=(4, 4))
    init = {n: rs.standard_normal(s).astype(np.float32) for n, s in shapes.items()}
    init['z'][:] = 0                                              # zero weights: phi = 1
    init['w'] *= 3                                                # |r| is about 1 per element: phi is about 3 here
    init['b'] *= 0.25                                             # and about 1/4 here, when it applies
    grads = {n: rs.standard_normal(s).astype(np.float32) for n, s in shapes.items()}
    grads['idle'] = None                                          # never receives a gradient
    hp = dict(beta1=0.9, beta2=0.98, eps=1e-6, lr=0.01, weight_decay=0.05, exclude_1d=exclude_1d)
    params = {n: torch.nn.Parameter(torch.from_numpy(init[n].copy())) for n in shapes}
    opt = O.Lamb(list(params.values()), lr=hp['lr'], betas=(hp['beta1'], hp['beta2']), eps=hp['eps'],
                 weight_decay=hp['weight_decay'], exclude_1d=exclude_1d)
    for _ in range(3):
        for n, p in params.items():
            p.grad = None if grads[n] is None else torch.from_numpy(grads[n].copy())
        if max_norm > 0:
            opt.clip_grad_norm(max_norm)
        opt.step()
    ref = {n: dict(p=init[n].astype(np.float64), m=np.zeros(shapes[n]), v=np.zeros(shapes[n]), step=0, ndim=len(shapes[n]))
           for n in shapes}
    _lamb_numpy(ref, {n: None if g is None else g.astype(np.float64) for n, g in grads.items()}, hp, 3, max_norm)
    if max_norm > 0:
        assert math.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in grads.values() if g is not None)) > max_norm   # the clip bites
    # fp32 rounding: each of the three steps rounds m, v, r and p a handful of times relative to their own size
    # (|p| <= ~4, |lr phi r| <= lr |p|-ish), 64 u of the largest magnitude in play is ample and far below any rule error
    for n, p in params.items():
        st = opt.state[p]
        assert st['step'] == ref[n]['step'] == (0 if n == 'idle' else 3)
        for got, want in ((p.data, ref[n]['p']), (st['exp_avg'], ref[n]['m']), (st['exp_avg_sq'], ref[n]['v'])):
            tol = 64 * U32 * max(1.0, float(np.abs(want).max()))
            assert float(np.abs(got.double().numpy() - want).max()) <= tol, n
    assert np.array_equal(params['idle'].data.numpy(), init['idle'])
    assert torch.equal(opt.state[params['idle']]['exp_avg'], torch.zeros(4, 4))
    assert ref['z']['step'] == 3 and float(np.abs(ref['z']['p']).max()) > 0
    # the trust ratio did something: an adapted 2-d tensor's factor is far from 1, the 1-d tensor's is 1 when excluded
    assert abs(ref['w']['phi'] - 1.0) > 0.1
    assert (ref['b']['phi'] == 1.0) == exclude_1d


# ---- the piece table's host half ---------------------------------------------------------------------------------------
def test_piece_table_layout_and_refusals():
    from m3p_amd import lib as L, ops
    pieces = [(0, 64, 0, 1, 0), (64, 1024, 1, 1, 0), (1024, 1536, 1, 0, 1), (2048, 2048 + 4 * 256 * 40, 3, 1, 1)]
    t = ops.LambTable(pieces, n_tensors=4, n_classes=2, arena_elems=1 << 20)
    assert t.n_pieces == 4 and t.blk0[0] == 0 and t.blk0[-1] == t.n_blocks
    assert all(b > a for a, b in zip(t.blk0, t.blk0[1:]))                    # every piece has a workgroup
    # tensor 1 owns the workgroups of pieces 1 and 2; tensor 2 has no piece: an empty run in its place
    assert t.tensor_blk0 == [t.blk0[0], t.blk0[1], t.blk0[3], t.blk0[3], t.n_blocks]
    assert t.n_blocks == 1 + 1 + 1 + 40 and t.quads_per_thread() == [1, 1, 1, 1]
    capped = ops.LambTable(pieces, 4, 2, 1 << 20, max_blocks=8)
    assert capped.n_blocks <= 8 + 3 and max(capped.quads_per_thread()) >= 5
    for bad in ([(0, 62, 0, 1, 0)],                                          # border off the quad grid
                [(2, 66, 0, 1, 0)],
                [(0, 64, 0, 1, 0), (32, 128, 1, 1, 0)],                      # overlap
                [(64, 128, 1, 1, 0), (128, 256, 0, 1, 0)],                   # a tensor's pieces not adjacent / out of order
                [(0, 64, 4, 1, 0)],                                          # tensor id past the table
                [(0, 64, 0, 1, 2)],                                          # class past the classes
                [(0, (1 << 20) + 64, 0, 1, 0)],                              # past the arena
                [(64, 64, 0, 1, 0)]):                                        # empty
        with pytest.raises(L.M3PError, match='M3P_EINVAL'):
            ops.LambTable(bad, 4, 2, 1 << 20)
    with pytest.raises(L.M3PError, match='M3P_EINVAL'):
        ops.LambTable(pieces, 4, ops.LAMB_MAX_CLASSES + 1, 1 << 20)
