"""The three LAMB launches (csrc/optim.hip: lamb_update_kernel, lamb_norms_kernel, lamb_apply_kernel; the rule in
include/m3p_hip.h) on a synthetic arena against the rule in fp64, every element within a bound counted from the kernels'
operations, in the manner of util.adam_ref64 / util.sumsq_bound.

With u = 2^-24, per element (gc = coef g, A_m = |beta1 m| + |(1 - beta1) gc| as in adam_ref64):
  m, v   Adam's own roundings: ADAM_M_U u A_m and ADAM_V_U u v_ref (the same statements as adam_kernel's).
  r      r = (m rbc1) / (sqrtf(v rbc2) + eps) + wd p.  The quotient inherits m's 8 u A_m (scaled by rbc1 / den) and rounds at the
         product with rbc1 (1), in the denominator (v's 12 u and the product's 1 halve through the square root: 6.5; the
         correctly rounded sqrtf 1; the sum with eps 1 - all relative to den, and |m| <= A_m) and at the division (1); the
         closing sum rounds once relative to |quotient| + |wd p| (1):  LAMB_T_U = 8 + 1 + 6.5 + 1 + 1 + 1 + 1 = 19.5 -> 20
         on A_m rbc1 / den, and LAMB_W_U = 2 (product, sum) on |wd p|.  Contraction to FMA only removes roundings.
  norms  one thread adds t quads into each running sum: (t + 8) u relative, sumsq_bound's count (squares and sums inside a
         quad, the butterfly across the wave); the workgroups' pairs meet in fp64.  sum r^2 also carries what r itself is off by:
         d = 2 sum |r| r_bound + sum r_bound^2.
  phi    sqrt(PP / RR) in fp64 halves the two relative errors; rounded to fp32 once (1).
  p      p - (lr phi) r: the product lr phi (1), the product with r (1) and the difference (1, relative to |p| + |lr phi r|):
         |p - ref| <= u |p| + (|s r| + s r_bound) (eps_phi + 3 u) + s r_bound,   s = lr phi,
         eps_phi = (e_PP / PP + e_RR / RR) / 2 + u   (0 where phi is 1 by rule).
The bf16 working copy is the rounding of the p the kernel wrote: bit-equal to that p cast.  The worst ratios are printed."""
import math

import numpy as np
import pytest
import torch

from m3p_amd import lib as L, ops

from tests.util import ADAM_M_U, ADAM_V_U, U32, _f32, assert_bits_equal, assert_exact_zero

pytestmark = pytest.mark.gpu

LAMB_T_U, LAMB_W_U = 20.0, 2.0
HP = dict(lr=0.01, beta1=0.9, beta2=0.98, eps=1e-6, max_norm=100.0, grad_scale=0.5)
WD = 0.05
# classes of one launch: (step count, wd_t, adapt_t) -> (rbc1, rbc2, wd_t, adapt_t)
STEPS = (2, 2, 5)
CLASSES = [(1.0 / (1 - HP['beta1'] ** s), 1.0 / (1 - HP['beta2'] ** s), wd, ad)
           for s, (wd, ad) in zip(STEPS, ((WD, True), (0.0, False), (0.0, True)))]
ADAPT, PLAIN, NODECAY = 0, 1, 2
GAP = 64                  # guard elements between tensors
MAX_BLOCKS = 64           # the launches' workgroup cap here: the big tensor's threads then make two trips


def lamb_ref64(p, g, m, v, cls, hp, t, foreign=(0.0, 0.0)):
    """One tensor's LAMB step in fp64 from fp32 state (the elements this rank owns, concatenated) and the fp32 values of the
    scalars.  cls = (rbc1, rbc2, wd_t, adapt_t); hp: lr, beta1, beta2, eps, max_norm, grad_scale, gnorm_sq; t = the most quads
    one thread adds; foreign = the other ranks' (sum p^2, sum r^2).  -> dict of references and bounds (module docstring)."""
    b1, b2, eps, lr = _f32(hp['beta1']), _f32(hp['beta2']), _f32(hp['eps']), _f32(hp['lr'])
    rbc1, rbc2, wd, adapt = _f32(cls[0]), _f32(cls[1]), _f32(cls[2]), bool(cls[3])
    gs = _f32(hp['grad_scale']) or 1.0
    coef = gs
    if hp.get('gnorm_sq') is not None and hp['max_norm'] > 0:
        coef *= min(_f32(hp['max_norm']) / (math.sqrt(float(hp['gnorm_sq'])) * gs + _f32(1e-6)), 1.0)
    p, g, m, v = (x.double() for x in (p, g, m, v))
    gc = g * coef
    a_m = (b1 * m).abs() + ((1.0 - b1) * gc).abs()
    m_ref = b1 * m + (1.0 - b1) * gc
    v_ref = b2 * v + (1.0 - b2) * gc * gc
    den = (v_ref * rbc2).sqrt() + eps
    r_ref = (m_ref * rbc1) / den + wd * p
    r_bound = U32 * (LAMB_T_U * a_m * rbc1 / den + LAMB_W_U * (wd * p).abs())
    pp, rr = float((p * p).sum()), float((r_ref * r_ref).sum())
    d = float((2 * r_ref.abs() * r_bound + r_bound * r_bound).sum())
    e_pp, e_rr = (t + 8) * U32 * pp, (t + 8) * U32 * (rr + d) + d
    PP, RR = pp + float(foreign[0]), rr + float(foreign[1])
    phi, eps_phi = 1.0, 0.0
    if adapt and PP > 0 and RR > 0:
        phi = math.sqrt(PP / RR)
        eps_phi = 0.5 * (e_pp / PP + e_rr / RR) + U32
    s = lr * phi
    p_ref = p - s * r_ref
    p_bound = U32 * p.abs() + ((s * r_ref).abs() + s * r_bound) * (eps_phi + 3 * U32) + s * r_bound
    return dict(p=p_ref, m=m_ref, v=v_ref, r=r_ref, p_bound=p_bound, m_bound=ADAM_M_U * U32 * a_m, v_bound=ADAM_V_U * U32 * v_ref,
                r_bound=r_bound, pp=pp, rr=rr, e_pp=e_pp, e_rr=e_rr, phi=phi)


def _ratio(got, ref, bound):
    """Largest |got - ref| / bound; an element whose bound is 0 must be exact; NaN counts as infinite."""
    err = (got.double() - ref).abs()
    r = torch.nan_to_num(torch.where(err == 0, torch.zeros_like(err), err / bound), nan=math.inf, posinf=math.inf)
    return float(r.max()) if r.numel() else 0.0


class Synthetic:
    """Tensors laid out in one flat arena with GAP poisoned guard elements before, between and behind them, and inside a
    tensor wherever a range belongs to "another rank".  spec: [(name, elements, class, [(from, to, zero_grad)] pieces relative
    to the tensor, kind)]."""

    def __init__(self, seed=0):
        rs = np.random.RandomState(seed)
        spec = [('wave', 64, PLAIN, None, ''),                      # 16 quads: less than one wave
                ('row', 768, ADAPT, None, ''),                      # an excluded 1-d tensor next to an adapted one
                ('big', 200004, ADAPT, None, ''),                   # several workgroups, two trips per thread under MAX_BLOCKS
                ('two', 1024, ADAPT, [(0, 384, 1), (384, 1024, 0)], ''),
                ('gap', 1024, ADAPT, [(0, 256, 1), (512, 768, 0), (768, 1024, 1)], ''),      # [256, 512) is another rank's
                ('zero_w', 388, ADAPT, None, 'zero_w'),             # zero weights, gradient: phi = 1
                ('idle', 260, NODECAY, None, 'idle')]               # zero gradient and moments: p unchanged to the bit
        spec += [('s%d' % i, 68 + 36 * (i % 7) + 4 * i, (ADAPT, PLAIN, NODECAY)[i % 3], None, '') for i in range(40)]
        self.tensors, pieces, off = [], [], GAP
        for tid, (name, n, cls, cut, kind) in enumerate(spec):
            cut = cut or [(0, n, 1)]
            self.tensors.append(dict(name=name, tid=tid, start=off, n=n, cls=cls, kind=kind, cut=[(off + a, off + b, z) for a, b, z in cut]))
            pieces += [(off + a, off + b, tid, z, cls) for a, b, z in cut]
            off += (n + 3) // 4 * 4 + GAP
        self.total, self.pieces = off, pieces
        host = {k: rs.standard_normal(off).astype(np.float32) for k in 'pgm'}
        host['p'] *= rs.choice([0.02, 1.0, 30.0], size=off).astype(np.float32)       # |p| / |r| far from 1 in both directions
        host['v'] = (rs.standard_normal(off).astype(np.float32) * 0.5) ** 2
        self.inside = torch.zeros(off, dtype=torch.bool)
        for a, b, *_ in pieces:
            self.inside[a:b] = True
        for t in self.tensors:
            sl = slice(t['start'], t['start'] + t['n'])
            if t['kind'] == 'zero_w':
                host['p'][sl] = 0
            if t['kind'] == 'idle':
                host['g'][sl] = host['m'][sl] = host['v'][sl] = 0
        self.before = {k: torch.from_numpy(x).cuda() for k, x in host.items()}
        for x in self.before.values():                # guards: 0xFF bytes (NaN) - a kernel that reads one poisons its sums
            x.view(torch.int32)[~self.inside.cuda()] = -1
        self.before['w'] = torch.full((off,), float('nan'), dtype=torch.bfloat16, device='cuda')
        self.inside = self.inside.cuda()
        self.table = ops.LambTable(pieces, len(self.tensors), len(CLASSES), off, device='cuda', max_blocks=MAX_BLOCKS)
        own = torch.cat([self.before['g'][a:b] for a, b, *_ in pieces]).double()
        # the device scalar of the clip: the pieces' sum of squares - with grad_scale 0.5 the norm is far above max_norm
        self.gnorm = (own * own).sum().reshape(1)
        self.hp = dict(HP, gnorm_sq=float(self.gnorm))

    def run(self, foreign=None):
        """The three launches on a fresh copy of the state -> dict(p, g, m, v, w, norms)."""
        s = {k: x.clone() for k, x in self.before.items()}
        t = self.table
        ops.lamb_update(s['p'], s['g'], s['m'], s['v'], t, CLASSES, HP['beta1'], HP['beta2'], HP['eps'], gnorm_sq=self.gnorm,
                        max_norm=HP['max_norm'], grad_scale=HP['grad_scale'])
        s['r'] = s['g'].clone()
        ops.lamb_norms(t)
        s['norms_own'] = t.norms.clone()
        if foreign is not None:                       # what the sum over the ranks adds between the two launches
            t.norms += foreign
        ops.lamb_apply(s['p'], s['g'], s['w'], t, CLASSES, HP['lr'])
        torch.cuda.synchronize()
        return s

    def owned(self, x, t):
        return torch.cat([x[a:b] for a, b, _ in t['cut']])


@pytest.fixture(scope='module')
def syn():
    s = Synthetic()
    s.after = s.run()
    return s


def _check(syn, after, foreign=None, what=''):
    qpt = syn.table.quads_per_thread()
    worst = dict(p=0.0, m=0.0, v=0.0, r=0.0, pp=0.0, rr=0.0)
    k = 0
    for t in syn.tensors:
        tq = max(qpt[k:k + len(t['cut'])])
        k += len(t['cut'])
        f = (0.0, 0.0) if foreign is None else foreign[t['tid']].tolist()
        ref = lamb_ref64(*(syn.owned(syn.before[c], t) for c in 'pgmv'), CLASSES[t['cls']], syn.hp, tq, f)
        for c in 'pmvr':
            w = _ratio(syn.owned(after[c], t), ref[c], ref[c + '_bound'])
            worst[c] = max(worst[c], w)
            assert w <= 1.0, '%s: %s of tensor %s (%d elements, %d pieces, %d quads per thread) is off by %.3g x its bound' % (
                what, c, t['name'], t['n'], len(t['cut']), tq, w)
        for i, c in enumerate(('pp', 'rr')):
            got = float(after['norms_own'][t['tid'], i])
            w = 0.0 if got == ref[c] else abs(got - ref[c]) / ref['e_' + c] if ref['e_' + c] > 0 else math.inf
            worst[c] = max(worst[c], w)
            assert w <= 1.0, '%s: sum %s^2 of tensor %s: %r against %r, %.3g x its bound' % (what, c[0], t['name'], got, ref[c], w)
    print('%s: worst error / bound  p %.3f  m %.3f  v %.3f  r %.3f  sum p^2 %.3f  sum r^2 %.3f' % (
        what, worst['p'], worst['m'], worst['v'], worst['r'], worst['pp'], worst['rr']))
    return worst


def test_table_covers_the_mechanisms(syn):
    t = syn.table
    assert t.n_tensors >= 40 and t.n_pieces > ops.LAMB_MAX_CLASSES          # more than any by-value table of 32
    big = syn.tensors[2]
    k = [i for i, p in enumerate(syn.pieces) if p[2] == big['tid']][0]
    q, nb = t.quads_per_thread()[k], t.blk0[k + 1] - t.blk0[k]
    assert nb >= 8 and q > 2, 'the big tensor wants several workgroups and more than one trip of two quads (%d, %d)' % (nb, q)
    assert syn.tensors[0]['n'] // 4 < 64


def test_every_element_within_its_bound(syn):
    worst = _check(syn, syn.after, what='lamb launches')
    assert worst['p'] > 0 and worst['r'] > 0           # (fp32 arithmetic is not exact: a ratio of 0 means nothing was compared)


def test_special_tensors(syn):
    by = {t['name']: t for t in syn.tensors}
    idle = by['idle']
    sl = slice(idle['start'], idle['start'] + idle['n'])
    for c in 'pmv':
        assert_bits_equal(syn.after[c][sl], syn.before[c][sl], 'zero gradient and moments: ' + c)
    z = by['zero_w']
    zs = slice(z['start'], z['start'] + z['n'])
    ref = lamb_ref64(*(syn.before[c][zs] for c in 'pgmv'), CLASSES[z['cls']], syn.hp, 1)
    assert ref['phi'] == 1.0 and ref['pp'] == 0.0 and ref['rr'] > 0
    assert float(syn.after['p'][zs].abs().max()) > 0
    # the gap tensor's norms cover its owned part only (the foreign range holds NaN: a read of it would show)
    g = by['gap']
    own = syn.owned(syn.before['p'], g).double()
    assert abs(float(syn.after['norms_own'][g['tid'], 0]) - float((own * own).sum())) <= 16 * U32 * float((own * own).sum())
    # an excluded tensor steps with phi = 1 although its norms would say otherwise
    w = by['wave']
    ref = lamb_ref64(*(syn.before[c][w['start']:w['start'] + w['n']] for c in 'pgmv'), CLASSES[ADAPT], syn.hp, 1)
    assert abs(ref['phi'] - 1.0) > 0.05


def test_nothing_outside_the_pieces_is_written(syn):
    out = ~syn.inside
    for c in 'pgmvw':
        assert_bits_equal(syn.after[c][out], syn.before[c][out], 'guard elements of ' + c)
    assert int(out.sum()) >= GAP * (len(syn.tensors) + 1) + 256


def test_gradient_and_working_copy_after_the_call(syn):
    for a, b, _, z, _ in syn.pieces:
        if z:
            assert_exact_zero(syn.after['g'][a:b], 'gradient of piece [%d, %d)' % (a, b))
        assert_bits_equal(syn.after['w'][a:b], syn.after['p'][a:b].to(torch.bfloat16), 'bf16 copy of piece [%d, %d)' % (a, b))
    assert any(not z for *_, z, _ in syn.pieces)


def test_same_state_same_bits(syn):
    again = syn.run()
    for c in 'pmvw':
        assert_bits_equal(again[c], syn.after[c], 'second run: ' + c)
    assert_bits_equal(again['norms_own'], syn.after['norms_own'], 'second run: norms')


def test_foreign_partial_sums_move_phi(syn):
    """What the other ranks' shards add to a tensor's sums between the norms and apply launches changes its factor as the
    fp64 twin says - for the tensor with the foreign gap and for one small tensor; a tensor whose row stays 0 is unmoved."""
    by = {t['name']: t for t in syn.tensors}
    foreign = torch.zeros((len(syn.tensors), 2), dtype=torch.float64, device='cuda')
    g, s0 = by['gap'], by['s0']
    foreign[g['tid']] = torch.tensor([3.0 * float(syn.after['norms_own'][g['tid'], 0]), 0.25 * float(syn.after['norms_own'][g['tid'], 1])])
    foreign[s0['tid']] = torch.tensor([0.0, 8.0 * float(syn.after['norms_own'][s0['tid'], 1])])
    after = syn.run(foreign)
    _check(syn, after, foreign, what='with foreign sums')
    for t, factor in ((g, math.sqrt(4.0 / 1.25)), (s0, math.sqrt(1.0 / 9.0))):
        sl = [slice(a, b) for a, b, _ in t['cut']]
        moved = torch.cat([after['p'][x] - syn.before['p'][x] for x in sl]).double()
        plain = torch.cat([syn.after['p'][x] - syn.before['p'][x] for x in sl]).double()
        got = float(moved.norm() / plain.norm())
        assert abs(got / factor - 1.0) < 1e-4, (t['name'], got, factor)
    row = by['row']
    sl = slice(row['start'], row['start'] + row['n'])
    assert_bits_equal(after['p'][sl], syn.after['p'][sl], 'a tensor without foreign sums')


def test_bad_arguments_change_nothing(syn):
    """Pieces and class counts are validated where the table is built (m3p_lamb_table_build, host only - by design nothing
    has been launched at that point, so the unchanged state is trivial for those cases and they only show the error code);
    the calls that reach a launcher and must be turned away by it are the ones with a misaligned base."""
    s = {k: x.clone() for k, x in syn.before.items()}
    t = syn.table
    a0 = syn.tensors[1]['start']
    for bad in ([(a0, a0 + 766, 0, 1, 0)], [(a0 + 2, a0 + 770, 0, 1, 0)],            # a piece border off the quad grid
                [(a0, a0 + 768, 0, 1, len(CLASSES))],                                  # a class the launch has no scalars for
                [(a0, syn.total + 64, 0, 1, 0)]):                                       # past the arena
        with pytest.raises(L.M3PError, match='M3P_EINVAL'):
            ops.LambTable(bad, 1, len(CLASSES), syn.total, device='cuda')
    with pytest.raises(L.M3PError, match='M3P_EINVAL'):
        ops.LambTable(syn.pieces, len(syn.tensors), ops.LAMB_MAX_CLASSES + 1, syn.total, device='cuda')
    with pytest.raises(L.M3PError, match='M3P_EINVAL'):                                 # a base off the 16-byte grid
        ops.lamb_update(s['p'][1:], s['g'][1:], s['m'][1:], s['v'][1:], t, CLASSES, HP['beta1'], HP['beta2'], HP['eps'])
    with pytest.raises(L.M3PError, match='M3P_EINVAL'):
        ops.lamb_apply(s['p'][1:], s['g'][1:], s['w'], t, CLASSES, HP['lr'])
    with pytest.raises(AssertionError):                                                 # fewer class scalars than the table names
        ops.lamb_update(s['p'], s['g'], s['m'], s['v'], t, CLASSES[:2], HP['beta1'], HP['beta2'], HP['eps'])
    torch.cuda.synchronize()
    for c in 'pgmvw':
        assert_bits_equal(s[c], syn.before[c], 'after refused calls: ' + c)
