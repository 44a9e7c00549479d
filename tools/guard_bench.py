#!/usr/bin/env python3
"""What the non-finite guard costs: the launches of one optimizer step on the cfg2-sized arena of tools/lamb_bench.py (280 M
elements), Adam and LAMB, in these arms:
    off/clip   norm reduction + update launches, unguarded entry points (what Adam.step launches with clip_grad_norm 5)
    on/clip    the same + m3p_step_guard, the _guarded entry points
    off/0      update launches alone (no clipping: nothing reduces the norm)
    on/0       norm reduction + m3p_step_guard + the _guarded entry points (the guard reduces the norm itself)
    skip       on/clip with a non-finite norm: the skipped step (one write of the flagged gradient pieces)
and, with --parent-lib, `parent`: off/clip through another build of the library (the parent commit's), to show that the
unguarded path did not move.  Protocol as lamb_bench.py: warm-up of every arm, then three rounds in which the arms alternate,
--iters steps per window between device events.
    python tools/guard_bench.py [--iters 100] [--parent-lib PATH] [--out profiles/nonfinite_guard.txt]"""
import argparse
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from m3p_amd import lib as L, ops   # noqa: E402
from lamb_bench import HP, N_TOTAL, N_VOCAB, tensors   # noqa: E402


def open_lib(path):
    """Another build of the library with the ctypes signatures of the entry points it shares with this tree."""
    lib = C.CDLL(path)
    for name, (res, args) in L.SIGNATURES.items():
        if hasattr(lib, name):
            getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'nonfinite_guard.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'guard_bench.py measures on the GPU: no device, no number'
    dev = 'cuda'
    tree = L.load()
    parent = open_lib(args.parent_lib) if args.parent_lib else None
    p, m = (torch.randn(N_TOTAL, device=dev) * 0.02 for _ in range(2))
    v = (torch.randn(N_TOTAL, device=dev) * 0.02) ** 2
    g = torch.empty(N_TOTAL, device=dev)
    w16 = torch.zeros(N_TOTAL, dtype=torch.bfloat16, device=dev)
    gn = torch.zeros(1, dtype=torch.float64, device=dev)
    bad = torch.full((1,), float('inf'), dtype=torch.float64, device=dev)
    guard = ops.StepGuard(dev)
    pieces, off = [(0, N_VOCAB, 0, 0, 0)], N_VOCAB
    for tid, (n, mat) in enumerate(tensors(), 1):
        pieces.append((off, off + n, tid, 1, 0 if mat else 1))
        off += n
    table = ops.LambTable(pieces, len(pieces), 2, N_TOTAL, device=dev)
    s = 10
    classes = [(1 / (1 - HP['beta1'] ** s), 1 / (1 - HP['beta2'] ** s), HP['wd'], True),
               (1 / (1 - HP['beta1'] ** s), 1 / (1 - HP['beta2'] ** s), 0.0, False)]
    rbc1, rbc2, wd, adapt = ops._lamb_classes(classes, 2)
    step_size = HP['lr'] * (1 - HP['beta2'] ** s) ** 0.5 / (1 - HP['beta1'] ** s)
    starts, counts = (C.c_longlong * 2)(0, N_VOCAB), (C.c_longlong * 2)(N_VOCAB, N_TOTAL - N_VOCAB)
    steps, zeros = (C.c_float * 2)(step_size, step_size), (C.c_int * 2)(0, 1)
    attempt = [0]

    def reduce_norm(lib):
        gn.zero_()
        L.check(lib.m3p_sumsq_f32(g.data_ptr(), N_TOTAL, gn.data_ptr(), L.stream()), 'sumsq')

    def decide(sums):
        ops.step_guard([sums], 1.0, attempt[0], guard)
        attempt[0] += 1

    def adam(lib, clip, guarded):
        a = [p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), w16.data_ptr(), starts, counts, steps, zeros, 2, HP['lr'], HP['beta1'],
             HP['beta2'], 1e-8, 0.0, gn.data_ptr() if clip else None, HP['max_norm'] if clip else 0.0, 1.0]
        if guarded:
            L.check(lib.m3p_adam_step_ranges_guarded(*a, guard.skip.data_ptr(), L.stream()), 'adam guarded')
        else:
            L.check(lib.m3p_adam_step_ranges(*a, L.stream()), 'adam')

    def lamb(lib, clip, guarded):
        sk = (guard.skip.data_ptr(),) if guarded else ()
        sfx = '_guarded' if guarded else ''
        t = table
        L.check(getattr(lib, 'm3p_lamb_update' + sfx)(
            p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), t.dev_pieces.data_ptr(), t.n_pieces, t.n_blocks, rbc1, rbc2, wd, adapt, 2,
            HP['beta1'], HP['beta2'], HP['eps'], gn.data_ptr() if clip else None, HP['max_norm'] if clip else 0.0, 1.0,
            t.partials.data_ptr(), *sk, L.stream()), 'update')
        L.check(getattr(lib, 'm3p_lamb_norms' + sfx)(t.partials.data_ptr(), t.dev_tblk.data_ptr(), t.n_tensors, t.norms.data_ptr(), *sk,
                                                    L.stream()), 'norms')
        L.check(getattr(lib, 'm3p_lamb_apply' + sfx)(p.data_ptr(), g.data_ptr(), w16.data_ptr(), t.dev_pieces.data_ptr(), t.n_pieces, t.n_blocks,
                                                    t.norms.data_ptr(), adapt, 2, HP['lr'], *sk, L.stream()), 'apply')

    def arms(update):
        out = {}
        if parent is not None:
            out['parent'] = lambda: (reduce_norm(parent), update(parent, True, False))
        out['off/clip'] = lambda: (reduce_norm(tree), update(tree, True, False))
        out['on/clip'] = lambda: (reduce_norm(tree), decide(gn), update(tree, True, True))
        out['off/0'] = lambda: update(tree, False, False)
        out['on/0'] = lambda: (reduce_norm(tree), decide(gn), update(tree, False, True))
        out['skip'] = lambda: (reduce_norm(tree), decide(bad), update(tree, True, True))
        return out

    def window(fn, iters):
        g.normal_(0, 0.01)                # (outside the window: a fresh gradient keeps the moments away from denormals)
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    def guard_alone(iters):
        return window(lambda: decide(gn), iters)

    lines = ['# tools/guard_bench.py: launches of one optimizer step, cfg2-sized arena (%d elements, %d of them the vocabulary range whose'
             % (N_TOTAL, N_VOCAB),
             '# gradient is not zeroed), %s; ms per step, %d steps per window between device events, three rounds of alternating arms'
             % (torch.cuda.get_device_name(0), args.iters),
             '# after a warm-up of every arm.  off = unguarded entry points, on = m3p_step_guard + the _guarded ones; clip = the norm is',
             '# reduced for clipping anyway, 0 = no clipping (the guard then pays for the reduction); skip = a step with a non-finite norm;',
             '# parent = off/clip through the parent commit\'s build of the library.']
    med = lambda xs: sorted(xs)[len(xs) // 2]       # noqa: E731
    for name, update in (('adam', adam), ('lamb', lamb)):
        fns = arms(update)
        for fn in fns.values():
            window(fn, 10)
        rows = [{k: window(fn, args.iters) for k, fn in fns.items()} for _ in range(3)]
        lines.append('%-5s round  ' % name + '  '.join('%9s' % k for k in fns))
        lines += ['%-5s %5d  ' % (name, i + 1) + '  '.join('%9.4f' % r[k] for k in fns) for i, r in enumerate(rows)]
        lines.append('%-5s median ' % name + '  '.join('%9.4f' % med([r[k] for r in rows]) for k in fns))
        if parent is not None:
            par = [r['parent'] for r in rows]
            lines.append('%-5s parent spread %.4f ms (max - min of its three windows); off/clip - parent (medians) %+.4f ms'
                         % (name, max(par) - min(par), med([r['off/clip'] for r in rows]) - med(par)))
        lines.append('%-5s on/clip - off/clip (medians) %+.4f ms;  on/0 - off/0 %+.4f ms'
                     % (name, med([r['on/clip'] for r in rows]) - med([r['off/clip'] for r in rows]),
                        med([r['on/0'] for r in rows]) - med([r['off/0'] for r in rows])))
    ga = [guard_alone(args.iters) for _ in range(3)]
    g.normal_(0, 0.01)
    rn = [window(lambda: reduce_norm(tree), args.iters) for _ in range(3)]
    lines.append('on their own: m3p_step_guard %.4f ms per launch;  norm reduction (memset + m3p_sumsq_f32, %.2f GB) %.4f ms'
                 % (med(ga), N_TOTAL * 4 / 1e9, med(rn)))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
