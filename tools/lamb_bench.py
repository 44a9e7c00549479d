#!/usr/bin/env python3
"""Time of the optimizer launches of one step on a cfg2-sized arena (280 M elements): fused Adam (m3p_adam_step_ranges, the
step's two pieces) against LAMB's three launches (m3p_lamb_update / _norms / _apply over a piece table of 194 tensors).
Both leave the vocabulary range's gradient un-zeroed, as the benchmarked step does.  Protocol: warm-up of both arms, then
three alternating pairs of windows of --iters steps each between device events; then one window per LAMB launch on its own.
    python tools/lamb_bench.py [--iters 100] [--out profiles/lamb_step.txt]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from m3p_amd import ops   # noqa: E402

D, LAYERS, N_TOTAL, N_VOCAB = 768, 12, 279_937_024, 192_086_016
HP = dict(lr=1e-4, beta1=0.9, beta2=0.98, eps=1e-6, wd=0.01, max_norm=5.0)


def tensors():
    """[(elements, two or more dimensions)] after the vocabulary matrix: per layer q, k, v, out, lin1, lin2 and their vectors,
    the rest of the arena as one matrix."""
    out = []
    for _ in range(LAYERS):
        for n, mat in ((D * D, 1), (D, 0)) * 4 + ((D, 0), (D, 0), (4 * D * D, 1), (4 * D, 0), (4 * D * D, 1), (D, 0), (D, 0), (D, 0)):
            out.append((n, mat))
    used = N_VOCAB + sum(n for n, _ in out)
    out.append((N_TOTAL - used, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lamb_step.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'lamb_bench.py measures on the GPU: no device, no number'
    dev = 'cuda'
    p, m = (torch.randn(N_TOTAL, device=dev) * 0.02 for _ in range(2))
    v = (torch.randn(N_TOTAL, device=dev) * 0.02) ** 2
    g = torch.empty(N_TOTAL, device=dev)
    w16 = torch.zeros(N_TOTAL, dtype=torch.bfloat16, device=dev)
    gn = torch.full((1,), 25.0, dtype=torch.float64, device=dev)
    pieces, off = [(0, N_VOCAB, 0, 0, 0)], N_VOCAB
    for tid, (n, mat) in enumerate(tensors(), 1):
        pieces.append((off, off + n, tid, 1, 0 if mat else 1))
        off += n
    assert off == N_TOTAL
    table = ops.LambTable(pieces, len(pieces), 2, N_TOTAL, device=dev)
    s = 10
    classes = [(1 / (1 - HP['beta1'] ** s), 1 / (1 - HP['beta2'] ** s), HP['wd'], True),
               (1 / (1 - HP['beta1'] ** s), 1 / (1 - HP['beta2'] ** s), 0.0, False)]
    step_size = HP['lr'] * (1 - HP['beta2'] ** s) ** 0.5 / (1 - HP['beta1'] ** s)
    adam_pieces = [(0, N_VOCAB, step_size, False), (N_VOCAB, N_TOTAL, step_size, True)]

    def adam():
        ops.adam_step_ranges(p, g, m, v, w16, adam_pieces, HP['lr'], HP['beta1'], HP['beta2'], 1e-8, 0.0, gnorm_sq=gn, max_norm=HP['max_norm'])

    def update():
        ops.lamb_update(p, g, m, v, table, classes, HP['beta1'], HP['beta2'], HP['eps'], gnorm_sq=gn, max_norm=HP['max_norm'])

    def norms():
        ops.lamb_norms(table)

    def apply():
        ops.lamb_apply(p, g, w16, table, classes, HP['lr'])

    def lamb():
        update(); norms(); apply()

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

    for fn in (adam, lamb):               # warm-up: code objects, the table's upload, clocks
        window(fn, 10)
    rows = [(window(adam, args.iters), window(lamb, args.iters)) for _ in range(3)]
    # each launch on its own, repeated: `update` then reads its own r as the gradient and `apply` uses the norms of the last
    # full step, on state that drifts - meaningless as an optimizer, harmless for a time: no kernel's work depends on its data
    parts = {k: window(fn, args.iters) for k, fn in (('update', update), ('norms', norms), ('apply', apply))}
    rest = N_TOTAL - N_VOCAB
    gb = dict(adam=(N_VOCAB * 30 + rest * 34) / 1e9, update=N_TOTAL * 28 / 1e9, apply=(N_VOCAB * 14 + rest * 18) / 1e9)
    gb['lamb'] = gb['update'] + gb['apply']
    med = lambda xs: sorted(xs)[len(xs) // 2]       # noqa: E731
    ta, tl = med([a for a, _ in rows]), med([b for _, b in rows])
    lines = ['# tools/lamb_bench.py: optimizer launches of one step, cfg2-sized arena (%d elements, %d of them the vocabulary range'
             % (N_TOTAL, N_VOCAB),
             '# whose gradient is not zeroed), %s; %d steps per window between device events, three alternating pairs after warm-up.'
             % (torch.cuda.get_device_name(0), args.iters),
             '# LAMB: %d pieces of %d tensors in one table, %d workgroups; bytes counted from the design: Adam %.2f GB, LAMB %.2f GB'
             % (table.n_pieces, table.n_tensors, table.n_blocks, gb['adam'], gb['lamb']),
             '# (update 28 B / element; apply 18, 14 where the gradient is left; the norms launch reads %d pairs).' % table.n_blocks,
             'pair   adam ms   lamb ms   ratio']
    lines += ['%4d  %8.3f  %8.3f  %6.3f' % (i + 1, a, b, b / a) for i, (a, b) in enumerate(rows)]
    lines += ['median adam %.3f ms = %.2f TB/s;  lamb %.3f ms = %.2f TB/s;  ratio %.3f (by bytes: %.3f)'
              % (ta, gb['adam'] / ta, tl, gb['lamb'] / tl, tl / ta, gb['lamb'] / gb['adam']),
              'lamb launches on their own:  update %.3f ms = %.2f TB/s;  norms %.3f ms;  apply %.3f ms = %.2f TB/s'
              % (parts['update'], gb['update'] / parts['update'], parts['norms'], parts['apply'], gb['apply'] / parts['apply'])]
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
