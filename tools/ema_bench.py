#!/usr/bin/env python3
"""Cost of the exponential moving average of the weights on a cfg2-sized arena (280 M elements), at the level of the launches:
  * m3p_ema_update and m3p_ema_swap on their own, with the fused Adam launch (m3p_adam_step_ranges, the step's two pieces)
    timed in the same run for its bandwidth;
  * the optimizer launches of a step - Adam's one, LAMB's three - without EMA, with an update every step and with one every
    tenth step, in alternating windows;
  * one ema_weights() entry and exit: the swap over the whole arena and the batched transposes of the layer weights, twice.
Protocol as tools/lamb_bench.py: warm-up of every arm, then three rounds of windows of --iters steps each between device events.
    python tools/ema_bench.py [--iters 100] [--out profiles/ema_step.txt]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from m3p_amd import ops   # noqa: E402
from lamb_bench import D, HP, LAYERS, N_TOTAL, N_VOCAB, tensors   # noqa: E402

DECAY = 0.9999


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ema_step.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'ema_bench.py measures on the GPU: no device, no number'
    assert args.iters % 10 == 0, 'a window holds whole groups of ten steps'
    dev = 'cuda'
    p, m = (torch.randn(N_TOTAL, device=dev) * 0.02 for _ in range(2))
    v = (torch.randn(N_TOTAL, device=dev) * 0.02) ** 2
    g = torch.empty(N_TOTAL, device=dev)
    ema = p.clone()
    w16 = torch.zeros(N_TOTAL, dtype=torch.bfloat16, device=dev)
    gn = torch.full((1,), 25.0, dtype=torch.float64, device=dev)
    w = torch.tensor(1.0 - DECAY, dtype=torch.float64).to(torch.float32).item()
    pieces, off, mats = [(0, N_VOCAB, 0, 0, 0)], N_VOCAB, []
    for tid, (n, mat) in enumerate(tensors(), 1):
        pieces.append((off, off + n, tid, 1, 0 if mat else 1))
        if mat and n in (D * D, 4 * D * D):
            mats.append((off, n))
        off += n
    assert off == N_TOTAL
    table = ops.LambTable(pieces, len(pieces), 2, N_TOTAL, device=dev)
    s = 10
    classes = [(1 / (1 - HP['beta1'] ** s), 1 / (1 - HP['beta2'] ** s), HP['wd'], True),
               (1 / (1 - HP['beta1'] ** s), 1 / (1 - HP['beta2'] ** s), 0.0, False)]
    step_size = HP['lr'] * (1 - HP['beta2'] ** s) ** 0.5 / (1 - HP['beta1'] ** s)
    adam_pieces = [(0, N_VOCAB, step_size, False), (N_VOCAB, N_TOTAL, step_size, True)]
    whole = [(0, N_TOTAL)]
    # the transposed copies Arena.refresh_transposes makes: per layer q | k | v as one [3d, d] matrix, out, lin1, lin2
    rows, per_layer = [], len(mats) // LAYERS
    assert per_layer == 6
    for i in range(LAYERS):
        q, _, _, o, l1, l2 = mats[i * per_layer:(i + 1) * per_layer]
        for (o0, n), (r, c) in (((q[0], 3 * D * D), (3 * D, D)), (o, (D, D)), (l1, (4 * D, D)), (l2, (D, 4 * D))):
            dst = torch.zeros((c, r), dtype=torch.bfloat16, device=dev)
            rows.append(([w16[o0:o0 + r * c].data_ptr(), dst.data_ptr(), r, c, c, r], dst))
    tdesc = torch.tensor([r for r, _ in rows], dtype=torch.int64, device=dev)
    tiles = max(((r[2] + 63) // 64) * ((r[3] + 63) // 64) for r, _ in rows)
    t_bytes = sum(r[2] * r[3] * 4 for r, _ in rows)

    def adam():
        ops.adam_step_ranges(p, g, m, v, w16, adam_pieces, HP['lr'], HP['beta1'], HP['beta2'], 1e-8, 0.0, gnorm_sq=gn, max_norm=HP['max_norm'])

    def lamb():
        ops.lamb_update(p, g, m, v, table, classes, HP['beta1'], HP['beta2'], HP['eps'], gnorm_sq=gn, max_norm=HP['max_norm'])
        ops.lamb_norms(table)
        ops.lamb_apply(p, g, w16, table, classes, HP['lr'])

    def update():
        ops.ema_update(p, ema, whole, w)

    def swap():
        ops.ema_swap(p, ema, w16, whole)

    def enter_and_leave():
        for _ in range(2):
            swap()
            ops.transpose_batch(tdesc, len(rows), tiles)

    def with_ema(step, every):
        count = [0]

        def fn():
            step()
            if count[0] % every == 0:
                update()
            count[0] += 1
        return fn

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

    arms = [('adam', adam), ('adam+ema/1', with_ema(adam, 1)), ('adam+ema/10', with_ema(adam, 10)),
            ('lamb', lamb), ('lamb+ema/1', with_ema(lamb, 1)), ('lamb+ema/10', with_ema(lamb, 10))]
    singles = [('ema_update', update), ('adam', adam), ('ema_swap', swap)]
    for _, fn in arms + singles:          # warm-up: code objects, the table's upload, clocks
        window(fn, 10)
    # a window starts with one un-timed call: iters + 1 calls keep the every-tenth arm's count in step with the windows
    rounds = [[window(fn, args.iters) for _, fn in arms] for _ in range(3)]
    alone = [[window(fn, args.iters) for _, fn in singles] for _ in range(3)]
    t_ctx = sorted(window(enter_and_leave, 10) for _ in range(3))[1]
    med = lambda xs: sorted(xs)[len(xs) // 2]       # noqa: E731
    t = {name: med([r[i] for r in rounds]) for i, (name, _) in enumerate(arms)}
    a = {name: med([r[i] for r in alone]) for i, (name, _) in enumerate(singles)}
    rest = N_TOTAL - N_VOCAB
    gb = dict(adam=(N_VOCAB * 30 + rest * 34) / 1e9, ema_update=N_TOTAL * 12 / 1e9, ema_swap=N_TOTAL * 18 / 1e9)
    bw = {k: gb[k] / a[k] for k in gb}
    lines = ['# tools/ema_bench.py: the EMA of the weights on a cfg2-sized arena (%d elements), %s; %d steps per window between'
             % (N_TOTAL, torch.cuda.get_device_name(0), args.iters),
             '# device events, three rounds over all arms after a warm-up of each; medians below the table.  decay %g (w = %.9g).'
             % (DECAY, w),
             '# Bytes counted from the design: ema_update 12 B / element (p and ema read, ema written) = %.2f GB, ema_swap 18 (two'
             % gb['ema_update'],
             '# fp32 streams read, two written, the bf16 copy written) = %.2f GB, the Adam launch %.2f GB (34 B / element, 30 where'
             % (gb['ema_swap'], gb['adam']),
             '# the vocabulary gradient is left un-zeroed).',
             'round ' + ''.join('%13s' % name for name, _ in arms) + '   (ms per step)']
    lines += ['%5d ' % (i + 1) + ''.join('%13.3f' % x for x in r) for i, r in enumerate(rounds)]
    lines += ['median' + ''.join('%13.3f' % t[name] for name, _ in arms),
              'EMA every step:        adam %+.3f ms (%+.1f %%),  lamb %+.3f ms (%+.1f %%)'
              % (t['adam+ema/1'] - t['adam'], 100 * (t['adam+ema/1'] / t['adam'] - 1), t['lamb+ema/1'] - t['lamb'],
                 100 * (t['lamb+ema/1'] / t['lamb'] - 1)),
              'EMA every tenth step:  adam %+.3f ms (%+.1f %%),  lamb %+.3f ms (%+.1f %%)'
              % (t['adam+ema/10'] - t['adam'], 100 * (t['adam+ema/10'] / t['adam'] - 1), t['lamb+ema/10'] - t['lamb'],
                 100 * (t['lamb+ema/10'] / t['lamb'] - 1)),
              'launches on their own, back to back (three windows each, median):',
              '  m3p_ema_update        %.3f ms = %.2f TB/s' % (a['ema_update'], bw['ema_update']),
              '  m3p_adam_step_ranges  %.3f ms = %.2f TB/s' % (a['adam'], bw['adam']),
              '  m3p_ema_swap          %.3f ms = %.2f TB/s' % (a['ema_swap'], bw['ema_swap']),
              '  ema_update / adam bandwidth: %.2f' % (bw['ema_update'] / bw['adam']),
              'one ema_weights() entry and exit (two swaps + two batched transposes of %d matrices, %.2f GB each): %.3f ms'
              % (len(rows), t_bytes / 1e9, t_ctx)]
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
