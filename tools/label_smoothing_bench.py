#!/usr/bin/env python
"""What label smoothing costs the vocabulary head.

The head alone - model.predict forward plus backward on a synthetic bf16 (T, B, d) tensor - at BASELINE configs[1]'s head
(V = 250 002, d = 768, 256 x 19 = 4864 predicted rows), timed with device events:

  * eps = 0.1 against eps = 0 in one process, alternating, three pairs.  Every timed pass follows a simulated optimizer step
    (the arena is told its weights were updated), so the smoothed passes include the once-per-step mean row - asserted by
    counting its launches; the mean-row launch and the uniform add are also timed on their own;
  * with --parent PATH (a built checkout of the parent commit): eps = 0 of this tree against the parent's head, one fresh
    process per sample, alternating, three pairs - the off state must cost nothing beyond the noise between samples.

    python tools/label_smoothing_bench.py [--parent PATH] [--pairs 3] [--iters 20] > profiles/label_smoothing.txt
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _setup(tree, d, V, T, B):
    sys.path.insert(0, tree)
    import torch
    from m3p_amd import synth
    from m3p_amd.model.transformer import TransformerModel
    P = synth.model_params(d, d // 64, 1, V)
    torch.manual_seed(0)
    m = TransformerModel(P, is_encoder=True, with_output=True, is_crossModal=True).cuda().train()
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        m.embeddings.weight.copy_((torch.randn((V, d), generator=g) * (1.2 / math.sqrt(d))))
        m.pred_layer.proj.bias.copy_(torch.randn((V,), generator=g) * 0.5)
    m.arena().mark_master_changed()
    H = torch.randn((T, B, d), generator=g).to(torch.bfloat16).cuda()
    y = torch.randint(0, V, (T * B,), generator=g).cuda()
    mask = torch.ones((T, B), dtype=torch.bool, device='cuda')
    return torch, m, H, y, mask


def _time_head(torch, m, H, y, mask, eps, iters):
    """Median and spread (ms) of `iters` forward + backward passes of the head, each behind a zeroed gradient and an optimizer step's notice."""
    from m3p_amd import ops
    m.label_smoothing = eps
    ar = m.arena()
    times = []
    launches, real = [0], getattr(ops, 'vocab_mean', None)
    if eps > 0:
        def counted(*a, **kw):
            launches[0] += 1
            return real(*a, **kw)
        ops.vocab_mean = counted
    for it in range(iters + 3):
        ar.zero_grad()
        ar.mark_updated_by_fused_optimizer()     # what an optimizer step tells the arena: the cached mean row is stale
        tensor = H.clone().requires_grad_(True)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _, loss = m('predict', tensor=tensor, pred_mask=mask, y=y, get_scores=False)
        loss.backward()
        b.record()
        torch.cuda.synchronize()
        if it >= 3:
            times.append(a.elapsed_time(b))
    m.label_smoothing = 0.0
    if eps > 0:
        ops.vocab_mean = real
        assert launches[0] == iters + 3, 'the smoothed passes did not each include a mean-row launch'
    return statistics.median(times), min(times), max(times)


def _time_call(torch, fn, iters):
    times = []
    for it in range(iters + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if it >= 3:
            times.append(a.elapsed_time(b))
    return statistics.median(times)


def _sample(args):
    """One process, one figure: the eps = 0 head of the tree in --tree."""
    torch, m, H, y, mask = _setup(args.tree, args.d, args.V, args.T, args.B)
    med, lo, hi = _time_head(torch, m, H, y, mask, 0.0, args.iters)
    print(json.dumps({'tree': args.tree, 'ms': med, 'min': lo, 'max': hi}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit')
    ap.add_argument('--pairs', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--d', type=int, default=768)
    ap.add_argument('--V', type=int, default=250002)
    ap.add_argument('--T', type=int, default=19)
    ap.add_argument('--B', type=int, default=256)
    ap.add_argument('--sample', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--tree', default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.sample:
        return _sample(args)
    torch, m, H, y, mask = _setup(ROOT, args.d, args.V, args.T, args.B)
    from m3p_amd import ops
    n, d, V = args.T * args.B, args.d, args.V
    gb_mean, gb_add = V * d * 2 / 1e9, V * d * 8 / 1e9
    est = (gb_mean + gb_add) / 5.0          # ms at 5.0 TB/s, the fused Adam pass's rate inside the step
    print('label smoothing of the vocabulary head: V = %d, d = %d, n = %d rows, %s' % (V, d, n, torch.cuda.get_device_name(0)))
    print('bytes: mean row %.3f GB read (once per optimizer step), uniform add %.3f GB read + written; %.3f ms at 5.0 TB/s' % (
        gb_mean, gb_add, est))
    ar = m.arena()
    ar.refresh()
    t_mean = _time_call(torch, lambda: ops.vocab_mean(ar.w('embeddings.weight'), ar.p('pred_layer.proj.bias'), V), args.iters)
    u = torch.randn(d, device='cuda')
    g1 = torch.ones(1, device='cuda')
    ar.zero_grad()
    t_add = _time_call(torch, lambda: ops.ls_uniform_add(ar.g('embeddings.weight'), ar.g('pred_layer.proj.bias'), u, g1, -0.1 / V, V),
                       args.iters)
    print('kernels alone: vocab_mean %.3f ms (%.2f TB/s), ls_uniform_add %.3f ms (%.2f TB/s)' % (
        t_mean, gb_mean / t_mean, t_add, gb_add / t_add))
    added = []
    for k in range(args.pairs):
        on = _time_head(torch, m, H, y, mask, 0.1, args.iters)
        off = _time_head(torch, m, H, y, mask, 0.0, args.iters)
        added.append(on[0] - off[0])
        print('pair %d: eps = 0.1 %.3f ms [%.3f, %.3f], eps = 0 %.3f ms [%.3f, %.3f], added %.3f ms' % ((k + 1,) + on + off + (added[-1],)))
    med_added = statistics.median(added)
    print('added by eps = 0.1: median %.3f ms = %.2f x the byte estimate (bar: 1.5 x)' % (med_added, med_added / est))
    result = {'added_ms': med_added, 'estimate_ms': est, 'ratio': med_added / est, 'vocab_mean_ms': t_mean, 'uniform_add_ms': t_add}
    if args.parent:
        here, there = [], []
        for k in range(args.pairs):
            order = ((ROOT, here), (os.path.abspath(args.parent), there))
            for tree, out in (order if k % 2 == 0 else order[::-1]):       # (which tree goes first alternates too)
                cmd = [sys.executable, os.path.abspath(__file__), '--sample', '--tree', tree, '--iters', str(args.iters), '--d', str(d),
                       '--V', str(V), '--T', str(args.T), '--B', str(args.B)]
                r = subprocess.run(cmd, stdout=subprocess.PIPE, check=True, timeout=300, cwd=tree)
                out.append(json.loads(r.stdout.decode().strip().splitlines()[-1])['ms'])
            print('pair %d: eps = 0 here %.3f ms, parent commit %.3f ms' % (k + 1, here[-1], there[-1]))
        spread = max(max(here) - min(here), max(there) - min(there))
        diff = statistics.median(here) - statistics.median(there)
        print('eps = 0 against the parent: %+.3f ms (spread between samples of one tree: %.3f ms)' % (diff, spread))
        result.update(off_vs_parent_ms=diff, sample_spread_ms=spread)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
