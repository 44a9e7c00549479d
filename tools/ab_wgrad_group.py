#!/usr/bin/env python3
"""A/B of the grouped whole-tile weight-gradient launch against the launches it replaces, inside ONE process (see
tools/ab_wgrad.py): the layer weight gradients of 2 1/3 encoder layers at cfg2's sizes - seven 36-tile units: lin2, lin1, the
q/k/v + out_lin pair, ... - with operands of their own per unit, as in the step.
  grouped     one m3p_gemm_wgrad_group_bf16 launch (252 tiles, one workgroup each over all of M)
  per product the same products through m3p_gemm_wgrad_bf16 / m3p_gemm_wgrad_pair_bf16 (seven launches + seven reductions)
The arms alternate; the median of the rounds is reported, and with --check the two results must agree to fp32 accumulation
error.      python tools/ab_wgrad_group.py [--check] [--rounds 9]        (AB_M: rows, default 41984)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from m3p_amd import ops   # noqa: E402

check = '--check' in sys.argv
rounds = int(sys.argv[sys.argv.index('--rounds') + 1]) if '--rounds' in sys.argv else 9
M = int(os.environ.get('AB_M', '41984'))
d = 768
bf = torch.bfloat16


def rnd(*shape):
    return torch.randn(*shape, device='cuda').to(bf)


def unit(kind):
    if kind == 'lin2':
        return [(rnd(M, d), rnd(M, 4 * d), torch.zeros(d, 4 * d, device='cuda'))]
    if kind == 'lin1':
        return [(rnd(M, 4 * d), rnd(M, d), torch.zeros(4 * d, d, device='cuda'))]
    return [(rnd(M, 3 * d), rnd(M, d), torch.zeros(3 * d, d, device='cuda')), (rnd(M, d), rnd(M, d), torch.zeros(d, d, device='cuda'))]


units = [unit(k) for k in ('lin2', 'lin1', 'attn', 'lin2', 'lin1', 'attn', 'lin2')]
items = [p for u in units for p in u]
flops = sum(2.0 * M * dy.shape[1] * x.shape[1] for dy, x, _ in items)


def grouped():
    assert ops.gemm_wgrad_group(items), 'the grouped launch declined'


def per_product():
    for u in units:
        if len(u) == 2:
            ops.gemm_wgrad_pair(*u[0], *u[1])
        else:
            ops.gemm_wgrad(*u[0])


arms = [('grouped', grouped), ('per product', per_product)]
if check:
    res = []
    for _, fn in arms:
        for _, _, dw in items:
            dw.zero_()
        fn()
        torch.cuda.synchronize()
        res.append([dw.clone() for _, _, dw in items])
    for k, (a, b) in enumerate(zip(*res)):
        err = float((a - b).abs().max() / b.abs().max())
        assert err < 1e-5, (k, err)
    print('check: the arms agree (max relative deviation of any product below 1e-5)')
for _, fn in arms:
    fn()
torch.cuda.synchronize()
times = [[] for _ in arms]
for _ in range(rounds):
    for i, (_, fn) in enumerate(arms):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times[i].append(e0.elapsed_time(e1) / 5)
print('M = %d, seven units, %d products, %.2f TFLOP' % (M, len(items), flops / 1e12))
print('%-14s %12s %12s %12s %10s' % ('arm', 'median us', 'min us', 'max us', 'TF'))
for (name, _), t in zip(arms, times):
    t = sorted(t)
    med = t[len(t) // 2]
    print('%-14s %12.1f %12.1f %12.1f %10.0f' % (name, med * 1e3, t[0] * 1e3, t[-1] * 1e3, flops / med / 1e9))
