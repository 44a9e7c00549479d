#!/usr/bin/env python3
"""A/B of the vocabulary weight gradient that also sums the output-bias gradient's columns (m3p_gemm_wgrad_bias_bf16)
against what it replaces, inside ONE process (see tools/ab_wgrad_group.py), at the benchmark's shape: e bf16 [n, V_pad],
hs bf16 [n, d], dE fp32 [V_pad, d] stored, w fp32 [n].
  wgrad       m3p_gemm_wgrad_store_bf16 alone (what both arms share)
  now         the same launch + m3p_ce_shift_colsum (tile pass, fold and memset: a pass of its own over e)
  new         m3p_gemm_wgrad_bias_bf16 alone
The arms alternate; the median of the rounds is reported, then what the column sums cost in either form (arm - wgrad) and the
stop rule of the change: the new form is wired into the step only below a third of the present one.  With --check the arms
must agree: dE bit for bit, the sums to fp32 accumulation error of their absolute sums.
    python tools/ab_vocab_wgrad_bias.py [--check] [--rounds 9]        (AB_N, AB_V, AB_D: default 4864, 250112, 768)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from m3p_amd import ops   # noqa: E402

check = '--check' in sys.argv
rounds = int(sys.argv[sys.argv.index('--rounds') + 1]) if '--rounds' in sys.argv else 9
n = int(os.environ.get('AB_N', '4864'))
V_pad = int(os.environ.get('AB_V', '250112'))
d = int(os.environ.get('AB_D', '768'))
V = V_pad - 110                  # pad columns: exact zeros, as the projection leaves them
bf = torch.bfloat16

torch.manual_seed(5)
e = torch.empty((n, V_pad), dtype=bf, device='cuda')
for r0 in range(0, n, 256):      # exp(logit - shift): positive, a few decades wide
    e[r0:r0 + 256] = torch.exp(2.0 * torch.randn(256, V_pad, device='cuda') - 4.0).to(bf)
e[:, V:] = 0
hs = (torch.randn(n, d, device='cuda') * 1e-3).to(bf)
w = torch.exp(torch.randn(n, device='cuda')) / n
dE = [torch.zeros((V_pad, d), device='cuda') for _ in range(2)]
bsum = torch.empty(V_pad, device='cuda')
out = {}


def wgrad():
    ops.gemm_wgrad(e, hs, dE[0], n=V_pad, k=d, dw_is_zero=True)


def now():
    ops.gemm_wgrad(e, hs, dE[0], n=V_pad, k=d, dw_is_zero=True)
    out['now'] = ops.ce_shift_colsum(e, w)


def new():
    assert ops.gemm_wgrad_bias(e, hs, dE[1], w, bsum, n=V_pad, k=d, store=True), 'the launcher declined the whole-tile schedule'
    out['new'] = bsum


arms = [('wgrad', wgrad), ('now', now), ('new', new)]
if check:
    bsum.fill_(float('nan'))
    now()
    new()
    torch.cuda.synchronize()
    assert torch.equal(dE[0], dE[1]), 'dE differs between the arms'
    a, b = out['now'].double(), out['new'].double()
    # positive terms: a sum is its own absolute sum.  Two fp32 accumulations of n terms, and the new arm's weights are
    # rounded to bf16: at most 2^-8 of every term
    err = float((a - b).abs().max())
    assert bool(((a - b).abs() <= (16 * n ** 0.5 * 2.0 ** -24 + 2.0 ** -8) * b.abs()).all()), err
    assert bool((b[V:] == 0).all())
    print('check: dE bit-identical, column sums agree (largest difference %.3g of a largest sum of %.3g)' % (err, float(b.abs().max())))
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
print('n = %d, V_pad = %d, d = %d' % (n, V_pad, d))
print('%-8s %12s %12s %12s' % ('arm', 'median us', 'min us', 'max us'))
med = {}
for (name, _), t in zip(arms, times):
    t = sorted(t)
    med[name] = t[len(t) // 2] * 1e3
    print('%-8s %12.1f %12.1f %12.1f' % (name, med[name], t[0] * 1e3, t[-1] * 1e3))
cost_now, cost_new = med['now'] - med['wgrad'], med['new'] - med['wgrad']
print('column sums: %.1f us as a pass of their own, %.1f us inside the weight gradient (%.2f of it; the change is wired in below 0.33)'
      % (cost_now, cost_new, cost_new / cost_now))
