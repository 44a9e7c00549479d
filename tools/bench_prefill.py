#!/usr/bin/env python3
"""A/B of the prefill of a prompted decoding call inside ONE process: the rows kernel (csrc/decode.hip: m3p_attn_query_fwd,
a wave per (sequence, head, query)) against the prefix mask of the tiled MFMA forward (csrc/attn_tiled.hip:
m3p_attn_prefix_fwd).
  1. the attention alone at B = 32, H = 12, dh = 64, pos0 = 0, Tq in {8, 16, 32, 64, 128, 256}: three alternating pairs per
     shape, device events; decoder.PREFILL_TILED_MIN_T is the smallest Tq from which the tiled kernel wins every pair;
  2. generate() with a 256-word prompt on the 12-layer / 768-d / V = 250 002 decoder, bs = 32, 8 free steps behind the prompt,
     with the route on (PREFILL_TILED_MIN_T as shipped) and off (0): three alternating pairs, host clock around calls that
     end in a device synchronise.
    timeout -k 10 600 python tools/bench_prefill.py > profiles/decode_prefill.txt"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from m3p_amd import decoder, ops, synth   # noqa: E402

B, H, DH = 32, 12, 64
TQS = [8, 16, 32, 64, 128, 256]
PAIRS, REPS = 3, 500


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernels():
    d = H * DH
    print('attention alone, B = %d, H = %d, dh = %d, pos0 = 0; ms per launch (mean of %d), %d alternations' % (B, H, DH, REPS, PAIRS))
    print('%-6s %-30s %-30s %s' % ('Tq', 'rows ms', 'tiled ms', 'rows / tiled per alternation'))
    wins = {}
    for Tq in TQS:
        g = torch.Generator(device='cuda').manual_seed(7)
        q = (torch.randn(B * Tq, d, device='cuda', generator=g) / np.sqrt(DH)).to(torch.bfloat16)
        kv = torch.randn(B, max(Tq, 64), 2 * d, device='cuda', generator=g).to(torch.bfloat16)
        out = (torch.empty((B * Tq, d), dtype=torch.bfloat16, device='cuda'), torch.empty((B, H, Tq), dtype=torch.float32, device='cuda'))

        def rows():
            ops.attn_query_fwd(q, kv, None, B, Tq, H, DH, Tq, causal=True, pos0=0)

        def tiled():
            assert ops.attn_prefix_fwd(q, kv, B, Tq, H, DH, 0, out=out) is not None

        a = ops.attn_query_fwd(q, kv, None, B, Tq, H, DH, Tq, causal=True, pos0=0).float()
        b = ops.attn_prefix_fwd(q, kv, B, Tq, H, DH, 0)[0].float()
        rel = float((a - b).norm() / a.norm())
        assert rel < 6e-3, rel
        r, t = [], []
        for _ in range(PAIRS):
            r.append(timed(rows, REPS))
            t.append(timed(tiled, REPS))
        ratios = [x / y for x, y in zip(r, t)]
        wins[Tq] = min(ratios) > 1
        print('%-6d %-30s %-30s %s   tiled %s   (rel. L2 between the two: %.2g)' % (
            Tq, ' '.join('%8.4f' % v for v in r), ' '.join('%8.4f' % v for v in t), ' '.join('%6.2fx' % v for v in ratios),
            'wins all three' if wins[Tq] else 'does NOT win all three', rel))
    from_on = [Tq for i, Tq in enumerate(TQS) if all(wins[u] for u in TQS[i:])]
    print('smallest measured Tq from which the tiled kernel wins every pair at every larger measured Tq: %s '
          '(decoder.PREFILL_TILED_MIN_T = %d)' % (from_on[0] if from_on else 'none', decoder.PREFILL_TILED_MIN_T))


def generate():
    from m3p_amd.model.transformer import TransformerModel
    bs, V, n_prompt, free = 32, 250002, 256, 8
    P = synth.model_params(768, 12, 1, V, n_dec_layers=12)
    torch.manual_seed(0)
    m = TransformerModel(P, is_encoder=False, with_output=True, is_crossModal=True).cuda()
    m.eval()
    rs = np.random.RandomState(1)
    prefix = torch.from_numpy(rs.randint(3, V - 1, size=(n_prompt, bs))).long().cuda()
    plen = torch.full((bs,), n_prompt, dtype=torch.long, device='cuda')
    max_len = 1 + n_prompt + free + 1
    shipped = decoder.PREFILL_TILED_MIN_T

    def one():
        with torch.no_grad():
            out = m.generate(None, None, None, max_len=max_len, prefix=prefix, prefix_len=plen)
        torch.cuda.synchronize()
        return out

    def clock(reps=10):
        one()
        t0 = time.perf_counter()
        for _ in range(reps):
            one()
        return (time.perf_counter() - t0) / reps * 1e3

    decoder.PREFILL_TILED_MIN_T = shipped
    on = one()
    decoder.PREFILL_TILED_MIN_T = 0
    off = one()
    n = min(on[0].shape[0], off[0].shape[0])
    same = float((on[0][:n] == off[0][:n]).float().mean())
    print('\ngenerate(), decoder-only, 12 layers, d = 768, V = %d, bs = %d, %d-word prompt, max_len = %d (prefill of %d positions + '
          '%d steps); ms per call (mean of 10), %d alternations' % (V, bs, n_prompt, max_len, 1 + n_prompt, free + 1, PAIRS))
    r, t = [], []
    for _ in range(PAIRS):
        decoder.PREFILL_TILED_MIN_T = 0
        r.append(clock())
        decoder.PREFILL_TILED_MIN_T = shipped
        t.append(clock())
    print('PREFILL_TILED_MIN_T = 0 (rows)     %s' % ' '.join('%8.2f' % v for v in r))
    print('PREFILL_TILED_MIN_T = %-3d (tiled)  %s' % (shipped, ' '.join('%8.2f' % v for v in t)))
    print('rows / tiled                      %s' % ' '.join('%7.2fx' % (a / b) for a, b in zip(r, t)))
    print('tokens equal on both routes: %.1f %% (randomly initialised weights: near-ties are common)' % (100 * same))


if __name__ == '__main__':
    print(torch.cuda.get_device_name(0))
    kernels()
    generate()
