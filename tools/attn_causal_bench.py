#!/usr/bin/env python3
"""A/B of the causal self-attention of a decoder-only pass inside ONE process: the rows kernels (csrc/decode.hip, a wave per
query, dk / dv through fp32 atomics) against the tiled MFMA kernels (csrc/attn_tiled.hip, causal mask), forward + backward as
functional.DecoderFn runs each branch (the rows branch with its zeroed fp32 dkv buffer and the copy into dqkv), p = 0.1,
H = 12, dh = 64, three alternating pairs per shape, device events.  Then one clm_step of the 12-layer / 768-d / V = 250 002
model at B = 32, T = 256 with functional.CAUSAL_TILED_MIN_T forced to 0 (tiled) and to 10^9 (rows).
    timeout -k 10 600 python tools/attn_causal_bench.py > profiles/attn_causal_vs_rows.txt && ..."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from m3p_amd import functional as Fn, ops, synth   # noqa: E402

H, DH, P_DROP, SEED = 12, 64, 0.1, 4242
SHAPES = [(256, 32), (128, 64), (64, 128), (32, 256), (16, 512)]
PAIRS, REPS = 3, 5


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
    qscale = 1.0 / np.sqrt(DH)
    print('forward + backward, H = %d, dh = %d, p = %.1f; ms per pair of launches (mean of %d), %d alternations' % (H, DH, P_DROP, REPS, PAIRS))
    print('%-12s %-32s %-32s %s' % ('(B, T)', 'rows ms', 'tiled ms', 'rows / tiled per alternation'))
    for B, T in SHAPES:
        g = torch.Generator(device='cuda').manual_seed(7)
        qkv = torch.randn(B * T, 3 * d, device='cuda', generator=g)
        qkv[:, :d] *= qscale
        qkv = qkv.to(torch.bfloat16)
        dctx = torch.randn(B * T, d, device='cuda', generator=g).to(torch.bfloat16)
        kv = qkv.view(B, T, 3 * d)[:, :, d:]

        def rows():
            _, lse = ops.attn_rows_fwd(qkv, kv, None, B, T, H, DH, T, causal=True, seed=SEED, p_drop=P_DROP)
            dqkv = torch.empty_like(qkv)
            _, dkv = ops.attn_rows_bwd(qkv, kv, None, dctx, lse, B, T, H, DH, T, qscale, causal=True, seed=SEED, p_drop=P_DROP, dq_out=dqkv)
            dqkv.view(B, T, 3 * d)[:, :, d:] = dkv

        def tiled():
            _, lse = ops.attn_causal_fwd(qkv, B, T, H, DH, seed=SEED, p_drop=P_DROP)
            ops.attn_causal_bwd(qkv, dctx, lse, B, T, H, DH, qscale, seed=SEED, p_drop=P_DROP)

        r, t = [], []
        for _ in range(PAIRS):
            r.append(timed(rows, REPS))
            t.append(timed(tiled, REPS))
        ratios = [a / b for a, b in zip(r, t)]
        print('%-12s %-32s %-32s %s   tiled %s' % ((B, T), ' '.join('%8.3f' % v for v in r), ' '.join('%8.3f' % v for v in t),
                                                   ' '.join('%6.2fx' % v for v in ratios),
                                                   'wins all three' if min(ratios) > 1 else 'does NOT win all three'))


def step():
    from m3p_amd.model.transformer import TransformerModel
    from m3p_amd.trainer import XTrainer
    B, T, V = 32, 256, 250002
    P = synth.model_params(768, 12, 12, V, dropout=0.1, attention_dropout=0.1)
    for k, v in synth.trainer_params(batch_size=B, clm_steps=[('en', None)], context_size=0).items():
        setattr(P, k, v)
    torch.manual_seed(0)
    m = TransformerModel(P, is_encoder=True, with_output=True, is_crossModal=True).cuda()
    tr = XTrainer(m, {}, P)
    rs = np.random.RandomState(1)
    x = torch.from_numpy(rs.randint(3, V - 1, size=(T, B))).long()
    lengths = torch.full((B,), T, dtype=torch.long)
    alen = torch.arange(T)
    pred_mask = alen[:, None] < lengths[None] - 1
    y = x[1:].masked_select(pred_mask[:-1])

    def one():
        tr.clm_step_on_batch(x, lengths, pred_mask, y, 'en', 1.0)

    print('\nclm_step, 12 layers, d = 768, V = %d, B = %d, T = %d (8192 tokens), dropout 0.1; ms per step (mean of 3), %d alternations' % (
        V, B, T, PAIRS))
    r, t = [], []
    for _ in range(PAIRS):
        Fn.CAUSAL_TILED_MIN_T = 10 ** 9
        r.append(timed(one, 3))
        Fn.CAUSAL_TILED_MIN_T = 0
        t.append(timed(one, 3))
    print('CAUSAL_TILED_MIN_T = 10^9 (rows)  %s' % ' '.join('%8.2f' % v for v in r))
    print('CAUSAL_TILED_MIN_T = 0 (tiled)    %s' % ' '.join('%8.2f' % v for v in t))
    print('rows / tiled                      %s' % ' '.join('%7.2fx' % (a / b) for a, b in zip(r, t)))


if __name__ == '__main__':
    print(torch.cuda.get_device_name(0))
    kernels()
    step()
