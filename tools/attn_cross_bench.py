#!/usr/bin/env python3
"""A/B of the attention over a source encoding in a teacher-forced decoder pass inside ONE process: the rows kernels
(csrc/decode.hip, a wave per query, dk / dv through fp32 atomics) against the tiled MFMA kernels (csrc/attn_tiled.hip, source mask),
forward + backward as functional.DecoderFn runs each branch (the rows branch with its zeroed fp32 dkv buffer and the cast to
bf16), p = 0.1, H = 12, dh = 64, ragged key counts uniform on [S / 2, S], three alternating pairs per shape, device events.
Then the self-attention pair (rows against the causal kernels of csrc/attn_tiled.hip) at the seq2seq shapes, and one mt_step / ic_step of the
12-layer / 768-d / V = 250 002 model with the dispatch constants of functional.py forced to 10^9 (rows: the code path before
the tiled kernels) and to 0 (tiled).  The constants the grid supports - the simplest rule Tq >= a and S >= b under which every
selected shape won all three alternations - are printed at the end; tests/test_seq2seq_tiled.py compares functional.py's
with them.
    timeout -k 10 600 python tools/attn_cross_bench.py > profiles/attn_cross_vs_rows.txt"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from m3p_amd import functional as Fn, ops, synth   # noqa: E402

H, DH, P_DROP, SEED = 12, 64, 0.1, 4242
TQS, SS = (8, 32, 64, 256), (36, 100, 256, 512)
SELF_SHAPES = [(64, 32), (64, 64), (32, 256)]
PAIRS, REPS = 3, 3
BF16 = torch.bfloat16


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


def alternate(a, b, reps):
    ra, rb = [], []
    for _ in range(PAIRS):
        ra.append(timed(a, reps))
        rb.append(timed(b, reps))
    return ra, rb


def cross_grid():
    d = H * DH
    qscale = 1.0 / np.sqrt(DH)
    print('attention over a source encoding, forward + backward, H = %d, dh = %d, p = %.1f, klen uniform on [S/2, S]; ms per pair of '
          'launches (mean of %d), %d alternations; ratio = rows / tiled' % (H, DH, P_DROP, REPS, PAIRS))
    won = {}
    for Tq in TQS:
        for S in SS:
            B = min(256, 8192 // Tq)
            g = torch.Generator(device='cuda').manual_seed(7)
            q = (torch.randn(B * Tq, d, device='cuda', generator=g) * qscale).to(BF16)
            kv = torch.randn(B, S, 2 * d, device='cuda', generator=g).to(BF16)
            dctx = torch.randn(B * Tq, d, device='cuda', generator=g).to(BF16)
            klen = torch.randint(S // 2, S + 1, (B,), device='cuda', generator=g).to(torch.int32)

            def rows():
                _, lse = ops.attn_rows_fwd(q, kv, klen, B, Tq, H, DH, S, seed=SEED, p_drop=P_DROP)
                _, dkv = ops.attn_rows_bwd(q, kv, klen, dctx, lse, B, Tq, H, DH, S, qscale, seed=SEED, p_drop=P_DROP)
                dkv.to(BF16)

            def tiled():
                _, lse = ops.attn_cross_fwd(q, kv, klen, B, Tq, H, DH, S, seed=SEED, p_drop=P_DROP)
                ops.attn_cross_bwd(q, kv, klen, dctx, lse, B, Tq, H, DH, S, qscale, seed=SEED, p_drop=P_DROP)

            r, t = alternate(rows, tiled, REPS)
            ratios = [a / b for a, b in zip(r, t)]
            won[(Tq, S)] = min(ratios) > 1
            print('cross  B %4d  Tq %4d  S %4d  rows ms %s  tiled ms %s  tiled wins %d/3  ratio %s' % (
                B, Tq, S, ' '.join('%8.3f' % v for v in r), ' '.join('%8.3f' % v for v in t), sum(x > 1 for x in ratios),
                ' '.join('%7.2f' % v for v in ratios)))
    return won


def self_pairs():
    d = H * DH
    qscale = 1.0 / np.sqrt(DH)
    print('\ncausal self-attention of the same pass, forward + backward, rows against the causal kernels of csrc/attn_tiled.hip')
    ok = True
    for B, T in SELF_SHAPES:
        g = torch.Generator(device='cuda').manual_seed(7)
        qkv = torch.randn(B * T, 3 * d, device='cuda', generator=g)
        qkv[:, :d] *= qscale
        qkv = qkv.to(BF16)
        dctx = torch.randn(B * T, d, device='cuda', generator=g).to(BF16)
        kv = qkv.view(B, T, 3 * d)[:, :, d:]

        def rows():
            _, lse = ops.attn_rows_fwd(qkv, kv, None, B, T, H, DH, T, causal=True, seed=SEED, p_drop=P_DROP)
            dqkv = torch.empty_like(qkv)
            _, dkv = ops.attn_rows_bwd(qkv, kv, None, dctx, lse, B, T, H, DH, T, qscale, causal=True, seed=SEED, p_drop=P_DROP, dq_out=dqkv)
            dqkv.view(B, T, 3 * d)[:, :, d:] = dkv

        def tiled():
            _, lse = ops.attn_causal_fwd(qkv, B, T, H, DH, seed=SEED, p_drop=P_DROP)
            ops.attn_causal_bwd(qkv, dctx, lse, B, T, H, DH, qscale, seed=SEED, p_drop=P_DROP)

        r, t = alternate(rows, tiled, REPS)
        ratios = [a / b for a, b in zip(r, t)]
        ok = ok and min(ratios) > 1
        print('self   B %4d  T  %4d          rows ms %s  tiled ms %s  tiled wins %d/3  ratio %s' % (
            B, T, ' '.join('%8.3f' % v for v in r), ' '.join('%8.3f' % v for v in t), sum(x > 1 for x in ratios),
            ' '.join('%7.2f' % v for v in ratios)))
    print('the tiled causal pair %s every alternation at the seq2seq shapes' % ('wins' if ok else 'does NOT win'))


def force(value):
    Fn.CAUSAL_TILED_MIN_T = Fn.CROSS_TILED_MIN_TQ = Fn.CROSS_TILED_MIN_S = value


def steps():
    from m3p_amd.model.transformer import TransformerModel
    from m3p_amd.trainer import XTrainer
    V = 250002
    P = synth.model_params(768, 12, 12, V, dropout=0.1, attention_dropout=0.1, n_langs=2, id2lang={0: 'en', 1: 'zh'},
                           lang2id={'en': 0, 'zh': 1}, mt_steps=[('en', 'zh')], encoder_only=True)
    for k, v in synth.trainer_params(batch_size=32, langs=['en', 'zh'], ft_lgs=[]).items():
        setattr(P, k, v)
    torch.manual_seed(0)
    m = TransformerModel(P, is_encoder=True, with_output=True, is_crossModal=True).cuda()
    tr = XTrainer(m, {}, P)
    rs = np.random.RandomState(1)

    def sentences(T, B):
        return torch.from_numpy(rs.randint(3, V - 1, size=(T, B))).long(), torch.full((B,), T, dtype=torch.long)

    x1, len1 = sentences(256, 32)
    x2, len2 = sentences(256, 32)
    c2, clen2 = sentences(32, 64)
    x_img = torch.from_numpy(rs.standard_normal((64, 100, 2048)).astype(np.float32))
    loc = torch.from_numpy(rs.uniform(0, 1, size=(64, 100, 5)).astype(np.float32))
    img_mask = torch.ones((64, 100), dtype=torch.long)
    saved = (Fn.CAUSAL_TILED_MIN_T, Fn.CROSS_TILED_MIN_TQ, Fn.CROSS_TILED_MIN_S)
    cases = (('mt_step_on_batch, B = 32, T = S = 256', lambda: tr.mt_step_on_batch(x1, len1, x2, len2, 'en', 'zh', 1.0)),
             ('ic_step_on_batch, B = 64, 100 regions, T = 32', lambda: tr.ic_step_on_batch(c2, clen2, x_img, img_mask, loc, 'coco', 'img', 1.0)))
    print('\nsteps, 12 layers, d = 768, V = %d, dropout 0.1; ms per step (mean of 3), %d alternations; the dispatch constants forced' % (V, PAIRS))
    for name, one in cases:
        r, t = [], []
        for _ in range(PAIRS):
            force(10 ** 9)
            r.append(timed(one, 3))
            force(0)
            t.append(timed(one, 3))
        ratios = [a / b for a, b in zip(r, t)]
        print('%s' % name)
        print('    constants = 10^9 (rows)  %s' % ' '.join('%8.2f' % v for v in r))
        print('    constants = 0 (tiled)    %s' % ' '.join('%8.2f' % v for v in t))
        print('    rows / tiled             %s   tiled %s' % (' '.join('%7.2fx' % v for v in ratios),
                                                             'wins all three' if min(ratios) > 1 else 'does NOT win all three'))
    Fn.CAUSAL_TILED_MIN_T, Fn.CROSS_TILED_MIN_TQ, Fn.CROSS_TILED_MIN_S = saved


def rule(won):
    """The simplest rule the grid supports: thresholds (a, b) from the measured lengths with every selected shape a
    three-fold win, selecting as many shapes as possible (ties: the smaller thresholds)."""
    best = None
    for a in TQS:
        for b in SS:
            sel = [k for k in won if k[0] >= a and k[1] >= b]
            if all(won[k] for k in sel) and (best is None or len(sel) > best[0]):
                best = (len(sel), a, b)
    print('\nthe rule the grid supports (tiled where Tq >= CROSS_TILED_MIN_TQ and S >= CROSS_TILED_MIN_S; %d of %d measured shapes):' % (
        best[0] if best else 0, len(won)))
    if best is None:
        print('none: the tiled kernels win all three alternations nowhere')
        return
    print('CROSS_TILED_MIN_TQ = %d' % best[1])
    print('CROSS_TILED_MIN_S = %d' % best[2])


if __name__ == '__main__':
    print(torch.cuda.get_device_name(0))
    won = cross_grid()
    self_pairs()
    steps()
    rule(won)
