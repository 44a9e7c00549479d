#!/usr/bin/env python3
"""Validation scoring head at cfg2's head size (4864 prediction rows, d = 768, V = 250 002): ``predict_stats`` against the only
route to the same numbers without it - ``predict(get_scores=True)`` + ``max(1)[1] == y`` + two ``.item()`` reads, what the
reference's evaluators do per batch.  Seeded inputs, both paths in one process, alternated in three pairs, device events,
every shape warmed up first, windows of a few hundred milliseconds.

  python tools/eval_head_bench.py                 the A/B
  python tools/eval_head_bench.py --kernel-only   a few launches of ce_eval_kernel alone, for a kernel trace
                                                  (rocprofv3 --kernel-trace --stats -- python tools/eval_head_bench.py --kernel-only)
  python tools/eval_head_bench.py --kernel-time-us T   achieved bytes/s of the kernel from its traced time
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from m3p_amd import ops, synth  # noqa: E402

N_ROWS, D, V = 4864, 768, 250002
HBM_PEAK = 8.0e12


def kernel_bytes(ld):
    """What the scoring pass has to move: every logit once (targets and outputs are noise beside it)."""
    return N_ROWS * ld * 2


def kernel_only():
    ld = (V + 255) // 256 * 256
    gen = torch.Generator(device='cuda').manual_seed(1)
    logits = (torch.randn((N_ROWS, ld), generator=gen, device='cuda') * 2).to(torch.bfloat16)
    y = torch.randint(0, V, (N_ROWS,), generator=gen, device='cuda')
    for _ in range(12):
        ops.ce_eval(logits, V, y)
    torch.cuda.synchronize()
    print('ce_eval_kernel launched 12 times on %d x %d (ld %d): %.3f GB per launch' % (N_ROWS, V, ld, kernel_bytes(ld) / 1e9))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernel-only', action='store_true')
    ap.add_argument('--kernel-time-us', type=float, default=None)
    ap.add_argument('--window-ms', type=float, default=400.0)
    args = ap.parse_args()
    if args.kernel_time_us is not None:
        ld = (V + 255) // 256 * 256
        rate = kernel_bytes(ld) / (args.kernel_time_us * 1e-6)
        print('ce_eval_kernel: %.1f us for %.3f GB -> %.2f TB/s, %.0f %% of the 8 TB/s HBM bound' % (
            args.kernel_time_us, kernel_bytes(ld) / 1e9, rate / 1e12, 100 * rate / HBM_PEAK))
        return
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    if args.kernel_only:
        return kernel_only()
    from m3p_amd.model.transformer import TransformerModel
    torch.manual_seed(0)
    P = synth.model_params(D, 12, 1, V)
    m = TransformerModel(P, is_encoder=True, with_output=True, is_crossModal=True).cuda().eval()
    gen = torch.Generator(device='cuda').manual_seed(2)
    T, B = 19, 256
    assert T * B == N_ROWS
    tensor = torch.randn((T, B, D), generator=gen, device='cuda').to(torch.bfloat16)
    pred_mask = torch.ones((T, B), dtype=torch.bool, device='cuda')
    y = torch.randint(3, V, (N_ROWS,), generator=gen, device='cuda')

    def new_path():
        return m.predict_stats(tensor, pred_mask, y)

    def old_path():
        scores, loss = m('predict', tensor=tensor, pred_mask=pred_mask, y=y, get_scores=True)
        return loss.item() * len(y), (scores.max(1)[1] == y).sum().item()

    def timed(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters, out

    with torch.no_grad():
        for _ in range(3):                      # warm-up of every shape either path launches
            new_path(), old_path()
        ms_new, out_new = timed(new_path, 5)
        ms_old, out_old = timed(old_path, 5)
        it_new, it_old = (max(5, math.ceil(args.window_ms / ms)) for ms in (ms_new, ms_old))
        print('rows %d, d %d, V %d; windows of %d / %d calls' % (N_ROWS, D, V, it_new, it_old))
        pairs = []
        for k in range(3):
            a, out_new = timed(new_path, it_new)
            b, out_old = timed(old_path, it_old)
            pairs.append((a, b))
            print('pair %d: predict_stats %.3f ms   predict(get_scores) + max + 2 x item %.3f ms   ratio %.2f' % (k, a, b, b / a))
    xe_new, ok_new = float(out_new[0]), int(out_new[1])
    xe_old, ok_old = out_old
    print('loss sums %.4f / %.4f (relative difference %.2e), hits %d / %d' % (xe_new, xe_old, abs(xe_new - xe_old) / abs(xe_old),
                                                                              ok_new, ok_old))
    a = sorted(p[0] for p in pairs)[1]
    b = sorted(p[1] for p in pairs)[1]
    print('median: predict_stats %.3f ms, old route %.3f ms, %.2f x' % (a, b, b / a))


if __name__ == '__main__':
    main()
