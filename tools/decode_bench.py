#!/usr/bin/env python3
"""A/B of the decoding step inside ONE process: the torch path of m3p_amd/decoder.py (fp32 copy of the logits, log_softmax,
topk over beam * V columns, index_select of every layer's caches, the source expanded per beam: decoder.VOCAB_SELECT_MAX_K = 0)
against the select path (csrc/select.hip on the bf16 logits, caches in place behind cache['owner'], the source once per
sentence), on the cfg2 decoder geometry - 12 layers / 768 wide / 12 heads, V = 250 002, S = 164 source rows - with seeded
weights, the <EOS> bias pushed far down so that no sentence ends early, early_stopping = False, max_len = 64:
    generate_beam  32 sentences x beam 4
    generate_beam  64 sentences x beam 5
    generate       128 sentences, greedy
Every run is warmed up on both paths, then timed in three alternating pairs with device events around a window that ends in
a synchronise; ms per decoding step = window / (max_len - 1).  The outputs of the two paths on the timed inputs are compared
(tokens and lengths) and every sentence that differs is reported.  It fails without a GPU.
    timeout -k 10 900 python tools/decode_bench.py > profiles/decode_select_vs_torch.txt
Kernel shares come from a run of its own under the profiler, select path only (the timings above are taken with it off):
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/decode_bench.py --trace beam4
    python tools/decode_bench.py --stats <dir>/.../*_kernel_stats.csv beam4 >> profiles/decode_select_vs_torch.txt
which gives the selection kernels' achieved bytes/s (bytes = n * V * 2 per step, counted here) against the HBM peak, and the
share of the summed KERNEL time (not of the step's wall time: host gaps between launches are not in it) that goes to
kernels other than the project's own, with the largest of those listed.  The round-2 form of this tool (one shape from the
command line, host clock; it wrote profiles/r02_decode_bench.txt) is the file as of the commit named in that profile.

`--sample` measures the sampled step instead: generate(sample_temperature=1.0) on 128 sentences through torch (fp32 copy of
the logits, divide, softmax, torch.multinomial on torch's generator) against generate(sample_temperature=1.0, sample_seed=...)
(csrc/select.hip: m3p_vocab_sample on the bf16 logits), same geometry, warm-up and pairs.  The two draw different words (two
random streams), so outputs are not compared; the device route stands on reproducibility, the number gates nothing.
    timeout -k 10 600 python tools/decode_bench.py --sample > profiles/decode_sample_vs_torch.txt
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/decode_bench.py --trace sample
    python tools/decode_bench.py --stats <dir>/.../*_kernel_stats.csv sample >> profiles/decode_sample_vs_torch.txt

`--sample --top-p P` measures the nucleus cut instead: generate(sample_seed=...) against generate(sample_seed=...,
sample_top_p=P) (csrc/select.hip: m3p_vocab_nucleus_sample), both on the device - the parent of the cut has no device top-p,
seeded sampling without it is the fair neighbour.  Same geometry, warm-up and pairs; `--trace nucleus --top-p P` is the run
for the profiler, `--stats ... nucleus` its per-kernel lines.
    timeout -k 10 600 python tools/decode_bench.py --sample --top-p 0.9 > profiles/decode_nucleus.txt

`--constraints` measures the decoding constraints (csrc/constrain.hip: m3p_logits_constrain in front of the selection kernels)
with no_repeat_ngram = 3, repetition_penalty = 1.2, min_len = 8 on greedy x 128 and beam 4 x 32: (a) the device route with the
constraints against the same route without them - the difference is the kernel's cost per step, launch included -, (b) the
device route against the fallback route (decoder.VOCAB_SELECT_MAX_K = 0: the torch twin on the fp32 scores in front of
log_softmax / topk), both with the constraints, outputs compared (for beam search with the score gap at which the two
selections part on the same constrained logits, as in the plain run).  Same geometry, warm-up and pairs.  `--trace greedy
--constraints` (or beam4) is the run for the profiler, `--stats ... greedy` then lists lc_constrain_kernel beside the selection
kernels.  The constraints-off path is not timed against its parent: it issues no launch (tests/test_logit_constraints.py).
    timeout -k 10 900 python tools/decode_bench.py --constraints > profiles/decode_constraints.txt

`--sample --top-k K [--top-p P]` measures seeded sampling over more than 16 candidates (csrc/select.hip: m3p_vocab_sample_wide):
(a) generate(sample_seed=..., sample_top_k=K[, sample_top_p=P]) on the device against the fallback route of the same call in
the same process (decoder.VOCAB_SELECT_MAX_K = 0: an fp32 copy of the logits, a device-to-host read and the NumPy twin of
m3p_amd/rng.py - the code this call ran before the kernels existed, as long as rng.py and decoder._sample_twin are untouched);
the fallback takes seconds per step, so its runs decode FALLBACK_LEN - 1 steps, and both sides are reported in ms per step.
(b) without --top-p, the device route's neighbours: ms per step at top_k = 0 and 16 (the routes of m3p_vocab_sample) beside K
and 1024.  Same geometry, 128 sentences, warm-up and three alternating pairs.  `--trace wide --top-k K [--top-p P]` is the run
for the profiler, `--stats ... wide` its per-kernel lines.
    timeout -k 10 900 python tools/decode_bench.py --sample --top-k 50 > profiles/decode_topk_wide.txt
    timeout -k 10 900 python tools/decode_bench.py --sample --top-k 50 --top-p 0.9 >> profiles/decode_topk_wide.txt

`--beam B --sentences N` measures ONE beam-search shape instead of the three runs above - generate_beam on N sentences x beam B,
the shapes beyond 8 beams that csrc/select.hip takes through m3p_vocab_select_wide (17 <= 2 B <= 64) - by the protocol of the
plain run: the device route against the torch route of the same call in the same process (decoder.VOCAB_SELECT_MAX_K = 0, the
code this call ran before the wide entry existed), warm-up on both, three alternating pairs, outputs and selections compared.
The run is named beamB: `--beam B --sentences N --trace beamB` is the run for the profiler, `--beam B --sentences N --stats
<csv> beamB` its per-kernel lines (vs_chunk_kernel, the six launches of the count selection, vsb_merge_kernel).
    timeout -k 10 600 python tools/decode_bench.py --beam 12 --sentences 32 > profiles/decode_beam_wide.txt
    timeout -k 10 600 python tools/decode_bench.py --beam 32 --sentences 16 >> profiles/decode_beam_wide.txt

`--hyps` measures the hypothesis bookkeeping of generate_beam on the select path: decoder.BEAM_HYPS_ON_DEVICE = False (one host
copy of the candidates per step, decoder.beam_advance_host, three small uploads, the gather of `generated`, advance_owner)
against True (csrc/beam.hip: ba_advance_kernel, one launch per step, one host read per call), on 32 sentences x beam 4, 64 x
beam 5 and 16 x beam 32 - or, with `--beam B --sentences N`, on that one shape.  Same geometry, warm-up and three alternating
pairs; afterwards the two routes' n_best = beam lists (tokens, lengths, fp64 scores) are compared for equality.  The switch is
the module constant, so `--hyps host` / `--hyps device` in front of any other beam-search run of this tool pin it for that run
(`--hyps host --beam 4 --sentences 32` is the run to set beside the same command in a checkout of the parent commit).
    timeout -k 10 600 python tools/decode_bench.py --hyps > profiles/decode_beam_device_hyps.txt"""
import csv
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from m3p_amd import decoder, synth   # noqa: E402

D, HEADS, LAYERS, V, S, MAX_LEN = 768, 12, 12, 250002, 164, 64
RUNS = {'beam4': ('generate_beam', 32, 4), 'beam5': ('generate_beam', 64, 5), 'greedy': ('generate', 128, 1)}
SAMPLE = ('sample', 128, 1)       # the --sample run: T = 1.0, seeded device route against torch.multinomial
SAMPLE_SEED = 17
TOP_P = [0.9]                     # --top-p: the nucleus of the `nucleus` runs
TOP_K = [0]                       # --top-k: the candidates of the `wide` runs (0: not given)
FALLBACK_LEN = 3                  # max_len of the fallback runs of --top-k: two decoding steps of seconds each
CONSTRAINTS = dict(no_repeat_ngram=3, repetition_penalty=1.2, min_len=8)      # the --constraints runs
PAIRS = 3
HBM_PEAK = 8.0e12               # bytes/s of an MI355X (HBM3E)


def model():
    from m3p_amd.model.transformer import TransformerModel
    P = synth.model_params(D, HEADS, LAYERS, V, n_dec_layers=LAYERS, n_langs=2, id2lang={0: 'en', 1: 'zh'}, lang2id={'en': 0, 'zh': 1})
    torch.manual_seed(0)
    m = TransformerModel(P, is_encoder=False, with_output=True, is_crossModal=True).cuda().eval()
    with torch.no_grad():
        m.pred_layer.proj.bias[synth.EOS] = -1e4          # nobody stops early: every run decodes max_len - 1 steps
    return m


def inputs(bs):
    g = torch.Generator(device='cuda').manual_seed(bs)
    src = torch.randn(bs, S, D, device='cuda', generator=g)
    src_len = torch.randint(S // 2, S + 1, (bs,), device='cuda', generator=g)
    src_len[0] = S
    return src, src_len


def call(m, kind, src, src_len, beam, **cons):
    with torch.no_grad():
        if kind == 'generate':
            return m.generate(src, src_len, 1, max_len=MAX_LEN, **cons)
        if kind == 'sample':
            return m.generate(src, src_len, 1, max_len=MAX_LEN, sample_temperature=1.0, sample_seed=SAMPLE_SEED)
        if kind == 'nucleus':
            return m.generate(src, src_len, 1, max_len=MAX_LEN, sample_temperature=1.0, sample_seed=SAMPLE_SEED, sample_top_p=TOP_P[0])
        if kind == 'wide':
            return m.generate(src, src_len, 1, sample_temperature=1.0, sample_seed=SAMPLE_SEED, **cons)
        if kind == 'sample_torch':
            return m.generate(src, src_len, 1, max_len=MAX_LEN, sample_temperature=1.0)
        return m.generate_beam(src, src_len, 1, beam, 1.0, False, max_len=MAX_LEN, **cons)


def timed(fn, max_len=MAX_LEN):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (max_len - 1), out


def with_rule(rule, fn):
    saved = decoder.VOCAB_SELECT_MAX_K
    decoder.VOCAB_SELECT_MAX_K = rule
    try:
        return fn()
    finally:
        decoder.VOCAB_SELECT_MAX_K = saved


def differing(a, b):
    """Sentences whose tokens or lengths differ between two (tokens (len, bs), lengths (bs)) results."""
    (ta, la), (tb, lb) = a, b
    out = []
    for s in range(la.shape[0]):
        n = int(la[s])
        if int(lb[s]) != n or not torch.equal(ta[:n, s], tb[:n, s]):
            out.append(s)
    return out


def selection_gaps(m, src, src_len, beam, **cons):
    """Where do the two selections part?  One generate_beam on the select path; at every step the torch selection
    (log_softmax of the fp32 logits + beam_scores, topk) is taken from the SAME logits.  The hidden states of the two paths
    are bit-identical up to a sentence's first differing selection, so that step is where its outputs part.  -> per sentence
    that ever differs: (sentence, step, |torch score of torch's entry - torch score of the kernel's entry|) at the first
    differing rank of its first differing step."""
    real, step, first = decoder._select, [0], {}

    def both(logits, V_, beam_scores, beam_, k, *route):
        res = real(logits, V_, beam_scores, beam_, k, *route)
        t = (torch.log_softmax(logits[:, :V_].float(), dim=-1) + beam_scores[:, None]).view(-1, beam_ * V_)
        _, ti = torch.topk(t, k, dim=1, largest=True, sorted=True)
        for s in (ti != res[1]).any(1).nonzero().view(-1).tolist():
            if s not in first:
                j = int((ti[s] != res[1][s]).nonzero()[0])
                first[s] = (step[0], abs(float(t[s, ti[s, j]]) - float(t[s, res[1][s, j]])))
        step[0] += 1
        return res
    decoder._select = both
    try:
        call(m, 'generate_beam', src, src_len, beam, **cons)
    finally:
        decoder._select = real
    return sorted((s, st, g) for s, (st, g) in first.items())


def bench(m):
    print('decoding step, %d layers, d = %d, V = %d, S = %d, max_len = %d; ms per decoding step, %d alternating pairs; '
          'ratio = torch / select' % (LAYERS, D, V, S, MAX_LEN, PAIRS))
    rule = decoder.VOCAB_SELECT_MAX_K
    for name, (kind, bs, beam) in RUNS.items():
        src, src_len = inputs(bs)
        one = lambda: call(m, kind, src, src_len, beam)   # noqa: E731
        with_rule(0, one)                                  # warm-up of every shape on both paths
        with_rule(rule, one)
        old, new = [], []
        for _ in range(PAIRS):
            t, out_old = timed(lambda: with_rule(0, one))
            old.append(t)
            t, out_new = timed(lambda: with_rule(rule, one))
            new.append(t)
        ratios = [a / b for a, b in zip(old, new)]
        rows = bs * beam
        print('%-6s %-13s bs %3d beam %2d (%3d rows)  torch ms %s  select ms %s  ratio %s  select %s' % (
            name, kind, bs, beam, rows, ' '.join('%7.3f' % v for v in old), ' '.join('%7.3f' % v for v in new),
            ' '.join('%5.2f' % v for v in ratios), 'wins all three' if min(ratios) > 1 else 'does NOT win all three'))
        assert out_old[0].shape[0] == MAX_LEN and out_new[0].shape[0] == MAX_LEN, 'a sentence ended early'
        diff = differing(out_old, out_new)
        print('       outputs on the timed inputs: %d of %d sentences differ between the paths%s' % (
            len(diff), bs, (' ' + str(diff)) if diff else ''))
        print('       bytes of logits per step (n * V * 2): %.1f MB' % (rows * V * 2 / 1e6))
        if kind == 'generate_beam':
            gaps = selection_gaps(m, src, src_len, beam)
            print('       selections on the same logits (kernel against log_softmax + topk): %d of %d sentences see a different '
                  'list at some step; score gap at the first difference: max %.3g%s' % (
                      len(gaps), bs, max([g for _, _, g in gaps] or [0.0]),
                      ''.join('\n         sentence %d step %d gap %.3g' % e for e in gaps)))


HYPS_RUNS = (('beam4', 32, 4), ('beam5', 64, 5), ('beam32', 16, 32))


def with_hyps(flag, fn):
    saved = decoder.BEAM_HYPS_ON_DEVICE
    decoder.BEAM_HYPS_ON_DEVICE = flag
    try:
        return fn()
    finally:
        decoder.BEAM_HYPS_ON_DEVICE = saved


def bench_hyps(m, runs):
    print('hypothesis bookkeeping of generate_beam on the select path, %d layers, d = %d, V = %d, S = %d, max_len = %d; ms per '
          'decoding step, %d alternating pairs; ratio = host / device (BEAM_HYPS_ON_DEVICE False / True)' % (
              LAYERS, D, V, S, MAX_LEN, PAIRS))
    for name, bs, beam in runs:
        src, src_len = inputs(bs)
        one = lambda: call(m, 'generate_beam', src, src_len, beam)   # noqa: E731
        with_hyps(False, one)                                      # warm-up of the shape on both routes
        with_hyps(True, one)
        host, dev = [], []
        for _ in range(PAIRS):
            t, out_host = timed(lambda: with_hyps(False, one))
            host.append(t)
            t, out_dev = timed(lambda: with_hyps(True, one))
            dev.append(t)
        ratios = [a / b for a, b in zip(host, dev)]
        print('%-6s generate_beam bs %3d beam %2d (%3d rows)  host ms %s  device ms %s  ratio %s  difference us per step %s  device %s' % (
            name, bs, beam, bs * beam, ' '.join('%7.3f' % v for v in host), ' '.join('%7.3f' % v for v in dev),
            ' '.join('%5.3f' % v for v in ratios), ' '.join('%6.1f' % (1e3 * (a - b)) for a, b in zip(host, dev)),
            'wins all three' if min(ratios) > 1 else 'does NOT win all three'))
        assert out_host[0].shape[0] == MAX_LEN and out_dev[0].shape[0] == MAX_LEN, 'a sentence ended early'
        full = {flag: with_hyps(flag, lambda: call(m, 'generate_beam', src, src_len, beam, n_best=beam, return_scores=True))
                for flag in (False, True)}
        same = all(torch.equal(a, b) for a, b in zip(full[False], full[True]))
        print('       n_best = %d lists of the two routes (tokens, lengths, fp64 scores) equal: %s; default outputs equal: %s' % (
            beam, same, all(torch.equal(a, b) for a, b in zip(out_host, out_dev))))


def bench_sample(m):
    kind, bs, beam = SAMPLE
    print('sampled decoding step (T = 1.0), %d layers, d = %d, V = %d, S = %d, max_len = %d, %d sentences; ms per decoding step, '
          '%d alternating pairs; ratio = torch / seeded' % (LAYERS, D, V, S, MAX_LEN, bs, PAIRS))
    src, src_len = inputs(bs)
    torch.manual_seed(0)
    call(m, 'sample_torch', src, src_len, beam)              # warm-up of both routes
    call(m, 'sample', src, src_len, beam)
    old, new = [], []
    for _ in range(PAIRS):
        t, out_old = timed(lambda: call(m, 'sample_torch', src, src_len, beam))
        old.append(t)
        t, out_new = timed(lambda: call(m, 'sample', src, src_len, beam))
        new.append(t)
    ratios = [a / b for a, b in zip(old, new)]
    assert out_old[0].shape[0] == MAX_LEN and out_new[0].shape[0] == MAX_LEN, 'a sentence ended early'
    print('sample generate       bs %3d          (%3d rows)  torch ms %s  seeded ms %s  ratio %s  the seeded route %s' % (
        bs, bs, ' '.join('%7.3f' % v for v in old), ' '.join('%7.3f' % v for v in new), ' '.join('%5.2f' % v for v in ratios),
        'is faster in all three pairs' if min(ratios) > 1 else 'is SLOWER than torch in at least one pair'))
    again = call(m, 'sample', src, src_len, beam)
    print('       a further seeded run gives the same tokens: %s' % torch.equal(again[0], out_new[0]))
    print('       bytes of logits per step (n * V * 2): %.1f MB' % (bs * V * 2 / 1e6))


def bench_nucleus(m):
    _, bs, beam = SAMPLE
    print('sampled decoding step (T = 1.0), %d layers, d = %d, V = %d, S = %d, max_len = %d, %d sentences; ms per decoding step, '
          '%d alternating pairs; seeded sampling on the device without and with top_p = %g; ratio = with / without' % (
              LAYERS, D, V, S, MAX_LEN, bs, PAIRS, TOP_P[0]))
    src, src_len = inputs(bs)
    call(m, 'sample', src, src_len, beam)                    # warm-up of both routes
    call(m, 'nucleus', src, src_len, beam)
    old, new = [], []
    for _ in range(PAIRS):
        t, out_old = timed(lambda: call(m, 'sample', src, src_len, beam))
        old.append(t)
        t, out_new = timed(lambda: call(m, 'nucleus', src, src_len, beam))
        new.append(t)
    assert out_old[0].shape[0] == MAX_LEN and out_new[0].shape[0] == MAX_LEN, 'a sentence ended early'
    print('nucleus generate      bs %3d          (%3d rows)  seeded ms %s  top-p ms %s  ratio %s' % (
        bs, bs, ' '.join('%7.3f' % v for v in old), ' '.join('%7.3f' % v for v in new),
        ' '.join('%5.2f' % (b / a) for a, b in zip(old, new))))
    again = call(m, 'nucleus', src, src_len, beam)
    print('       a further top-p run gives the same tokens: %s' % torch.equal(again[0], out_new[0]))
    print('       bytes of logits per step (n * V * 2): %.1f MB' % (bs * V * 2 / 1e6))


def bench_wide(m):
    _, bs, beam = SAMPLE
    K, P = TOP_K[0], TOP_P[0]
    print('sampled decoding step (T = 1.0), %d layers, d = %d, V = %d, S = %d, %d sentences; ms per decoding step, %d alternating '
          'pairs; seeded sampling with top_k = %d%s' % (LAYERS, D, V, S, bs, PAIRS, K, '' if P is None else ', top_p = %g' % P))
    src, src_len = inputs(bs)
    kw = dict(sample_top_k=K, sample_top_p=P)
    dev = lambda: call(m, 'wide', src, src_len, beam, max_len=MAX_LEN, **kw)                              # noqa: E731
    fall = lambda n: with_rule(0, lambda: call(m, 'wide', src, src_len, beam, max_len=n, **kw))           # noqa: E731
    dev()                                                    # warm-up of both routes
    fall(2)
    old, new = [], []
    for _ in range(PAIRS):
        t, out_old = timed(lambda: fall(FALLBACK_LEN), FALLBACK_LEN)
        old.append(t)
        t, out_new = timed(dev)
        new.append(t)
    ratios = [a / b for a, b in zip(old, new)]
    assert out_old[0].shape[0] == FALLBACK_LEN and out_new[0].shape[0] == MAX_LEN, 'a sentence ended early'
    print('(a) top_k %4d%s  bs %3d (%3d rows)  fallback ms %s (max_len %d)  device ms %s (max_len %d)  ratio %s  the device route %s' % (
        K, '' if P is None else ' top_p %g' % P, bs, bs, ' '.join('%9.1f' % v for v in old), FALLBACK_LEN,
        ' '.join('%7.3f' % v for v in new), MAX_LEN, ' '.join('%7.1f' % v for v in ratios),
        'wins all three' if min(ratios) > 1 else 'does NOT win all three'))
    print('    the fallback is decoder.VOCAB_SELECT_MAX_K = 0 in this process: rng.sample_words on a host copy of the fp32 scores')
    drawn = FALLBACK_LEN - 1                                 # (the fallback's last position is the forced <EOS>)
    same = int((out_old[0][:drawn] == out_new[0][:drawn]).all(0).sum())
    print('    drawn positions the two runs share: %d; the routes agree there in %d of %d sentences' % (drawn - 1, same, bs))
    again = dev()
    print('    a further device run gives the same tokens: %s' % torch.equal(again[0], out_new[0]))
    print('    bytes of logits per step (n * V * 2): %.1f MB' % (bs * V * 2 / 1e6))
    if P is not None:
        return
    ks = sorted(set((0, 16, K, 1024)))
    runs = {k: (lambda k=k: call(m, 'wide', src, src_len, beam, max_len=MAX_LEN, sample_top_k=k or None)) for k in ks}
    for k in ks:
        runs[k]()
    ms = {k: [] for k in ks}
    for _ in range(PAIRS):
        for k in ks:
            ms[k].append(timed(runs[k])[0])
    for k in ks:
        route = 'm3p_vocab_sample' if k <= 16 else 'm3p_vocab_sample_wide'
        print('(b) top_k %4d  %-22s device ms %s' % (k, route, ' '.join('%7.3f' % v for v in ms[k])))
    print('    the wide route against the narrow one at 16: %s us per step more at top_k %d, %s at 1024' % (
        ' '.join('%6.1f' % (1e3 * (a - b)) for a, b in zip(ms[K], ms[16])), K,
        ' '.join('%6.1f' % (1e3 * (a - b)) for a, b in zip(ms[1024], ms[16]))))


def bench_constraints(m):
    print('decoding constraints %s, %d layers, d = %d, V = %d, S = %d, max_len = %d; ms per decoding step, %d alternating pairs' % (
        CONSTRAINTS, LAYERS, D, V, S, MAX_LEN, PAIRS))
    rule = decoder.VOCAB_SELECT_MAX_K
    for name in ('greedy', 'beam4'):
        kind, bs, beam = RUNS[name]
        src, src_len = inputs(bs)
        plain = lambda: call(m, kind, src, src_len, beam)                          # noqa: E731
        cons = lambda: call(m, kind, src, src_len, beam, **CONSTRAINTS)            # noqa: E731
        plain()                                                                    # warm-up of the three routes
        cons()
        with_rule(0, cons)
        off, on, on_b, fall = [], [], [], []
        for _ in range(PAIRS):
            off.append(timed(plain)[0])
            t, out_on = timed(cons)
            on.append(t)
        for _ in range(PAIRS):
            t, out_fall = timed(lambda: with_rule(0, cons))
            fall.append(t)
            t, out_on = timed(lambda: with_rule(rule, cons))
            on_b.append(t)
        assert out_on[0].shape[0] == MAX_LEN and out_fall[0].shape[0] == MAX_LEN, 'a sentence ended early'
        fmt = lambda v: ' '.join('%7.3f' % x for x in v)                            # noqa: E731
        print('%-6s %-13s bs %3d beam %d (%3d rows)' % (name, kind, bs, beam, bs * beam))
        print('       (a) device route: without constraints ms %s  with ms %s  difference us per step %s' % (
            fmt(off), fmt(on), ' '.join('%6.1f' % (1e3 * (b - a)) for a, b in zip(off, on))))
        print('       (b) with constraints: fallback route ms %s  device route ms %s  ratio %s' % (
            fmt(fall), fmt(on_b), ' '.join('%5.2f' % (a / b) for a, b in zip(fall, on_b))))
        diff = differing(out_fall, out_on)
        print('       outputs of the two routes on the timed inputs: %d of %d sentences differ%s' % (
            len(diff), bs, (' ' + str(diff)) if diff else ''))
        if kind == 'generate_beam':
            gaps = selection_gaps(m, src, src_len, beam, **CONSTRAINTS)
            print('       selections on the same constrained logits (kernel against log_softmax + topk): %d of %d sentences see a '
                  'different list at some step; score gap at the first difference: max %.3g' % (
                      len(gaps), bs, max([g for _, _, g in gaps] or [0.0])))


def trace(m, name, cons=None):
    kind, bs, beam = (name,) + SAMPLE[1:] if name in ('nucleus', 'wide') else SAMPLE if name == 'sample' else RUNS[name]
    src, src_len = inputs(bs)
    cons = cons or {}
    if name == 'wide':
        cons = dict(max_len=MAX_LEN, sample_top_k=TOP_K[0], sample_top_p=TOP_P[0])
    call(m, kind, src, src_len, beam, **cons)
    torch.cuda.synchronize()
    t, _ = timed(lambda: call(m, kind, src, src_len, beam, **cons))
    print('%s%s under the profiler: %.3f ms per step (slower than the timed runs: tracing)' % (
        name, ' with constraints' if cons else '', t))


def own_kernel(kname):
    """Is this a kernel of libm3p_hip.so?  They all live in a top-level anonymous namespace: the demangled name starts with
    '(anonymous namespace)::' (behind an optional 'void '), the mangled one with '_ZN12_GLOBAL__N_1'.  Most torch kernels
    carry an anonymous namespace too, but inside at::native:: or in a template argument - never in front."""
    k = kname.strip()
    if k.startswith('void '):
        k = k[5:]
    if k.startswith('_ZN12_GLOBAL__N_1'):
        return True
    pre = '(anonymous namespace)::'
    if not k.startswith(pre):
        return False
    own_name = k[len(pre):].split('<')[0].split('(')[0]       # the kernel's own name, in front of template and call arguments
    return '::' not in own_name


def stats(path, name):
    """Kernel shares of a `--trace NAME` run from rocprofv3's kernel stats (Name, Calls, TotalDurationNs, ...): shares of
    the summed KERNEL time, not of the step's wall time (host gaps between launches are in neither term)."""
    kind, bs, beam = SAMPLE if name in ('sample', 'nucleus', 'wide') else RUNS[name]
    rows = bs * beam
    total = own = 0.0
    sel, others = {}, []
    for r in csv.DictReader(open(path)):
        ns, calls, kname = float(r['TotalDurationNs']), int(r['Calls']), r['Name']
        total += ns
        if own_kernel(kname):
            own += ns
        else:
            others.append((ns, calls, kname))
        for key in ('vs_chunk_kernel', 'vs_merge_kernel', 'vsmp_chunk_kernel', 'vsmp_merge_kernel', 'vsmp_topk_kernel',
                    'vnuc_coarse_kernel', 'vnuc_scan_kernel', 'vnuc_fine_kernel', 'vnuc_cut_kernel', 'vnuc_merge_kernel',
                    'lc_constrain_kernel', 'vsw_coarse_kernel', 'vsw_scan_kernel', 'vsw_tie_kernel', 'vsw_compact_kernel',
                    'vsw_draw_kernel', 'vsb_merge_kernel'):
            if key in kname:
                sel[key] = (ns / calls, calls)
    print('\nkernel shares, %s (%d rows), %s, from a profiled run of its own (warm-up + one timed run)' % (
        name, rows, {'sample': 'seeded sampling', 'nucleus': 'seeded nucleus sampling',
                     'wide': 'seeded sampling over more than 16 candidates'}.get(name, 'select path')))
    for key, (avg, calls) in sorted(sel.items()):
        print('  %-18s %5d calls  %8.1f us per call' % (key, calls, avg / 1e3))
    if name == 'wide':
        every = sum(avg * calls for avg, calls in sel.values()) / max(v[1] for k, v in sel.items() if k == 'vsw_draw_kernel')
        print('  wide sampling (all of the above, vsw_scan_kernel twice): %.1f us per step over %.1f MB of logits read four times' % (
            every / 1e3, rows * V * 2 / 1e6))
    elif 'vsb_merge_kernel' in sel:
        every = sum(avg * calls for avg, calls in sel.values()) / sel['vsb_merge_kernel'][1]
        print('  wide beam selection (all of the above, vsw_scan_kernel twice): %.1f us per step over %.1f MB of logits read five '
              'times' % (every / 1e3, rows * V * 2 / 1e6))
    elif name == 'nucleus':
        every = sum(v[0] for v in sel.values())
        print('  nucleus sampling (all of the above): %.1f us per step over %.1f MB of logits' % (every / 1e3, rows * V * 2 / 1e6))
    elif len(sel) - ('lc_constrain_kernel' in sel) == 2:
        both = sum(v[0] for k, v in sel.items() if k != 'lc_constrain_kernel')
        bps = rows * V * 2 / (both * 1e-9)
        print('  selection (both kernels): %.1f us per step for %.1f MB of logits = %.2f TB/s, %.0f %% of the %.1f TB/s HBM peak' % (
            both / 1e3, rows * V * 2 / 1e6, bps / 1e12, 100 * bps / HBM_PEAK, HBM_PEAK / 1e12))
    print('  kernel time outside the project\'s kernels: %.1f %% of %.1f ms of kernel time (host gaps between launches are not '
          'kernel time and are in neither figure)' % (100 * (total - own) / total, total / 1e6))
    print('  the largest kernels counted as NOT the project\'s (check the classification by eye):')
    for ns, calls, kname in sorted(others, reverse=True)[:8]:
        print('    %6.2f %%  %6d calls  %s' % (100 * ns / total, calls, kname[:150]))


if __name__ == '__main__':
    if '--beam' in sys.argv:
        at = sys.argv.index('--beam')
        one_beam = int(sys.argv[at + 1])
        del sys.argv[at:at + 2]
        assert '--sentences' in sys.argv, '--beam B --sentences N'
        at = sys.argv.index('--sentences')
        one_bs = int(sys.argv[at + 1])
        del sys.argv[at:at + 2]
        assert one_beam >= 1 and one_bs >= 1
        RUNS.clear()
        RUNS['beam%d' % one_beam] = ('generate_beam', one_bs, one_beam)
    if len(sys.argv) >= 4 and sys.argv[1] == '--stats':
        stats(sys.argv[2], sys.argv[3])
        sys.exit(0)
    assert torch.cuda.is_available(), 'decode_bench.py measures on a GPU'
    if '--hyps' in sys.argv:
        at = sys.argv.index('--hyps')
        pin = sys.argv[at + 1] if len(sys.argv) > at + 1 and sys.argv[at + 1] in ('host', 'device') else None
        del sys.argv[at:at + (2 if pin else 1)]
        if pin is None:
            print(torch.cuda.get_device_name(0))
            bench_hyps(model(), [(n, bs, beam) for n, (_, bs, beam) in RUNS.items()] if len(RUNS) == 1 else HYPS_RUNS)
            sys.exit(0)
        decoder.BEAM_HYPS_ON_DEVICE = pin == 'device'
        print('decoder.BEAM_HYPS_ON_DEVICE = %s' % decoder.BEAM_HYPS_ON_DEVICE)
    constrained = '--constraints' in sys.argv
    if constrained:
        sys.argv.remove('--constraints')
        if len(sys.argv) == 1:
            print(torch.cuda.get_device_name(0))
            bench_constraints(model())
            sys.exit(0)
    if '--top-k' in sys.argv:
        at = sys.argv.index('--top-k')
        TOP_K[0] = int(sys.argv[at + 1])
        del sys.argv[at:at + 2]
        assert 16 < TOP_K[0] <= 1024, '--top-k K: 16 < K <= 1024 (up to 16 is the route of --sample)'
        if '--top-p' not in sys.argv:
            TOP_P[0] = None
    if '--top-p' in sys.argv:
        at = sys.argv.index('--top-p')
        TOP_P[0] = float(sys.argv[at + 1])
        del sys.argv[at:at + 2]
        assert 0.0 < TOP_P[0] < 1.0, '--top-p P: 0 < P < 1'
        if len(sys.argv) >= 2 and sys.argv[1] == '--sample' and not TOP_K[0]:
            print(torch.cuda.get_device_name(0))
            bench_nucleus(model())
            sys.exit(0)
    if TOP_K[0] and len(sys.argv) >= 2 and sys.argv[1] == '--sample':
        print(torch.cuda.get_device_name(0))
        bench_wide(model())
        sys.exit(0)
    if len(sys.argv) >= 3 and sys.argv[1] == '--trace':
        trace(model(), sys.argv[2], CONSTRAINTS if constrained else None)
    elif len(sys.argv) >= 2 and sys.argv[1] == '--sample':
        print(torch.cuda.get_device_name(0))
        bench_sample(model())
    else:
        print(torch.cuda.get_device_name(0))
        bench(model())
