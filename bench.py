#!/usr/bin/env python3
"""Headline benchmark: M3P pre-training sequences/s (BASELINE.json metric) on 1..8 MI355X.

    python bench.py --gpus 1 --steps 20 --warmup 5
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W
    python bench.py --gpus N ...        (no launcher: re-executes itself under torch.distributed.run, N ranks)

One step = XTrainer.pretrain_under_step on a synthetic, device-resident batch of
BASELINE.json configs[1] (12L/768d/12h, 36 regions + 128 tokens, V=250002, 19 masked
tokens/sequence, ITM BCE, dropout 0.1, adam_inverse_sqrt + clip 5, bf16 compute with fp32
master weights): jointfwd -> MLM + ITM losses -> backward (+ bucketed RCCL all-reduce for
N>1) -> clip -> Adam.  Weak scaling: the per-GPU batch is fixed.
Prints ONE JSON line on rank 0 (contract in the task statement).  A plain run sets up, pre-warms, runs the
--warmup steps, times the --steps steps and prints the headline (sequences/s, ms_per_step).  --full adds the
measurements beside it, each at the cost of events or extra steps:
  roofline     the dominant MFMA GEMM timed live with HIP events on its own stream (+ the sustained clock, 5 extra steps)
  also.cfg3    the same step at 1024 sequences per GPU (default configuration only)
  cpu_baseline the oracle (plain PyTorch fp32 CPU restatement) on the host cores, bounded sample
  comm         N > 1: exposed collective wait and per-collective bus bandwidth (3 extra steps)
--dump-outputs DIR writes what the last timed step computed as DIR/<name>.npy (dump_outputs below).
"""
import argparse
import json
import os
os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')   # dmabuf IPC for RCCL across processes
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0   # MI355X dense bf16 MFMA peak (MI355X_MICROARCH.md; 2:1-sparse figure excluded)
PEAK_FP8_TFLOPS = 5000.0    # dense fp8 MFMA peak (same source)


def flops_train_per_seq(d, L, T, R, V, n_pred):
    """forward MACs = R(2048d+5d) + L[S(4d^2+2d*4d)+2S^2 d] + n_pred*d*V + d^2+d;
    train FLOPs = 6 x MACs."""
    S = T + R
    macs = R * (2048 * d + 5 * d) + L * (S * (4 * d * d + 2 * d * 4 * d) + 2 * S * S * d) + n_pred * d * V + d * d + d
    return 6.0 * macs


def build(cfg, dropout, world, rank, local_rank, refine_layers=0, ragged=False, fp8=False, lr='0.0001', wrapped=None):
    from m3p_amd import synth
    from m3p_amd.model.transformer import TransformerModel
    from m3p_amd.trainer import XTrainer
    P = synth.model_params(cfg['emb_dim'], cfg['n_heads'], cfg['n_layers'], cfg['n_words'], dropout=dropout,
                           attention_dropout=dropout, refine_layers=refine_layers)
    for k, v in dict(optimizer='adam_inverse_sqrt,beta1=0.9,beta2=0.98,lr=%s' % lr, clip_grad_norm=5, amp=1, fp16=True,
                     accumulate_gradients=1, multi_gpu=(world > 1) if wrapped is None else wrapped, local_rank=local_rank, epoch_size=100000,
                     cross_mlm_steps=[('google', 'img')], cross_mrm_steps=[], cross_mrfr_steps=[], cross_clcm_steps=[],
                     sample_n=2, refine_image=refine_layers > 0, multi_cls_loss_weight=0, bin_cls_loss_weight=1,
                     batch_size=cfg['B'], dump_path='/nonexistent_m3p_dump', fp8_gemm=fp8).items():
        setattr(P, k, v)
    torch.manual_seed(1234)   # identical random-init weights on every rank (then broadcast anyway)
    model = TransformerModel(P, is_encoder=True, with_output=True, is_crossModal=True).cuda()
    trainer = XTrainer(model, {}, P)
    batch = synth.make_batch(cfg['T'], cfg['R'], cfg['B'], cfg['n_words'], cfg['n_pred'], seed=1000 + rank, ragged=ragged)
    B, R = cfg['B'], cfg['R']
    dev = torch.device('cuda', local_rank)
    img = batch['x_img'].transpose(0, 1).contiguous().to(dev)           # (n, R, 2048) as the collate emits it
    loc = batch['image_loc'].transpose(0, 1).contiguous().to(dev)
    tup = ((batch['x'].to(dev), batch['lengths'].to(dev), batch['x_labels']),       # labels stay on the host (mask building)
           (img, torch.ones(B, R, dtype=torch.long, device=dev), loc, None, batch['pos_labels'].tolist(), None, None))
    return trainer, tup


def _host_info():
    """(physical cores, logical CPUs, CPU model) of this host."""
    import subprocess
    logical = os.cpu_count() or 1
    model, phys = 'unknown', None
    try:
        txt = subprocess.run(['lscpu'], capture_output=True, text=True, timeout=10).stdout
        kv = {l.split(':', 1)[0].strip(): l.split(':', 1)[1].strip() for l in txt.splitlines() if ':' in l}
        model = kv.get('Model name', model)
        phys = int(kv['Core(s) per socket']) * int(kv['Socket(s)'])
    except Exception:
        pass
    return phys or max(logical // 2, 1), logical, model


def _oracle_steps(cfg, Bs, dropout, threads, warm, timed, budget_s):
    """warm + up to `timed` full training steps of the oracle (fwd + bwd + clip 5 + Adam-inv-sqrt) -> seconds per step."""
    from m3p_amd import synth
    from oracle import ref_cpu as O
    torch.set_num_threads(threads)
    P = synth.model_params(cfg['emb_dim'], cfg['n_heads'], cfg['n_layers'], cfg['n_words'])
    shapes = synth.hot_param_shapes(P)
    gen = torch.Generator().manual_seed(0)
    sd = {k: torch.randn(tuple(s), generator=gen) * 0.02 for k, s in shapes.items()}
    for k in sd:
        if ('layer_norm' in k or 'LayerNorm' in k) and k.endswith('weight'):
            sd[k] += 1
    names = list(sd.keys())
    batch = synth.make_batch(cfg['T'], cfg['R'], Bs, cfg['n_words'], cfg['n_pred'], seed=1000, ragged=False)
    opt = O.AdamInvSqrt([sd[n] for n in names])
    kw = {}
    if dropout > 0:      # same keep probability at every site as the GPU run; masks drawn once (the oracle takes explicit masks)
        S, d, H, L = cfg['T'] + cfg['R'], cfg['emb_dim'], cfg['n_heads'], cfg['n_layers']
        g = torch.Generator().manual_seed(1)
        bern = lambda *shape: torch.rand(shape, generator=g) >= dropout    # noqa: E731
        keeps = {'img': bern(Bs, cfg['R'], d), 'emb': bern(Bs, S, d)}
        for i in range(L):
            keeps[('attn_p', i)] = bern(Bs, H, S, S)
            keeps[('attn_out', i)] = bern(Bs, S, d)
            keeps[('ffn', i)] = bern(Bs, S, d)
        kw = dict(dropout=dropout, attention_dropout=dropout, keeps=keeps)
    for _ in range(warm):
        O.train_step(sd, names, opt, cfg['n_layers'], cfg['n_heads'], batch, cfg['R'], clip=5.0, **kw)
    t0 = time.time()
    n = 0
    while n < timed:
        O.train_step(sd, names, opt, cfg['n_layers'], cfg['n_heads'], batch, cfg['R'], clip=5.0, **kw)
        n += 1
        if time.time() - t0 > budget_s:
            break
    return (time.time() - t0) / n, n


def cpu_baseline(cfg, dropout):
    """The reference path restated (oracle/ref_cpu.py, pinned to the reference by the golden vectors) timed on this
    host's cores, BASELINE.md section 4: the cfg1 step exactly (B = 8) and the cfg2 model at B = 8, dropout as in the
    GPU run, Adam-inv-sqrt + clip 5; threads = the better of {32, all physical cores} on a one-step probe; 3 warm-up
    steps, then 10 timed steps (the big model stops early after ~25 s)."""
    from m3p_amd import synth
    phys, logical, model = _host_info()
    Bs = 8
    probes = {}
    for n in sorted({min(32, phys), phys}):
        probes[n] = _oracle_steps(cfg, Bs, dropout, n, 1, 1, 60.0)[0]
    threads = min(probes, key=probes.get)
    sec, n = _oracle_steps(cfg, Bs, dropout, threads, 2, 10, 25.0)
    c1 = dict(synth.CONFIGS['cfg1'])
    sec1, n1 = _oracle_steps(c1, c1['B'], dropout, min(threads, 16), 3, 10, 10.0)
    return dict(value=round(Bs / sec, 3), unit='sequences/s', cores=threads, kind='port',
                sample='%d timed full train steps (fwd+bwd+clip+Adam, 3 warm-up incl. probe) of the same %dL/%dd V=%d model '
                       'at B=%d, fp32, dropout %.2f (oracle/ref_cpu.py)' % (n, cfg['n_layers'], cfg['emb_dim'], cfg['n_words'], Bs, dropout),
                cfg1=dict(value=round(c1['B'] / sec1, 2), unit='sequences/s', cores=min(threads, 16),
                          sample='%d timed steps of BASELINE configs[0] (2L/128d, 64+10, B=8, V=1000)' % n1),
                host=dict(physical_cores=phys, logical_cpus=logical, cpu_model=model,
                          thread_probe_s_per_step={str(k): round(v, 3) for k, v in probes.items()}))


def also_config(name, dropout, steps):
    """A second, shorter measurement of the same step on another BASELINE preset (one GPU, plain step): pre-warm until two
    3-step groups agree within 2 %, then `steps` timed steps between synchronisations."""
    from m3p_amd import synth
    cfg = dict(synth.CONFIGS[name])
    trainer, tup = build(cfg, dropout, 1, 0, torch.cuda.current_device())

    def group(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n):
            trainer.pretrain_under_step(tup, 'google', 't2i', 'en', 1.0, 1.0, 1.0, 1.0)
            trainer.n_iter += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / n
    prev, groups = group(3), 1
    while groups < 6:
        cur = group(3)
        groups += 1
        stable = abs(cur - prev) <= 0.02 * prev
        prev = cur
        if stable:
            break
    sec = group(steps)
    fl = flops_train_per_seq(cfg['emb_dim'], cfg['n_layers'], cfg['T'], cfg['R'], cfg['n_words'], cfg['n_pred'])
    value = cfg['B'] / sec
    del trainer, tup
    torch.cuda.empty_cache()
    return dict(workload='%s: the same %dL/%dd model and step at %d sequences per GPU' % (name, cfg['n_layers'], cfg['emb_dim'], cfg['B']),
                per_gpu_batch=cfg['B'], steps=steps, prewarm_steps=3 * groups, ms_per_step=round(sec * 1e3, 3),
                value=round(value, 2), unit='sequences/s',
                step_frac=round(value * fl / 1e12 / PEAK_BF16_TFLOPS, 4), step_frac_peak=PEAK_BF16_TFLOPS)


DUMP_BYTES = 48 << 20     # --dump-outputs stays below this (the contract allows 64 MB)


def dump_outputs(path, trainer, loss, rank, multi):
    """--dump-outputs: what the last timed step handed its caller, as <path>/<name>.npy - the step's total loss ('loss'),
    each head's loss ('loss.<stat key>', e.g. 'loss.CMLM-google') and the model's fp32 parameters after the update
    ('param.<name>').  A parameter larger than `cap` elements is sampled at sorted positions drawn from a generator seeded by
    its name (the same positions for every build); `cap` is halved until the whole dump fits in DUMP_BYTES."""
    import zlib
    import numpy as np
    from m3p_amd.trainer import _unwrap
    if multi:       # zero1 keeps the fp32 master of the big matrices on its owner rank: gather it (a collective)
        trainer._sync_master()
    if rank != 0:
        return
    torch.cuda.synchronize()
    os.makedirs(path, exist_ok=True)
    out = {'loss': loss.detach().float().reshape(-1).cpu().numpy()}
    for key, vals in trainer.stats.items():
        if isinstance(vals, list) and vals and torch.is_tensor(vals[-1]):
            out['loss.' + key] = vals[-1].detach().float().reshape(-1).cpu().numpy()
    named = sorted(_unwrap(trainer.model).named_parameters(), key=lambda kv: kv[0])
    cap = 1 << 16
    while 4 * sum(min(p.numel(), cap) for _, p in named) > DUMP_BYTES:
        cap //= 2
    for name, p in named:
        flat = p.detach().reshape(-1)
        if flat.numel() > cap:
            idx = np.sort(np.random.RandomState(zlib.crc32(name.encode())).randint(0, flat.numel(), cap))
            flat = flat[torch.from_numpy(idx).to(flat.device)]
        out['param.' + name] = flat.float().cpu().numpy()
    for name, a in out.items():
        np.save(os.path.join(path, name + '.npy'), a.astype(np.float32))


def _self_launch(args):
    """`python bench.py --gpus N` without a launcher: re-exec under torch.distributed.run, one rank per GPU."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(args.gpus),
           '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.exit(subprocess.call(cmd))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--batch', type=int, default=None, help='sequences per GPU (default: the preset\'s)')
    ap.add_argument('--config', default='cfg2',
                    help='BASELINE.json preset: cfg2 = configs[1] (12L/768d, 256 sequences per GPU; the default N=1 line), '
                         'cfg3 = configs[2] (the same model at 1024 sequences per GPU = global batch 8192 on 8 GPUs), '
                         'cfg4 = configs[3] (24L/1024d, 100 + 256; use --batch 64 --fp8), cfg5 = configs[4] shapes')
    ap.add_argument('--dropout', type=float, default=0.1)
    ap.add_argument('--full', action='store_true',
                    help='also measure what the headline does not need: roofline + sustained clock, the cfg3 line of the default '
                         'configuration, the CPU baseline, and for N > 1 the "comm" block')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write the losses and (sampled) updated parameters of the last timed step as DIR/<name>.npy')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='with --full: skip the CPU baseline')
    ap.add_argument('--instances', action='store_true',
                    help='add "gemm_instances": every GEMM instance of the step with its in-step median time (HIP events of the warm-up steps)')
    ap.add_argument('--no-also', action='store_true', help='with --full: skip the second measurement (cfg3: 1024 sequences per GPU) of the default line')
    ap.add_argument('--ragged', action='store_true',
                    help='text lengths ~ U[T/2, T] with padding (the second throughput run of SURVEY 8d) instead of all = T')
    ap.add_argument('--refine-layers', type=int, default=0,
                    help='AoA refiner layers on the image rows (jointfwd refine_image=True; the reference default is 6). '
                         '0 = the README configuration the headline metric is quoted on')
    ap.add_argument('--fp8', action='store_true',
                    help='encoder-layer projections and their data gradients on the fp8 MFMA GEMM (BASELINE configs[3]; '
                         'needs per-GPU batch x (T + R) to be a multiple of 256, e.g. --config cfg4 --batch 64)')
    args = ap.parse_args()
    # The timed loop needs ONE host thread (it only enqueues kernels; its few CPU tensor ops are tiny), but torch's intra-op
    # pool defaults to every physical core (128 here) and its workers spin after each small host op.  The GPU boxes run this
    # container under a 16-CPU quota (cpu.max 1600000/100000): a pool of 256 turned the 39-ms step into 125-130 ms, and the
    # default 128 is the likeliest reason for the occasional 42-47 ms runs with unchanged kernel times.  A small pool
    # removes the exposure (1-2 threads 38.4 ms, 4-16 threads 38.1 ms on a quiet box).  M3P_BENCH_HOST_THREADS overrides; the
    # CPU baseline sets its own count.
    torch.set_num_threads(int(os.environ.get('M3P_BENCH_HOST_THREADS', '4')))
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        _self_launch(args)

    from m3p_amd import synth, ops
    from m3p_amd.distributed import init_distributed_mode
    import torch.distributed as dist
    # M3P_BENCH_SHARED_GPU=1 (development dry run of the multi-rank path on a one-GPU box): every rank on cuda:0 over gloo;
    # the line it prints says so and is not a measurement
    shared = os.environ.get('M3P_BENCH_SHARED_GPU', '0') != '0'
    if shared:
        os.environ['LOCAL_RANK'] = '0'
    rank, local_rank, world = init_distributed_mode(backend='gloo' if shared else None)
    assert world == args.gpus, 'WORLD_SIZE=%d but --gpus %d' % (world, args.gpus)
    if world > 1:
        assert dist.get_world_size() == world
    # M3P_DP_FORCE=1 under torchrun --nproc-per-node 1 (development): the one rank is wrapped and runs its collectives over
    # RCCL, so the N > 1 code of this file executes on a one-GPU box; the line says so in "parallelism"
    forced = world == 1 and dist.is_initialized()
    multi = world > 1 or forced
    torch.cuda.set_device(local_rank)
    cfg = dict(synth.CONFIGS[args.config])
    if args.batch is not None:
        cfg['B'] = args.batch
    trainer, tup = build(cfg, args.dropout, world, rank, local_rank, args.refine_layers, args.ragged, args.fp8, wrapped=multi)
    dp = trainer.model if multi else None
    if dp is not None:
        dp.uniform_tokens = not args.ragged      # every rank's batch has the same token-row count: no count exchange at all

    last = {}

    def step():
        last['loss'] = trainer.pretrain_under_step(tup, 'google', 't2i', 'en', 1.0, 1.0, 1.0, 1.0).detach()
        trainer.n_iter += 1

    # Pre-warm OUTSIDE the counted warm-up (the engine clock ramps up from idle over a few hundred ms, lazy allocations
    # settle), so that the result does not depend on the caller's --warmup.  A fixed count, so that the step
    # --dump-outputs records is the same step of the same training run every time: 36 steps, where two 3-step groups
    # agree within 2 % after 6-15.
    groups = 12
    for _ in range(3 * groups):
        step()
    torch.cuda.synchronize()

    # --full: the warm-up steps time EVERY GEMM launch with HIP events (on the launch stream) to find the dominant
    # instance; the timed region then brackets only that instance's launches (the events of all ~100
    # GEMMs per step cost 0.9 ms of a 42-ms step).  A plain run records no events.
    profile = args.full or args.instances
    ops.PROFILE = {} if profile else None
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    warm_prof = ops.PROFILE or {}
    # per instance: median launch time x launches - one outlier among the warm-up launches (a first launch, a clock ramp)
    # must not decide which instance the timed region brackets
    def _robust_total(evs):
        ts = sorted(a.elapsed_time(b) for a, b in evs)
        return ts[len(ts) // 2] * len(ts)
    warm_agg = {k: _robust_total(evs) for k, evs in warm_prof.items()}
    # --instances: every GEMM instance of the step with its in-step median launch time (events of the warm-up steps) and rate
    instances = None
    if args.instances:
        instances = []
        for (kind, M_, N_, K_), evs in sorted(warm_prof.items(), key=lambda kv: -warm_agg[kv[0]]):
            ts = sorted(a.elapsed_time(b) for a, b in evs)
            med = ts[len(ts) // 2]
            instances.append(dict(kernel='%s M=%d N=%d K=%d' % (kind, M_, N_, K_), per_step=round(len(ts) / max(args.warmup, 1), 2),
                                  median_us=round(med * 1e3, 1), tflops=round(2.0 * M_ * N_ * K_ / (med * 1e-3) / 1e12, 0)))
    gemm_ms_per_step = sum(warm_agg.values()) / max(args.warmup, 1)
    ops.PROFILE_ONLY = max(warm_agg.items(), key=lambda kv: kv[1])[0] if warm_agg else None
    if dp is not None and args.full:
        dp.exposed_events = []
    if multi:
        dist.barrier()
        torch.cuda.synchronize()
    ops.PROFILE = {} if args.full else None
    t0 = time.perf_counter()
    host_ms = []
    for _ in range(args.steps):
        h0 = time.perf_counter()
        step()
        host_ms.append((time.perf_counter() - h0) * 1e3)      # (time to ENQUEUE a step: the host must stay ahead of the GPU)
    torch.cuda.synchronize()
    if multi:
        dist.barrier()
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    prof, ops.PROFILE = ops.PROFILE, None
    if multi:
        t = torch.tensor([dt], device='cuda', dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if args.dump_outputs:      # before any further step changes the model
        dump_outputs(args.dump_outputs, trainer, last['loss'], rank, multi)
    comm = None
    if multi and args.full:
        evs = dp.exposed_events or []
        exposed = [a.elapsed_time(b) for a, b, _, _ in evs]
        payload = [n for _, _, n, _ in evs]
        # the exposed tail, split: until the exchange stream has finished the GRADIENT buckets (an event recorded there right in
        # front of the token-row gather) against everything behind it (the token-row gather + the scatter of the gathered rows)
        grad_tail = [max(a.elapsed_time(t), 0.0) if t is not None else None for a, b, _, t in evs]
        grad_tail = [min(g, x) for g, x in zip(grad_tail, exposed) if g is not None]
        e = torch.tensor([sum(exposed) / max(len(exposed), 1)], device='cuda', dtype=torch.float64)
        dist.all_reduce(e, op=dist.ReduceOp.MAX)
        # per-collective bus bandwidth: three more steps with every collective bracketed by events on the side stream
        dp.exposed_events = None
        dp.reducer.timings = []
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        fam = {}
        for label, a, b, nbytes, kind in dp.reducer.timings:
            if isinstance(label, tuple) and label[0] == 'params':
                name = 'params ' + (label[1] if isinstance(label[1], str) else 'layer')
            else:
                name = 'layer' if isinstance(label, tuple) else str(label)
            ms = a.elapsed_time(b)
            ent = fam.setdefault('%s (%s)' % (name, kind), [0, 0.0, 0.0])
            ent[0] += 1; ent[1] += nbytes; ent[2] += ms
        dp.reducer.timings = None
        # Which side of SURVEY section 5's two bounds a collective lands on tells which algorithm RCCL picked: a RING moves
        # (N-1)/N of the bytes over ONE xGMI link per hop (~153 GB/s per direction), a DIRECT exchange spreads them over all N-1
        # links at once (an all-reduce = reduce-scatter + all-gather: twice that).
        XGMI_LINK_GBPS = 153.0

        def _bounds(name, nbytes):
            f = (2.0 if 'allreduce' in name else 1.0) * (world - 1) / max(world, 1)
            ring = f * nbytes / (XGMI_LINK_GBPS * 1e9) * 1e3
            direct = ring / max(world - 1, 1)
            return ring, direct
        buckets = {}
        for k, v in fam.items():
            if v[2] <= 0:
                continue
            mb, ms = v[1] / v[0], v[2] / v[0]
            ring, direct = _bounds(k, mb)
            side = 'n/a (one rank)' if world == 1 else ('direct-like' if ms < (ring * direct) ** 0.5 else ('ring-like' if ms < 1.5 * ring else 'slower than a ring'))
            buckets[k] = dict(MB=round(mb / 1e6, 2), ms=round(ms, 3),
                              busbw_GBps=round(v[1] * ((2.0 if 'allreduce' in k else 1.0) * (world - 1) / world) / (v[2] * 1e-3) / 1e9, 1),
                              ring_bound_ms=round(ring, 3), direct_bound_ms=round(direct, 3), lands=side)
        g_tail = torch.tensor([sum(grad_tail) / max(len(grad_tail), 1)], device='cuda', dtype=torch.float64)
        dist.all_reduce(g_tail, op=dist.ReduceOp.MAX)
        ident = dp.identify()       # (collective: every rank is here)
        comm = dict(mode=dp.mode, exposed_ms_per_step=round(float(e.item()), 3),
                    exposed_split_ms=dict(gradient_buckets=round(float(g_tail.item()), 3),
                                          token_rows=round(max(float(e.item()) - float(g_tail.item()), 0.0), 3)),
                    backend=ident['backend'], ranks=ident['ranks'], rccl_ranks_seen=ident['devices_seen'],
                    nccl_env={k: v for k, v in os.environ.items() if k.startswith(('NCCL_', 'RCCL_')) and 'DEBUG' not in k},
                    payload_MB_per_step=round(sum(payload) / max(len(payload), 1) / 1e6, 1), buckets=buckets,
                    reserved_cus=__import__('m3p_amd.distributed', fromlist=['x']).reserve_cus(),
                    note='exposed = compute-stream wait for the gradient collectives + token-row scatter before clip/Adam '
                         '(max over ranks); payload = bytes handed to RCCL per rank and step in backward (gradient buckets '
                         'fp32, token rows bf16 with their ids in eight extra columns: one gather); exposed_split_ms = that wait up to the end of the gradient buckets on the '
                         'exchange stream / the token-row gather + scatter behind it; rccl_ranks_seen = distinct devices among the ranks (all-gather of device tags); '
                         'buckets = average size / time / bus bandwidth per collective with the ring and direct bounds of SURVEY section 5 (153 GB/s per xGMI link) and which one it lands by, measured on '
                         'rank 0 in three extra steps with each collective bracketed by events; zero1 gathers the updated '
                         'bf16 working copy during the next forward (the "params" rows; the fp32-read vectors travel in one packed all-reduce)')

    # sustained engine clock under this very workload: amdsmi's sclk (torch.cuda.clock_rate()) sampled from a host thread
    # every 2 ms over five more steps AFTER the timed region (the sampler never runs inside it).  The 2.5 PF of the roofline
    # is the matrix peak at the 2.4 GHz ceiling; clock x 256 CUs x 4096 FLOP/clk is what the chip could do at the clock its
    # power budget actually let it hold (MI355X_MICROARCH.md, DVFS section)
    clock = None
    if rank == 0 and not multi and args.full:
        import threading
        samples, stop = [], threading.Event()

        def _sample():
            while not stop.is_set():
                try:
                    samples.append(torch.cuda.clock_rate())
                except Exception:      # (no amdsmi on this box: the block is simply absent)
                    return
                time.sleep(0.002)
        th = threading.Thread(target=_sample, daemon=True)
        th.start()
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        stop.set()
        th.join(timeout=2)
        if len(samples) >= 10:
            s_mhz = sorted(samples)
            clock = dict(sclk_ghz_mean=round(sum(samples) / len(samples) / 1e3, 3), sclk_ghz_median=round(s_mhz[len(s_mhz) // 2] / 1e3, 3),
                         samples=len(samples), source='torch.cuda.clock_rate() (amdsmi sclk) every 2 ms over 5 extra steps after the timed region')
    if rank == 0:
        seqs = args.steps * cfg['B'] * world
        value = seqs / dt
        fl = flops_train_per_seq(cfg['emb_dim'], cfg['n_layers'], cfg['T'], cfg['R'], cfg['n_words'], cfg['n_pred'])
        # dominant kernel: the (epilogue, M, N, K) GEMM instance with the largest summed event time
        roof = None
        if prof:
            agg = {}
            for key, evs in prof.items():
                ms = [a.elapsed_time(b) for a, b in evs]
                agg[key] = (sum(ms), len(ms))
            key, (tot, cnt) = max(agg.items(), key=lambda kv: kv[1][0])
            kind, M, N, K = key
            avg_ms = tot / cnt
            flops = 2.0 * M * N * K
            ach = flops / (avg_ms * 1e-3) / 1e12
            kname = '%s M=%d N=%d K=%d' % (kind, M, N, K)
            traffic, tsrc = None, None
            counter_clock = None
            import glob
            # newest round first (profiles/rNN_traffic.json, then rNN_cfg3_traffic.json for the 1024-sequence batch's shapes)
            for tpath in sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r[0-9][0-9]*_traffic.json')), reverse=True):
                rel = os.path.relpath(tpath, ROOT)
                if os.path.exists(tpath):   # HBM bytes/launch from the committed rocprofv3 --pmc passes of this command
                    tj = json.load(open(tpath))
                    traffic = tj.get('bench_keys', {}).get(kname)
                    counter_clock = counter_clock or tj.get('gemm_clock_ghz')
                    if traffic is not None:
                        tsrc = rel + ' (committed rocprofv3 --pmc passes of this command; not measured in this run)'
                        break
            peak = PEAK_FP8_TFLOPS if kind.startswith('gemm_fp8') else PEAK_BF16_TFLOPS
            roof = dict(bound='mfma', achieved=round(ach, 1), peak=peak, unit='TFLOP/s',
                        frac=round(ach / peak, 4), traffic=traffic, traffic_source=tsrc,
                        kernel=kname, launches=cnt, avg_ms=round(avg_ms, 4),
                        gemm_time_share=round((gemm_ms_per_step * args.steps if ops.PROFILE_ONLY is not None else
                                               sum(v[0] for v in agg.values())) / (dt * 1e3), 3),
                        step_frac=round(value / world * fl / 1e12 / (PEAK_FP8_TFLOPS if args.fp8 else PEAK_BF16_TFLOPS), 4),
                        step_frac_peak=PEAK_FP8_TFLOPS if args.fp8 else PEAK_BF16_TFLOPS)
            # secondary roofline: the same two fractions against the matrix peak AT THE SUSTAINED CLOCK (x2 for fp8)
            ghz = (clock or {}).get('sclk_ghz_mean') or counter_clock
            if ghz:
                pk = ghz * 256 * 4096 / 1e3 * (2.0 if kind.startswith('gemm_fp8') else 1.0)
                pk_step = ghz * 256 * 4096 / 1e3 * (2.0 if args.fp8 else 1.0)
                roof['at_sustained_clock'] = dict(
                    clock_ghz=ghz, peak=round(pk, 1), frac=round(ach / pk, 4),
                    step_frac=round(value / world * fl / 1e12 / pk_step, 4),
                    clock_source=(clock['source'] if clock else 'GRBM_GUI_ACTIVE / dispatch duration over the GEMM kernels, committed '
                                  'rocprofv3 pass (profiles/*_counters.md); not measured in this run'),
                    live=clock, counters_gemm_clock_ghz=counter_clock)
        metric = 'pre-train samples/sec (whole node), %dL/%dd seq=%d+%d' % (cfg['n_layers'], cfg['emb_dim'], cfg['T'], cfg['R'])
        out = dict(metric=metric, value=round(value, 2),
                   unit='sequences/s', n_gpus=world, steps=args.steps, warmup=args.warmup,
                   ms_per_step=round(dt / args.steps * 1e3, 3), higher_is_better=True, scaling='weak',
                   vs_baseline=None, dtype='fp8 e4m3/e5m2 layer GEMMs, bf16 elsewhere' if args.fp8 else 'bf16', data='synthetic',
                   config=dict(workload='%s: %dL/%dd/%dh, %d regions + %d tokens, V=%d, %d MLM targets/seq + ITM BCE, '
                                        'dropout %.2f, adam_inverse_sqrt + clip 5%s'
                                        % (args.config, cfg['n_layers'], cfg['emb_dim'], cfg['n_heads'], cfg['R'], cfg['T'],
                                           cfg['n_words'], cfg['n_pred'], args.dropout,
                                           (' + %d AoA refiner layers (not in flops_train_per_seq)' % args.refine_layers
                                            if args.refine_layers else '') + (', ragged text lengths U[T/2, T]' if args.ragged else '')
                                           + (', fp8 layer projections + data gradients' if args.fp8 else '')),
                               per_gpu_batch=cfg['B'], global_batch=cfg['B'] * world, seq_len=cfg['T'] + cfg['R'],
                               parallelism='dp%d' % world, flops_train_per_seq=fl, prewarm_steps=3 * groups,
                               host_enqueue_ms_per_step=round(sorted(host_ms)[len(host_ms) // 2], 2)))
        if args.full:
            out['roofline'] = roof
        if instances is not None:
            out['gemm_instances'] = instances
        if comm is not None:
            out['comm'] = comm
        if shared:
            out['data'] = 'synthetic; DRY RUN: %d ranks sharing one GPU over gloo - not a measurement' % world
        if forced:
            out['config']['parallelism'] = 'dp1 wrapped (M3P_DP_FORCE: one rank running its collectives over RCCL; development run)'
        plain_default = (world == 1 and not forced and args.config == 'cfg2' and args.batch is None and not args.fp8
                         and not args.ragged and not args.refine_layers)
        if args.full and plain_default and not args.no_also:
            #  the 0.40-of-roofline target is stated on 1024 sequences per GPU (BASELINE configs[2]'s per-GPU share):
            # the default line carries that number too, so that it is not a builder-only measurement.  Same model, same step,
            # B = 1024; its own pre-warm, then 20 timed steps between synchronisations (~2.5 s).
            del trainer, tup, step, last
            torch.cuda.empty_cache()
            out['also'] = dict(cfg3=also_config('cfg3', args.dropout, 20))
        if args.full and world == 1 and not args.no_cpu_baseline:
            trainer = None
            torch.cuda.empty_cache()
            out['cpu_baseline'] = cpu_baseline(cfg, args.dropout)
        print(json.dumps(out), flush=True)
    if multi:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
