"""Data-parallel wrapper on the real model, driven through XTrainer like a training run: two
ranks each take half of a batch and go through ``pretrain_under_step`` / ``t2i_step`` /
``mlm_step_on_batch`` -> ``optimize`` (clip 5 + fused Adam).  Compared with ONE process running
the whole batch:
  * the reduced, averaged gradient arena the optimizer consumes (captured right before Adam -
    Adam's normalisation would hide a gradient that is a constant factor too large),
  * the clip norm, and the parameters after the steps;
  * ranks end bit-identical.
Scenarios: MLM + ITM; i2t with MRM + MRFR + CLCM (two encoder passes per step); gradient
accumulation over 2 micro-steps; ITM fine-tuning (no dense vocabulary gradient); text MLM; translation; captioning.
Both ranks share cuda:0 over gloo (one MI355X is all a test box has); the same scenarios run
over RCCL ('nccl') when at least two devices are visible."""
import os
import socket
import traceback

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from m3p_amd import synth

pytestmark = pytest.mark.gpu

CFG = dict(emb_dim=128, n_heads=4, n_layers=2, n_words=1000, T=24, R=10, B=8, n_pred=4)


def _free_port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close()
    return p


def _params(scenario, multi_gpu):
    two = dict(n_langs=2, id2lang={0: 'en', 1: 'zh'}, lang2id={'en': 0, 'zh': 1}, mt_steps=[('en', 'zh')]) if scenario in ('mt', 'ic') else {}
    P = synth.model_params(CFG['emb_dim'], CFG['n_heads'], CFG['n_layers'], CFG['n_words'], **two)
    for k, v in dict(optimizer='adam_inverse_sqrt,beta1=0.9,beta2=0.98,lr=0.0001', clip_grad_norm=5, amp=1, fp16=True,
                     accumulate_gradients=2 if scenario == 'accumulate' else 1, multi_gpu=multi_gpu, local_rank=0,
                     epoch_size=1000, batch_size=CFG['B'], dump_path='/nonexistent_m3p_dump', is_master=True,
                     cross_mlm_steps=[('google', 'img')], cross_rel_steps=[('google', 'img')],
                     cross_mrm_steps=[('google', 'img')] if scenario == 'clcm' else [],
                     cross_mrfr_steps=[('google', 'img')] if scenario == 'clcm' else [],
                     cross_clcm_steps=[('google', 'img')] if scenario == 'clcm' else [],
                     sample_n=2, refine_image=False, multi_cls_loss_weight=1 if scenario == 'finetune' else 0,
                     bin_cls_loss_weight=1, langs=['en', 'zh'] if scenario in ('mt', 'ic') else ['en']).items():
        setattr(P, k, v)
    return P


def _build(scenario, multi_gpu):
    from m3p_amd.model.transformer import TransformerModel
    from m3p_amd.trainer import XTrainer
    P = _params(scenario, multi_gpu)
    m = TransformerModel(P, is_encoder=True, with_output=True, is_crossModal=True)
    sd = synth.golden_state_dict(synth.hot_param_shapes(P))
    sd.update(synth.golden_state_dict(synth.region_head_param_shapes(P), seed=4321, pad_index=None))
    sd.update(synth.golden_state_dict(synth.clcm_head_param_shapes(P), seed=9753, pad_index=None))
    if scenario in ('mt', 'ic'):
        sd.update(synth.golden_state_dict(synth.cross_attention_param_shapes(P), seed=2468, pad_index=None))
    m.load_state_dict(sd, strict=False)
    m = m.cuda()
    return XTrainer(m, {}, P), m


def _slice(full, extra, sl, ng):
    """Columns ``sl`` of the synthetic batch as the tuples the collates emit."""
    lens = full['lengths'][sl].contiguous()
    tmax = int(lens.max())               # a rank's batch is as long as ITS longest sentence: token-row counts differ across ranks
    x, lab = full['x'][:tmax, sl].contiguous(), full['x_labels'][:tmax, sl].contiguous()
    img = full['x_img'][:, sl].transpose(0, 1).contiguous()
    loc = full['image_loc'][:, sl].transpose(0, 1).contiguous()
    n = x.shape[1]
    mask = torch.ones(n, CFG['R'], dtype=torch.long)
    pos = full['pos_labels'][ng].tolist()
    obj = extra['obj_labels'][sl].contiguous()
    ori = extra['ori_att_feats'][sl].contiguous()
    t2i = ((x, lens, lab), (img, mask, loc, obj, pos, ori, list(range(n))))
    x2, len2 = extra['x2'][:, sl].contiguous(), extra['len2'][sl].contiguous()
    i2t = ((x, lens, lab), (x2, len2), (extra['clcm'][sl].contiguous(), img, mask, loc, obj, pos, ori, list(range(n))))
    fin = ((x, lens, torch.zeros_like(x)), (img, mask, loc, obj, pos, list(range(n))))
    text = (x, lens, full['pred_mask'][:tmax, sl].contiguous(), lab[full['pred_mask'][:tmax, sl]])
    return dict(t2i=t2i, i2t=i2t, fin=fin, text=text, mt=(x, lens, x2, len2), ic=(x2, len2, img, mask, loc))


def _batches(step):
    B = CFG['B']
    full = synth.make_batch(CFG['T'], CFG['R'], B, CFG['n_words'], CFG['n_pred'], seed=11 + step, ragged=True)
    other = synth.make_batch(CFG['T'], CFG['R'], B, CFG['n_words'], 0, seed=50 + step, ragged=True)
    extra = synth.make_region_targets(CFG['R'], B, seed=77 + step)
    lab = extra['obj_labels']                                # the same number of masked regions on both halves: a rank's
    lab[B // 2:] = torch.where(lab[:B // 2] != -1, (lab[:B // 2] + 7) % 1600, lab[:B // 2])   # mean is then the global mean
    len2 = other['lengths'].clone()
    len2[B // 2:] = len2[:B // 2]           # the same number of target words on both halves (translation scenario)
    extra.update(x2=other['x'], len2=len2, clcm=torch.tensor([1, 0, 0, 1, 1, 0, 1, 0])[:B])
    return full, extra


def _run_step(tr, scenario, tup):
    if scenario in ('pretrain', 'accumulate'):
        tr.pretrain_under_step(tup['t2i'], 'google', 't2i', 'en', 1.0, 1.0, 1.0, 1.0)
    elif scenario == 'clcm':
        tr.pretrain_under_step(tup['i2t'], 'google', 'i2t', 'en', 1.0, 1.0, 1.0, 1.0)
    elif scenario == 'finetune':
        tr.t2i_step(tup['fin'], 'google', 1.0)
    elif scenario == 'text':
        tr.mlm_step_on_batch(*tup['text'], 'en', 1.0)
    elif scenario == 'mt':          # two differentiated passes per step: encoder stream, then the causal stream over it
        tr.mt_step_on_batch(*tup['mt'], 'en', 'zh', 1.0)
    elif scenario == 'ic':          # captioning: image stream -> layers-only encoder pass -> causal stream (three passes; the
        tr.ic_step_on_batch(*tup['ic'], 'google', 'img', 1.0)       # image stream's gradients are the LAST backward writes)
    tr.n_iter += 1


def _capture_grads(tr, m):
    """Snapshot (averaged gradient arena, clip norm) every time the optimizer is about to step."""
    opt = tr.optimizers['model']
    snaps = []
    inner = opt.step

    def step(closure=None):
        hook = m.ddp_hook
        if hook is not None:
            hook.finish()
        torch.cuda.synchronize()
        # (under the sharded exchange a rank holds the reduced gradient of its shards only: gather them for the comparison)
        g = hook.full_reduced_grad() if hook is not None else m.arena().grad
        snaps.append(((g * opt.grad_scale).cpu(), opt.grad_norm()))
        return inner(closure)
    opt.step = step
    return snaps


N_STEPS = 2


def _drive(scenario, world, rank, wrapped=None):
    tr, m = _build(scenario, world > 1 if wrapped is None else wrapped)
    snaps = _capture_grads(tr, m)
    micro = 2 if scenario == 'accumulate' else 1
    tr.n_iter = 1 if micro == 2 else 0                        # so that micro-steps go (non-boundary, boundary)
    for step in range(N_STEPS * micro):
        full, extra = _batches(step)
        per = CFG['B'] // world
        sl = slice(rank * per, (rank + 1) * per)
        ng = slice(rank * per // 2, (rank + 1) * per // 2)
        _run_step(tr, scenario, _slice(full, extra, sl, ng))
    torch.cuda.synchronize()
    return tr, m, snaps


def _worker(rank, world, port, q, scenario, backend, mode='zero1'):
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          HSA_ENABLE_IPC_MODE_LEGACY='0', M3P_DP_MODE=mode, M3P_DP_FORCE='1' if world == 1 else '0',
                          M3P_DP_TILE_QUEUE='1')       # (opt-in since round 4: keep the queue instantiations under test)
        torch.cuda.set_device(rank if backend == 'nccl' else 0)
        dist.init_process_group(backend, rank=rank, world_size=world)
        tr, m, snaps = _drive(scenario, world, rank, wrapped=True)
        assert tr.model.mode == mode, (tr.model.mode, mode)
        if mode == 'zero1':
            # between steps the big matrices' fp32 master is current on its owner rank only: state_dict() must refuse to
            # hand that out, and materialize_master() - a collective, every rank - must complete it
            assert tr.model.master_partial
            try:
                m.state_dict()
                raise AssertionError('state_dict() handed out a partial master')
            except RuntimeError as e:
                assert 'materialize_master' in str(e)
        tr.model.materialize_master()
        assert not tr.model.master_partial
        m.state_dict()
        pm = m.arena().master.clone()
        gathered = [torch.zeros_like(pm) for _ in range(world)]
        dist.all_gather(gathered, pm)
        same = all(torch.equal(gathered[0], t) for t in gathered)
        leftover = float(m.arena().grad.abs().max())
        launched_vocab = 'vocab' in tr.model._launched or scenario != 'finetune'
        if rank == 0:
            # numpy, not tensors: a tensor crosses the queue as a shared-memory handle that dies with this process
            q.put(('ok', [(g.numpy(), n) for g, n in snaps], pm.cpu().numpy(), same, leftover, launched_vocab))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        if rank == 0:
            q.put(('err', traceback.format_exc(), None, False, 0.0, False))
        raise


def _check(scenario, backend, world=2, mode='zero1'):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, scenario, backend, mode)) for r in range(world)]
    for p in procs:
        p.start()
    status, snaps, pm, same, leftover, _ = q.get(timeout=600)
    for p in procs:
        p.join(timeout=120)
    assert status == 'ok', snaps
    assert same, 'parameters diverged across ranks'
    assert leftover == 0.0, 'gradient arena not zeroed by the fused step'
    tr, m, ref = _drive(scenario, 1, 0)
    assert len(snaps) == len(ref) == N_STEPS
    off = m.arena().offsets
    v0, v1 = off['embeddings.weight'][0], off['embeddings.weight'][0] + off['embeddings.weight'][1]
    pm = torch.from_numpy(pm)
    for i, ((g, n), (gr, nr)) in enumerate(zip(snaps, ref)):
        g = torch.from_numpy(g)
        err = float((g - gr).norm() / gr.norm())
        err_vocab = float((g[v0:v1] - gr[v0:v1]).norm() / gr[v0:v1].norm())
        assert err < 2e-2, (scenario, i, err)
        assert err_vocab < 2e-2, (scenario, i, err_vocab)     # the tied matrix: dense head part + exchanged token rows
        assert abs(n - nr) / nr < 1e-2, (scenario, i, n, nr)
    lr_sum = sum(tr.optimizers['model'].get_lr_for_step(k) for k in range(N_STEPS))
    diff = float((pm - m.arena().master.cpu()).abs().max())
    assert diff <= 2.5 * lr_sum, (scenario, diff, lr_sum)    # Adam moves every weight by <= ~lr per step


@pytest.mark.parametrize('scenario', ['pretrain', 'clcm', 'accumulate', 'finetune', 'text', 'mt', 'ic'])
def test_dp_two_ranks_match_single_process(scenario):
    _check(scenario, 'gloo')


def test_dp_four_ranks_ragged_token_counts():
    _check('pretrain', 'gloo', world=4)


@pytest.mark.parametrize('scenario', ['pretrain', 'finetune'])
def test_dp_all_reduce_mode(scenario):
    _check(scenario, 'gloo', mode='allreduce')


@pytest.mark.parametrize('mode', ['zero1', 'allreduce'])
def test_dp_one_rank_over_rccl(mode):
    """The RCCL-only branches (in-place reduce_scatter_tensor / all_gather_into_tensor on the arena buckets, the side stream,
    the tile queues data parallelism switches on) on the one device a test box has: a world of one rank, wrapped, must
    reproduce the unwrapped step."""
    _check('pretrain', 'nccl', world=1, mode=mode)


BIG = dict(emb_dim=768, n_heads=12, n_layers=1, n_words=88000, T=96, R=32, B=128, n_pred=32)   # 4096 predicted rows: the store path


def _lazy_worker(rank, world, port, q, mode, backend):
    """Ranks over RCCL (a forced world of one) or gloo (two ranks on the one device) at a size where the MLM head STORES the
    vocabulary weight gradient: MLM + ITM, MLM + ITM, an ITM-only step, MLM + ITM - with the lazy zero of the vocabulary range
    on, off, off (the third run is the noise floor)."""
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          HSA_ENABLE_IPC_MODE_LEGACY='0', M3P_DP_MODE=mode, M3P_DP_FORCE='1' if world == 1 else '0')
        torch.cuda.set_device(0)
        dist.init_process_group(backend, rank=rank, world_size=world)
        from m3p_amd import optim as Om
        global CFG
        CFG = BIG
        outs, events = [], []
        for lazy in (True, False, False):
            Om._LAZY_VOCAB_ZERO = lazy
            tr, m = _build('pretrain', True)
            assert tr.model.mode == mode
            ar = m.arena()
            ev = []
            real_zero, real_defer = ar.ensure_zero, ar.defer_vocab_zero

            def ensure_zero(ar=ar, ev=ev, real_zero=real_zero):
                if ar.stale is not None:
                    ev.append('memset')
                real_zero()

            def defer(ev=ev, real_defer=real_defer):
                ev.append('defer')
                real_defer()
            ar.ensure_zero, ar.defer_vocab_zero = ensure_zero, defer
            full = synth.make_batch(CFG['T'], CFG['R'], CFG['B'], CFG['n_words'], CFG['n_pred'], seed=3 + rank)
            assert full['y'].numel() == 4096
            extra = synth.make_region_targets(CFG['R'], CFG['B'], seed=77 + rank)
            extra.update(x2=full['x'], len2=full['lengths'], clcm=torch.zeros(CFG['B'], dtype=torch.long))
            tup = _slice(full, extra, slice(0, CFG['B']), slice(0, CFG['B'] // 2))
            for step in range(4):
                _run_step(tr, 'finetune' if step == 2 else 'pretrain', tup)
            tr.model.materialize_master()
            torch.cuda.synchronize()
            ar.ensure_zero()
            assert float(ar.grad.abs().max()) == 0.0
            outs.append(ar.master.float().cpu().numpy())
            events.append(ev)
        pm = m.arena().master.clone()
        gathered = [torch.zeros_like(pm) for _ in range(world)]
        dist.all_gather(gathered, pm)
        same = all(torch.equal(gathered[0], t) for t in gathered)
        if rank == 0:
            q.put(('ok', outs, events, same))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        if rank == 0:
            q.put(('err', traceback.format_exc(), None, False))
        raise


@pytest.mark.parametrize('mode,world,backend', [('zero1', 1, 'nccl'), ('allreduce', 1, 'nccl'), ('zero1', 2, 'gloo')])
def test_dp_lazy_vocab_zero_changes_nothing(mode, world, backend):
    """Round 6: the lazily zeroed vocabulary gradient range (Arena.defer_vocab_zero) under the data-parallel wrapper - the bucket
    collectives, the exchanged token rows (which enter through Arena.g()) and, sharded, the foreign shards the rank leaves
    un-zeroed: same weights with the switch on and off, to the step's own run-to-run noise, the switch was exercised, and the
    ranks end bit-identical."""
    import numpy as np
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_lazy_worker, args=(r, world, port, q, mode, backend)) for r in range(world)]
    for p in procs:
        p.start()
    status, outs, events, same = q.get(timeout=900)
    for p in procs:
        p.join(timeout=120)
    assert status == 'ok', outs
    assert same, 'parameters diverged across ranks'
    assert events[0].count('defer') == 3 and events[0].count('memset') >= 1 and events[1] == [] and events[2] == [], events
    a, b, c = outs
    noise = float(np.linalg.norm(c - b) / np.linalg.norm(b))
    diff = float(np.linalg.norm(a - b) / np.linalg.norm(b))
    assert diff <= max(10 * noise, 1e-7), (diff, noise)


@pytest.mark.parametrize('scenario', ['pretrain', 'clcm'])
def test_dp_two_ranks_over_rccl(scenario):
    if torch.cuda.device_count() < 2:
        pytest.skip('RCCL needs two devices (the driver\'s multi-GPU bench exercises it)')
    _check(scenario, 'nccl')


def test_bench_multi_gpu_half_runs_unattended():
    """bench.py's N > 1 half (launcher environment, wrapped model, `comm` block with the exposed wait and the per-bucket
    bus bandwidth, which --full adds) is otherwise first executed by the driver's 8-GPU run: here it runs as a forced one-rank world under
    torch.distributed.run on the one device a test box has, and the JSON line must parse with the fields the driver reads."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, M3P_DP_FORCE='1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '1', '--master-addr', '127.0.0.1',
           '--master-port', '29613', os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1',
           '--full', '--no-cpu-baseline', '--batch', '32']
    res = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    line = [ln for ln in res.stdout.splitlines() if ln.startswith('{')][-1]
    out = json.loads(line)
    assert out['n_gpus'] == 1 and out['steps'] == 2 and out['value'] > 0 and out['scaling'] == 'weak'
    comm = out['comm']
    assert comm['mode'] in ('zero1', 'allreduce') and comm['exposed_ms_per_step'] >= 0
    assert comm['buckets'] and all(b['ms'] > 0 and b['MB'] > 0 for b in comm['buckets'].values())
    assert any(k.startswith('params') for k in comm['buckets']) == (comm['mode'] == 'zero1')
    # round 5, first-contact kit: who is in the group, where the exposed tail sits, which bound each collective lands by
    assert comm['backend'] == 'nccl' and comm['ranks'] == 1 and comm['rccl_ranks_seen'] == 1
    split = comm['exposed_split_ms']
    assert split['gradient_buckets'] >= 0 and split['token_rows'] >= 0
    assert abs(split['gradient_buckets'] + split['token_rows'] - comm['exposed_ms_per_step']) < 1e-2
    assert all({'ring_bound_ms', 'direct_bound_ms', 'lands'} <= set(b) for b in comm['buckets'].values())
    assert 'token rows (all_gather)' in comm['buckets'] and not any('token ids' in k for k in comm['buckets'])   # ONE gather
