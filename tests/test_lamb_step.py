"""Lamb.step on real models: every tensor of the arena after a real backward against the per-tensor fp64 twin and bounds of
tests/test_lamb_kernels.py (lamb_ref64), the lazily zeroed vocabulary range, a short training run through XTrainer, and a
forced one-rank data-parallel world in both exchange modes."""
import os
import socket
import traceback

import pytest
import torch

from m3p_amd import synth
from tests.test_lamb_kernels import _ratio, lamb_ref64
from tests.test_model_parity import _build, _losses
from tests.util import assert_bits_equal, assert_exact_zero

pytestmark = pytest.mark.gpu

SPEC = 'lamb,lr=0.002,weight_decay=0.01,beta1=0.9,beta2=0.98'
CLIP = 5.0


def _snapshot(m, opt):
    """State of the arena right before Lamb.step (after clip_grad_norm, which reduced the norm on the device)."""
    ar = m.arena()
    ent = next(iter(opt._arenas.values()))
    hook = ar.model.ddp_hook
    if hook is not None:
        hook.finish()
    torch.cuda.synchronize()
    return dict(p=ar.master.clone(), g=(hook.full_reduced_grad() if hook is not None else ar.grad).clone(), m=ent['m'].clone(),
                v=ent['v'].clone(), touched=set(ar.touched), steps={n: opt.state[p]['step'] for n, p in ar.params.items()},
                lr=opt.param_groups[0]['lr'], gnorm_sq=float(ent['gnorm'].item()))


def _quads_per_thread(opt, ar):
    """name -> the most quads one thread of the update launch adds for that tensor, over the optimizer's cached tables."""
    starts = sorted((o, n) for n, (o, _, _) in ar.offsets.items())
    out = {}
    for cache in opt._tables.values():
        for table in cache.values():
            for (s, _, _, _, _), q in zip(table.pieces, table.quads_per_thread()):
                name = [n for o, n in starts if o <= s][-1]
                out[name] = max(out.get(name, 1), q)
    return out


def check_step(m, opt, snap, max_norm=CLIP, what=''):
    """Every tensor of the arena after the step that followed `snap`: touched ones within the kernel test's bounds of the fp64
    twin (parameters, both moments, the bf16 copy bit-equal to the rounded parameter), untouched ones bit-unchanged with their
    step count.  -> the worst error / bound of p, m, v."""
    ar = m.arena()
    ent = next(iter(opt._arenas.values()))
    group = opt.param_groups[0]
    hp = dict(lr=snap['lr'], beta1=group['betas'][0], beta2=group['betas'][1], eps=group['eps'], max_norm=max_norm,
              grad_scale=opt.grad_scale, gnorm_sq=snap['gnorm_sq'] if max_norm > 0 else None)
    qpt = _quads_per_thread(opt, ar)
    after = dict(p=ar.master, m=ent['m'], v=ent['v'])
    worst = dict(p=0.0, m=0.0, v=0.0)
    n_touched = 0
    for name, p in ar.params.items():
        o, cnt, _ = ar.offsets[name]
        sl = slice(o, o + cnt)
        if name not in snap['touched']:
            for c in 'pmv':
                assert_bits_equal(after[c][sl], snap[c][sl], '%s: untouched %s, %s' % (what, name, c))
            assert opt.state[p]['step'] == snap['steps'][name]
            continue
        n_touched += 1
        s = snap['steps'][name] + 1
        assert opt.state[p]['step'] == s, name
        plain = opt.exclude_1d and p.dim() < 2
        cls = (1.0 / (1 - hp['beta1'] ** s), 1.0 / (1 - hp['beta2'] ** s), 0.0 if plain else group['weight_decay'], not plain)
        ref = lamb_ref64(snap['p'][sl], snap['g'][sl], snap['m'][sl], snap['v'][sl], cls, hp, qpt[name])
        for c in 'pmv':
            w = _ratio(after[c][sl], ref[c], ref[c + '_bound'])
            worst[c] = max(worst[c], w)
            assert w <= 1.0, '%s: %s of %s (%d elements, step %d) is off by %.3g x its bound' % (what, c, name, cnt, s, w)
        assert_bits_equal(ar.w16[sl], ar.master[sl].to(torch.bfloat16), '%s: bf16 copy of %s' % (what, name))
    print('%s: %d touched tensors, worst error / bound  p %.3f  m %.3f  v %.3f' % (what, n_touched, worst['p'], worst['m'], worst['v']))
    return worst, n_touched


def test_plain_step_matches_the_twin():
    """cfg1, one real backward of the MLM loss (the ITM head stays untouched), clip 5 + step."""
    from m3p_amd import optim as Om
    cfg = synth.CONFIGS['cfg1']
    m, P, sd = _build(cfg)
    opt = Om.get_optimizer(m.parameters(), SPEC)
    assert type(opt) is Om.Lamb
    batch = synth.make_batch(cfg['T'], cfg['R'], cfg['B'], cfg['n_words'], cfg['n_pred'])
    out, mlm, rel, bce = _losses(m, batch, cfg['R'])
    mlm.backward()
    opt.clip_grad_norm(CLIP)
    snap = _snapshot(m, opt)
    ar = m.arena()
    untouched = [n for n in ar.names if n not in snap['touched']]
    assert snap['touched'] and untouched, 'the case wants both touched and untouched tensors'
    assert any(ar.params[n].dim() < 2 for n in snap['touched']) and float(snap['g'].abs().max()) > 0
    opt.step()
    torch.cuda.synchronize()
    worst, n = check_step(m, opt, snap, what='plain step')
    assert n == len(snap['touched']) and worst['p'] > 0
    tables = [t for c in opt._tables.values() for t in c.values()]
    assert len(tables) == 1 and tables[0].n_tensors == n > 32        # one table, three launches, however many tensors
    for name in ar.names:
        assert_exact_zero(ar.g(name), 'gradient of %s after the step' % name)
    # the same step type again: the cached table serves
    out, mlm, rel, bce = _losses(m, batch, cfg['R'])
    mlm.backward()
    opt.clip_grad_norm(CLIP)
    snap = _snapshot(m, opt)
    opt.step()
    torch.cuda.synchronize()
    check_step(m, opt, snap, what='second plain step')
    assert [t for c in opt._tables.values() for t in c.values()] == tables


def test_more_step_counts_than_one_launch_carries():
    """A launch carries 32 classes of per-tensor scalars by value.  Here every touched tensor has sat out a different number of
    steps (the counts are set by hand): more classes than that, so the group goes on in a second table and three more launches,
    and every tensor still meets the twin with the bias corrections of its own count."""
    from m3p_amd import ops, optim as Om
    cfg = synth.CONFIGS['cfg1']
    m, P, sd = _build(cfg)
    opt = Om.get_optimizer(m.parameters(), SPEC)
    batch = synth.make_batch(cfg['T'], cfg['R'], cfg['B'], cfg['n_words'], cfg['n_pred'])
    out, mlm, rel, bce = _losses(m, batch, cfg['R'])
    mlm.backward()
    ar = m.arena()
    for k, name in enumerate(n for n in ar.names if n in ar.touched):
        opt.state[ar.params[name]]['step'] = k
    opt.clip_grad_norm(CLIP)
    snap = _snapshot(m, opt)
    assert len({snap['steps'][n] for n in snap['touched']}) > ops.LAMB_MAX_CLASSES
    opt.step()
    torch.cuda.synchronize()
    worst, n = check_step(m, opt, snap, what='43 step counts')
    tables = [t for c in opt._tables.values() for t in c.values()]
    assert len(tables) == 2 and tables[0].n_classes == ops.LAMB_MAX_CLASSES and sum(t.n_tensors for t in tables) == n
    for name in ar.names:
        assert_exact_zero(ar.g(name), 'gradient of %s after the step' % name)


def test_second_step_takes_the_lazy_vocabulary_path():
    """At a size where the MLM head STORES the tied matrix's weight gradient (the case of test_model_parity's lazy-zero test)
    the step leaves the vocabulary range un-zeroed: its pieces hold r, logically zero.  The second step - whose store
    overwrites them - meets the twin like the first, and every gradient reads zero through Arena.g() afterwards."""
    from m3p_amd import optim as Om
    cfg = dict(emb_dim=768, n_heads=12, n_layers=1, n_words=88000, T=96, R=32, B=128, n_pred=32)
    batch = synth.make_batch(cfg['T'], cfg['R'], cfg['B'], cfg['n_words'], cfg['n_pred'], seed=3)
    m, P, sd = _build(cfg)
    opt = Om.get_optimizer(m.parameters(), SPEC)
    ar = m.arena()
    v0, vc = ar.vocab_range()
    for step in range(2):
        out, mlm, rel, bce = _losses(m, batch, cfg['R'])
        (mlm + bce).backward()
        assert ar.vocab_stored and ar.stale is None, 'the MLM head did not store over the vocabulary range'
        opt.clip_grad_norm(CLIP)
        snap = _snapshot(m, opt)
        opt.step()
        torch.cuda.synchronize()
        assert ar.stale == (v0, vc), 'the step did not defer the vocabulary range'
        check_step(m, opt, snap, what='lazy path, step %d' % (step + 1))
    table = [t for c in opt._tables.values() for t in c.values()]
    assert len(table) == 1
    kept = [(a, b) for a, b, _, z, _ in table[0].pieces if not z]
    assert kept and min(a for a, _ in kept) == v0 and all(v0 <= a and b <= v0 + vc for a, b in kept)
    assert sum(b - a for a, b in kept) >= ar.offsets['embeddings.weight'][1]
    assert all(b <= v0 or a >= v0 + vc for a, b, _, z, _ in table[0].pieces if z)
    assert float(ar.grad[v0:v0 + vc].abs().max()) > 0             # physically r ...
    for name in ar.names:                                            # ... logically zero
        assert_exact_zero(ar.g(name), 'gradient of %s after the lazy step' % name)


def test_six_steps_lower_the_loss():
    from m3p_amd.trainer import XTrainer
    from m3p_amd import optim as Om
    cfg = synth.CONFIGS['cfg1']
    m, P, sd = _build(cfg)
    for k, v in dict(optimizer='lamb_inverse_sqrt,lr=0.01,warmup_updates=2,weight_decay=0.01,beta1=0.9,beta2=0.98', clip_grad_norm=5,
                     amp=-1, fp16=False, accumulate_gradients=1, multi_gpu=False, epoch_size=100, cross_mlm_steps=[('google', 'img')],
                     cross_mrm_steps=[], cross_mrfr_steps=[], cross_clcm_steps=[], sample_n=2, refine_image=False,
                     multi_cls_loss_weight=0, bin_cls_loss_weight=1, batch_size=cfg['B'], dump_path='/nonexistent_m3p_dump').items():
        setattr(P, k, v)
    tr = XTrainer(m, {}, P)
    opt = tr.optimizers['model']
    assert type(opt) is Om.LambInverseSqrtWithWarmup
    batch = synth.make_batch(cfg['T'], cfg['R'], cfg['B'], cfg['n_words'], cfg['n_pred'])
    B, R = cfg['B'], cfg['R']
    img = batch['x_img'].transpose(0, 1).contiguous()
    loc = batch['image_loc'].transpose(0, 1).contiguous()
    tup = ((batch['x'], batch['lengths'], batch['x_labels']),
           (img, torch.ones(B, R, dtype=torch.long), loc, torch.full((B, R), -1), batch['pos_labels'].tolist(), None, None))
    losses = []
    for step in range(6):
        tr.pretrain_under_step(tup, 'google', 't2i', 'en', 1.0, 1.0, 1.0, 1.0)
        losses.append(float(tr.stats['CMLM-google'][-1]) + float(tr.stats['t2i-google'][-1]))     # (iter() empties the lists every fifth)
        tr.iter()
    print('lamb_inverse_sqrt, six steps on one batch: losses', ['%.4f' % x for x in losses])
    assert len(losses) == 6 and losses[-1] < losses[0]
    g = opt.param_groups[0]
    assert g['num_updates'] == 6 and g['lr'] == opt.get_lr_for_step(6) == 0.01 * (2 / 6) ** 0.5


# ---- a forced one-rank data-parallel world (M3P_DP_FORCE=1), both exchange modes, in a fresh child process -------------
def _free_port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close()
    return p


def _dp_worker(port, q, mode):
    import torch.distributed as dist
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK='0', WORLD_SIZE='1', HSA_ENABLE_IPC_MODE_LEGACY='0',
                          M3P_DP_MODE=mode, M3P_DP_FORCE='1')
        torch.cuda.set_device(0)
        dist.init_process_group('nccl', rank=0, world_size=1)
        from m3p_amd import optim as Om
        import tests.test_distributed_gpu as D
        real_params = D._params

        def params(scenario, multi_gpu):
            P = real_params(scenario, multi_gpu)
            P.optimizer = SPEC
            return P
        D._params = params
        tr, m = D._build('pretrain', True)
        opt = tr.optimizers['model']
        assert type(opt) is Om.Lamb and tr.model.mode == mode
        snaps, inner = [], opt.step

        def step(closure=None):
            snaps.append(_snapshot(m, opt))
            return inner(closure)
        opt.step = step
        full, extra = D._batches(0)
        D._run_step(tr, 'pretrain', D._slice(full, extra, slice(0, D.CFG['B']), slice(0, D.CFG['B'] // 2)))
        wrapped = not tr.model.single
        tr.model.materialize_master()
        torch.cuda.synchronize()
        assert len(snaps) == 1
        worst, n = check_step(m, opt, snaps[0], max_norm=float(tr.params.clip_grad_norm), what='one-rank world, ' + mode)
        ar = m.arena()
        ar.ensure_zero()
        q.put(('ok', worst, n, wrapped, float(ar.grad.abs().max())))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        q.put(('err', traceback.format_exc(), 0, False, 0.0))
        raise


@pytest.mark.parametrize('mode', ['zero1', 'allreduce'])
def test_one_rank_world_matches_the_twin(mode):
    """The wrapped step - bucket collectives, shards, the norms table summed over the ranks between the norms and apply launches -
    meets the same per-tensor twin and bounds as the plain step (not its bits: the pieces are cut differently)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    proc = ctx.Process(target=_dp_worker, args=(_free_port(), q, mode))
    proc.start()
    status, worst, n, wrapped, leftover = q.get(timeout=600)
    proc.join(timeout=120)
    assert status == 'ok', worst
    assert wrapped, 'M3P_DP_FORCE=1 did not put the one-rank world on the data-parallel path'
    print('one-rank world (%s): %d touched tensors, worst error / bound %s' % (mode, n, worst))
    assert n > 32 and max(worst.values()) <= 1.0 and leftover == 0.0
