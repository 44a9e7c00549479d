"""The non-finite guard through real steps: Adam.guard_nonfinite / reconcile on cfg1 after real backward passes, the twin runs
(a skipped batch leaves the run where a run without it stands), the automatic reconcile at the ring's capacity, gradient
accumulation and the trainer's report, and a forced one-rank data-parallel world in both exchange modes.

Non-finite values enter through gradients only: (a) one element of a LayerNorm bias gradient set to +inf after a clean
backward, (b) the loss multiplied by NaN before backward()."""
import logging
import os
import traceback

import pytest
import torch

from m3p_amd import synth
from tests.test_lamb_step import _free_port
from tests.test_model_parity import _build, _losses
from tests.util import assert_bits_equal, assert_exact_zero

pytestmark = pytest.mark.gpu

SPECS = {
    'adam_inverse_sqrt': 'adam_inverse_sqrt,beta1=0.9,beta2=0.98,lr=0.0001,warmup_updates=2',
    'lamb_cosine': 'lamb_cosine,lr=0.002,weight_decay=0.01,beta1=0.9,beta2=0.98,warmup_updates=2,init_period=3',
    'adam': 'adam,lr=0.0001,beta1=0.9,beta2=0.98',
}
CLIPS = [5.0, 0.0]
LN_BIAS = 'layer_norm_emb.bias'
CFG = synth.CONFIGS['cfg1']
CLEAN_RERUNS = 24


def _batch(seed):
    return synth.make_batch(CFG['T'], CFG['R'], CFG['B'], CFG['n_words'], CFG['n_pred'], seed=seed)


@pytest.fixture(scope='module')
def batches():
    return [_batch(100 + k) for k in range(3)]


def _fresh(spec, guard=True):
    from m3p_amd import optim as Om
    m, P, sd = _build(CFG)
    opt = Om.get_optimizer(m.parameters(), SPECS[spec])
    opt.guard_nonfinite = guard
    return m, opt


def _step(m, opt, batch, clip, bad=None):
    out, mlm, rel, bce = _losses(m, batch, CFG['R'])
    loss = mlm + bce
    if bad == 'nan_loss':
        loss = loss * float('nan')
    loss.backward()
    if bad == 'inf_element':
        assert LN_BIAS in m.arena().touched
        m.arena().g(LN_BIAS)[3] = float('inf')
    if clip > 0:
        opt.clip_grad_norm(clip)
    opt.step()


def _state(m, opt):
    torch.cuda.synchronize()
    ar = m.arena()
    ent = next(iter(opt._arenas.values()))
    return dict(p=ar.master.clone(), m=ent['m'].clone(), v=ent['v'].clone(), w=ar.w16.clone(),
                steps={n: opt.state[p]['step'] for n, p in ar.params.items()},
                updates=[g.get('num_updates') for g in opt.param_groups], lr=[g['lr'] for g in opt.param_groups])


@pytest.mark.parametrize('bad', ['inf_element', 'nan_loss'])
@pytest.mark.parametrize('clip', CLIPS, ids=['clip5', 'noclip'])
@pytest.mark.parametrize('spec', sorted(SPECS))
def test_bad_step_leaves_the_model_as_it_was(spec, clip, bad, batches):
    m, opt = _fresh(spec)
    _step(m, opt, batches[0], clip)
    snap = _state(m, opt)
    assert float(snap['m'].abs().max()) > 0 and max(snap['steps'].values()) == 1
    _step(m, opt, batches[1], clip, bad=bad)
    now = _state(m, opt)
    for c in 'pmvw':          # (without the guard every touched element of all four is NaN here)
        assert_bits_equal(now[c], snap[c], '%s after the bad step' % c)
    ar = m.arena()
    ar.ensure_zero()
    assert_exact_zero(ar.grad, 'gradient arena after the bad step')
    touched = [n for n, s in snap['steps'].items() if s == 1]
    assert all(now['steps'][n] == 2 for n in touched), 'the host counts the attempt until reconcile()'
    report = opt.reconcile()
    after = _state(m, opt)
    assert after['steps'] == snap['steps'] and after['updates'] == snap['updates'] and after['lr'] == snap['lr']
    assert report['attempts'] == 2 and report['skipped_total'] == 1 and report['skipped_in_a_row'] == 1
    assert len(report['norms']) == 1 and 0 < report['norms'][0] < float('inf')


@pytest.mark.parametrize('clip', CLIPS, ids=['clip5', 'noclip'])
@pytest.mark.parametrize('spec', sorted(SPECS))
def test_twin_runs(spec, clip, batches):
    """A = b0, b1, b2.  B = b0, bad, reconcile, b1, b2.  Clean reruns A' measure what identical runs differ by (fp32 atomics in
    the embedding and bias gradients): if nothing, B equals A to the bit; else B may differ from A, per tensor, by at most
    twice the largest A - A' difference of that tensor.  That largest difference is taken over CLEAN_RERUNS reruns, not one:
    the noise is a last-bit flip here and there, and a single rerun shows 0 for a small tensor that the next one moves (B
    itself is one more draw of the same noise) - measured: image_embeddings bias, exp_avg, A - A' = 0 and A - B = 5.8e-11
    with one rerun.  A run is three steps of cfg1, a few tens of milliseconds."""
    def run(with_bad):
        m, opt = _fresh(spec)
        _step(m, opt, batches[0], clip)
        if with_bad:
            _step(m, opt, batches[1], clip, bad='nan_loss')
            assert opt.reconcile()['skipped_total'] == 1
        _step(m, opt, batches[1], clip)
        _step(m, opt, batches[2], clip)
        if with_bad:
            assert opt.reconcile()['skipped_total'] == 1
        return _state(m, opt), m.arena().offsets

    A, offsets = run(False)
    noise = {c: torch.zeros_like(A[c], dtype=torch.float64) for c in 'pmvw'}       # elementwise largest |A - A'| over the reruns
    for _ in range(CLEAN_RERUNS):
        A2, _ = run(False)
        for c in 'pmvw':
            noise[c] = torch.maximum(noise[c], (A[c].double() - A2[c].double()).abs())
    B, _ = run(True)
    for k in ('steps', 'updates', 'lr'):
        assert B[k] == A[k], k
    exact = all(float(noise[c].max()) == 0.0 for c in 'pmvw')
    print('%s, clip %g: %d clean reruns are %s' % (spec, clip, CLEAN_RERUNS, 'bit-equal to the first' if exact else 'NOT bit-equal to the first'))
    if exact:
        for c in 'pmvw':
            assert_bits_equal(B[c], A[c], 'run with a skipped batch against the run without it: ' + c)
        return
    worst = 0.0
    for name, (o, cnt, _) in offsets.items():
        for c in 'pmvw':
            n_t = float(noise[c][o:o + cnt].max())
            diff = float((A[c][o:o + cnt].double() - B[c][o:o + cnt].double()).abs().max())
            if n_t > 0 or diff > 0:
                print('  %-48s %s  A-A\' %.3e  A-B %.3e' % (name, c, n_t, diff))
            worst = max(worst, diff / n_t if n_t > 0 else (float('inf') if diff > 0 else 0.0))
            assert diff <= 2 * n_t, '%s of %s: A - B = %.3e, the largest A - A\' = %.3e' % (c, name, diff, n_t)
    print('  worst A-B / A-A\': %.3f' % worst)


def test_sixty_five_steps_reconcile_by_themselves():
    """Hand-written finite gradients on two small tensors, a non-finite one at attempt 3, no manual reconcile: the 65th step
    finds the ring full and reconciles first, so the counts are exact afterwards."""
    m, opt = _fresh('adam_inverse_sqrt')
    ar = m.arena()
    names = [LN_BIAS, 'layer_norm_emb.weight']
    reads = []
    inner = opt.reconcile
    opt.reconcile = lambda: (reads.append(len(opt._guard_log)), inner())[1]
    before = ar.master.clone()
    for attempt in range(65):
        for k, n in enumerate(names):
            ar.g(n).fill_(0.01 * (k + 1) * (1 + attempt % 3))
            ar.touch(n)
        if attempt == 3:
            ar.g(names[0])[0] = float('inf')
        if attempt % 2:
            opt.clip_grad_norm(5.0)
        opt.step()
    torch.cuda.synchronize()
    assert reads == [64], 'one automatic reconcile, with 64 attempts logged'
    assert len(opt._guard_log) == 1
    for n in names:
        assert opt.state[ar.params[n]]['step'] == 64, n
    g = opt.param_groups[0]
    assert g['num_updates'] == 64 and g['lr'] == opt.get_lr_for_step(64)
    report = inner()
    assert report['attempts'] == 65 and report['skipped_total'] == 1 and report['skipped_in_a_row'] == 0
    assert opt.state[ar.params[names[0]]]['step'] == 64 and g['num_updates'] == 64
    o, cnt, _ = ar.offsets[names[0]]
    assert bool((ar.master[o:o + cnt] != before[o:o + cnt]).all()) and bool(torch.isfinite(ar.master).all())
    assert set(opt.state_dict()) == {'state', 'param_groups'}


# ---- through the trainer ---------------------------------------------------------------------------------------------
def _trainer(accumulate=1, **extra):
    from m3p_amd.trainer import XTrainer
    m, P, sd = _build(CFG)
    for k, v in dict(optimizer=SPECS['adam_inverse_sqrt'], clip_grad_norm=5, amp=-1, fp16=False, accumulate_gradients=accumulate,
                     multi_gpu=False, epoch_size=100, cross_mlm_steps=[('google', 'img')], cross_mrm_steps=[], cross_mrfr_steps=[],
                     cross_clcm_steps=[], sample_n=2, refine_image=False, multi_cls_loss_weight=0, bin_cls_loss_weight=1,
                     batch_size=CFG['B'], dump_path='/nonexistent_m3p_dump', **extra).items():
        setattr(P, k, v)
    return XTrainer(m, {}, P), m


def _tup(batch):
    B, R = CFG['B'], CFG['R']
    img = batch['x_img'].transpose(0, 1).contiguous()
    loc = batch['image_loc'].transpose(0, 1).contiguous()
    return ((batch['x'], batch['lengths'], batch['x_labels']),
            (img, torch.ones(B, R, dtype=torch.long), loc, torch.full((B, R), -1), batch['pos_labels'].tolist(), None, None))


def _poison_next(tr, when):
    """The trainer's optimize() with the loss multiplied by NaN on the calls `when(call index)` says (way (b))."""
    inner, calls = tr.optimize, []

    def optimize(loss):
        calls.append(1)
        return inner(loss * float('nan') if when(len(calls) - 1) else loss)
    tr.optimize = optimize


def test_accumulated_group_with_a_bad_micro_step_is_dropped(batches):
    tr, m = _trainer(accumulate=2, skip_nonfinite_updates=True)
    assert tr.optimizers['model'].guard_nonfinite is True
    _poison_next(tr, lambda i: i == 0)
    ar = m.arena()
    ar.refresh()                                    # (the bf16 copy is first cast by the first forward: cast it now)
    torch.cuda.synchronize()
    before = dict(p=ar.master.clone(), w=ar.w16.clone())
    assert float(before['w'].float().abs().max()) > 0
    tr.n_iter = 1                                  # not a boundary: gradients only
    tr.pretrain_under_step(_tup(batches[0]), 'google', 't2i', 'en', 1.0, 1.0, 1.0, 1.0)
    tr.n_iter = 2                                   # boundary: the accumulated sum is poisoned - skip and zero
    tr.pretrain_under_step(_tup(batches[1]), 'google', 't2i', 'en', 1.0, 1.0, 1.0, 1.0)
    torch.cuda.synchronize()
    assert_bits_equal(ar.master, before['p'], 'master after the dropped group')
    assert_bits_equal(ar.w16, before['w'], 'bf16 copy after the dropped group')
    ar.ensure_zero()
    assert_exact_zero(ar.grad, 'gradients after the dropped group')
    assert tr.optimizers['model'].reconcile()['skipped_total'] == 1


def test_trainer_reports_and_rolls_back(batches, caplog):
    tr, m = _trainer(skip_nonfinite_updates=True)
    _poison_next(tr, lambda i: i == 2)
    with caplog.at_level(logging.INFO):
        for it in range(10):
            tr.pretrain_under_step(_tup(batches[it % 3]), 'google', 't2i', 'en', 1.0, 1.0, 1.0, 1.0)
            tr.iter()
    lines = [r.getMessage() for r in caplog.records if 'sent/s' in r.getMessage()]
    assert len(lines) == 2 and all('grad_norm:' in x and 'skipped:' in x for x in lines), lines
    assert 'skipped: 1' in lines[0] and 'skipped: 0' in lines[1]
    assert tr.last_guard_report['skipped_total'] == 1 and tr.last_guard_report['skipped_in_a_row'] == 0
    assert 0 < tr.last_guard_report['grad_norm'] < float('inf')
    g = tr.optimizers['model'].param_groups[0]
    assert g['num_updates'] == 9 and g['lr'] == tr.optimizers['model'].get_lr_for_step(9)
    assert bool(torch.isfinite(m.arena().master).all())


def test_trainer_stops_after_too_many_in_a_row(batches):
    tr, m = _trainer(skip_nonfinite_updates=True, max_skipped_in_a_row=2)
    _poison_next(tr, lambda i: True)
    for it in range(4):
        tr.pretrain_under_step(_tup(batches[0]), 'google', 't2i', 'en', 1.0, 1.0, 1.0, 1.0)
        tr.iter()                                   # (no print before the fifth iteration: nothing is read, nothing raised)
    tr.pretrain_under_step(_tup(batches[0]), 'google', 't2i', 'en', 1.0, 1.0, 1.0, 1.0)
    with pytest.raises(FloatingPointError, match=r'5 optimizer steps skipped in a row.*5 skipped in total'):
        tr.iter()
    assert bool(torch.isfinite(m.arena().master).all())


def test_parameter_off_keeps_the_statistics_and_the_line(batches, caplog):
    on, _ = _trainer(skip_nonfinite_updates=True)
    off, m = _trainer()
    assert off.optimizers['model'].guard_nonfinite is False and off.skip_nonfinite_updates is False
    with caplog.at_level(logging.INFO):
        for it in range(5):
            for tr in (on, off):
                tr.pretrain_under_step(_tup(batches[0]), 'google', 't2i', 'en', 1.0, 1.0, 1.0, 1.0)
            off.iter()
    assert list(off.stats) == list(on.stats) and not any('skipped' in k or 'grad_norm' in k for k in off.stats)
    lines = [r.getMessage() for r in caplog.records if 'sent/s' in r.getMessage()]
    assert len(lines) == 1 and 'skipped' not in lines[0] and 'grad_norm' not in lines[0]
    assert off.optimizers['model']._guard is None and not hasattr(off, 'last_guard_report')


# ---- a forced one-rank data-parallel world (M3P_DP_FORCE=1), both exchange modes, in a fresh child process -------------
def _dp_worker(port, q, mode):
    import torch.distributed as dist
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK='0', WORLD_SIZE='1', HSA_ENABLE_IPC_MODE_LEGACY='0',
                          M3P_DP_MODE=mode, M3P_DP_FORCE='1')
        torch.cuda.set_device(0)
        dist.init_process_group('nccl', rank=0, world_size=1)
        import tests.test_distributed_gpu as D
        real_params = D._params

        def params(scenario, multi_gpu):
            P = real_params(scenario, multi_gpu)
            P.skip_nonfinite_updates = True
            return P
        D._params = params
        tr, m = D._build('pretrain', True)
        opt = tr.optimizers['model']
        assert opt.guard_nonfinite is True and tr.model.mode == mode
        wrapped = not tr.model.single
        _poison_next(tr, lambda i: i == 1)
        ent = next(iter(opt._arenas.values()))
        ar = m.arena()

        def state():
            tr.model.materialize_master()
            torch.cuda.synchronize()
            return dict(p=ar.master.clone(), m=ent['m'].clone(), v=ent['v'].clone(), w=ar.w16.clone())
        full, extra = D._batches(0)
        tup = D._slice(full, extra, slice(0, D.CFG['B']), slice(0, D.CFG['B'] // 2))
        D._run_step(tr, 'pretrain', tup)
        snap = state()
        assert float(snap['m'].abs().max()) > 0
        D._run_step(tr, 'pretrain', tup)             # the poisoned one
        now = state()
        for c in 'pmvw':
            assert_bits_equal(now[c], snap[c], '%s after the bad step (%s)' % (c, mode))
        ar.ensure_zero()
        report = opt.reconcile()
        q.put(('ok', report, wrapped, float(torch.nan_to_num(ar.grad, nan=1.0).abs().max())))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        q.put(('err', traceback.format_exc(), False, 0.0))
        raise


@pytest.mark.parametrize('mode', ['zero1', 'allreduce'])
def test_one_rank_world_skips_alike(mode):
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    proc = ctx.Process(target=_dp_worker, args=(_free_port(), q, mode))
    proc.start()
    status, report, wrapped, leftover = q.get(timeout=600)
    proc.join(timeout=120)
    assert status == 'ok', report
    assert wrapped, 'M3P_DP_FORCE=1 did not put the one-rank world on the data-parallel path'
    assert report['attempts'] == 2 and report['skipped_total'] == 1 and leftover == 0.0
