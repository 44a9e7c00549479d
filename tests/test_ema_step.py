"""The exponential moving average through real steps on cfg1: Adam.enable_ema behind real backward passes for three optimizer
families, with the non-finite guard, the ema_weights() context down to an evaluation forward, and a forced one-rank
data-parallel world in both exchange modes.

The steps themselves are not bit-reproducible (fp32 atomics in backward), so every check is per step, on this run's own
buffers: the EMA after a step against the NumPy twin (tests/test_ema_cpu.py) of the EMA before it and the master after it."""
import os
import traceback

import numpy as np
import pytest
import torch

from m3p_amd import synth
from tests.test_ema_cpu import ema_twin, w_of
from tests.test_lamb_step import _free_port
from tests.test_model_parity import _build, _losses
from tests.test_nonfinite_guard_step import SPECS, _step
from tests.util import assert_bits_equal, assert_exact_zero

pytestmark = pytest.mark.gpu

CFG = synth.CONFIGS['cfg1']
DECAY = 0.9


@pytest.fixture(scope='module')
def batches():
    return [synth.make_batch(CFG['T'], CFG['R'], CFG['B'], CFG['n_words'], CFG['n_pred'], seed=200 + k) for k in range(4)]


def _fresh(spec, guard=False, **ema):
    from m3p_amd import optim as Om
    m, P, sd = _build(CFG)
    opt = Om.get_optimizer(m.parameters(), SPECS[spec])
    opt.guard_nonfinite = guard
    opt.enable_ema(DECAY, **ema)
    return m, opt, next(iter(opt._arenas.values()))


def _host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy()


def _assert_follows_twin(ent, ar, before, what):
    want = ema_twin(before, _host(ar.master), w_of(DECAY), contract=True)      # the kernel's form: one fused multiply-add
    assert_bits_equal(ent['ema'], torch.from_numpy(want), what)


def _assert_padding_zero(ent, ar, what):
    pos = 0
    for name, (o, cnt, _) in ar.offsets.items():
        assert_exact_zero(ent['ema'][pos:o], '%s: EMA padding in front of %s' % (what, name))
        pos = o + cnt
    assert_exact_zero(ent['ema'][pos:], '%s: EMA padding behind the last parameter' % what)


# ---- 10. three real steps ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('spec', sorted(SPECS))
def test_three_steps_follow_the_twin(spec, batches):
    m, opt, ent = _fresh(spec)
    ar = m.arena()
    assert ent['ema'].shape == ar.master.shape and ent['ema'].data_ptr() != ar.master.data_ptr()
    assert_bits_equal(ent['ema'], ar.master, 'the EMA starts as a copy of the master')
    p = ar.params['layer_norm_emb.bias']
    o, cnt, _ = ar.offsets['layer_norm_emb.bias']
    assert opt.state[p]['ema'].data_ptr() == ent['ema'][o:o + cnt].data_ptr(), 'state[p][ema] is a view of the EMA arena'
    for k in range(3):
        before = _host(ent['ema'])
        master_before = _host(ar.master)
        _step(m, opt, batches[k], 5.0)
        assert not np.array_equal(master_before, _host(ar.master)), 'the step moved the weights'
        if k == 0:                    # call 0 = start: a copy
            assert_bits_equal(ent['ema'], ar.master, '%s: the first update is a copy of the master' % spec)
        else:
            _assert_follows_twin(ent, ar, before, '%s: EMA after step %d' % (spec, k))
            assert not torch.equal(ent['ema'], ar.master)
        _assert_padding_zero(ent, ar, '%s step %d' % (spec, k))
    # a tensor that sat out a step (the ITM head under an MLM-only loss) still decays towards its value
    before = _host(ent['ema'])
    out, mlm, rel, bce = _losses(m, batches[3], CFG['R'])
    mlm.backward()
    untouched = [n for n in ar.names if n not in ar.touched]
    assert untouched
    opt.step()
    _assert_follows_twin(ent, ar, before, '%s: EMA after an MLM-only step' % spec)


def test_every_and_start_on_the_arena(batches):
    m, opt, ent = _fresh('adam', every=2, start=1)
    ar = m.arena()
    start_bits = _host(ent['ema'])
    _step(m, opt, batches[0], 5.0)                              # call 0: before start
    assert_bits_equal(ent['ema'], torch.from_numpy(start_bits), 'call 0')
    _step(m, opt, batches[1], 5.0)                              # call 1 = start: copy
    assert_bits_equal(ent['ema'], ar.master, 'call 1')
    before = _host(ent['ema'])
    _step(m, opt, batches[2], 5.0)                              # call 2: off the schedule
    assert_bits_equal(ent['ema'], torch.from_numpy(before), 'call 2')
    _step(m, opt, batches[3], 5.0)                              # call 3: update
    _assert_follows_twin(ent, ar, before, 'call 3')


# ---- 11. with the guard -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('spec', sorted(SPECS))
def test_skipped_step_leaves_the_ema_alone(spec, batches):
    m, opt, ent = _fresh(spec, guard=True)
    ar = m.arena()
    _step(m, opt, batches[0], 5.0)
    before = _host(ent['ema'])
    _step(m, opt, batches[1], 5.0)
    _assert_follows_twin(ent, ar, before, '%s: guarded clean step' % spec)
    before = _host(ent['ema'])
    master = _host(ar.master)
    _step(m, opt, batches[2], 5.0, bad='nan_loss')
    assert_bits_equal(ent['ema'], torch.from_numpy(before), '%s: EMA after the skipped step' % spec)
    assert_bits_equal(ar.master, torch.from_numpy(master), '%s: master after the skipped step' % spec)
    _step(m, opt, batches[3], 5.0)
    _assert_follows_twin(ent, ar, before, '%s: the clean step after the skipped one' % spec)
    assert not np.array_equal(_host(ent['ema']), before)
    assert opt.reconcile()['skipped_total'] == 1 and bool(torch.isfinite(ent['ema']).all())


# ---- 12. ema_weights() ---------------------------------------------------------------------------------------------------------
def _eval_losses(m, batch):
    m.eval()
    with torch.no_grad():
        out, mlm, rel, bce = _losses(m, batch, CFG['R'])
    torch.cuda.synchronize()
    return torch.stack([mlm.detach().float().reshape(()), bce.detach().float().reshape(())]).cpu()


def test_ema_weights_context(batches):
    """The evaluation forward inside the context against a second model that loaded ema_state(): both run the same kernels on
    the same bits without dropout.  Repeated identical forwards are compared first; where they are bit-equal the two models
    must be, else they may differ by at most the largest difference seen between repeats (as test_twin_runs bounds its runs).
    On the MI355X the repeats are bit-equal and so are the two models."""
    m, opt, ent = _fresh('adam_inverse_sqrt')
    ar = m.arena()
    for k in range(3):
        _step(m, opt, batches[k], 5.0)
    ar.refresh()
    torch.cuda.synchronize()
    raw = dict(p=ar.master.clone(), w=ar.w16.clone(), e=ent['ema'].clone(), t=ar.wt[('qkv', 0)].clone())
    named = list(m.state_dict(keep_vars=True).items())
    saved = opt.ema_state(named)
    epoch = ar.epoch
    with opt.ema_weights():
        torch.cuda.synchronize()
        assert_bits_equal(ar.master, raw['e'], 'master inside the context')
        assert_bits_equal(ar.w16, raw['e'].to(torch.bfloat16), 'bf16 copy inside the context')
        assert_bits_equal(ent['ema'], raw['p'], 'the EMA buffer holds the raw weights inside the context')
        assert ar.epoch > epoch and ar._transposes_stale
        ar.refresh()
        torch.cuda.synchronize()
        assert_bits_equal(ar.wt[('qkv', 0)], ar.qkv_w16(0).t().contiguous(), 'transposed qkv copy inside the context')
        assert not torch.equal(ar.wt[('qkv', 0)], raw['t'])
        assert_bits_equal(ar.w16, raw['e'].to(torch.bfloat16), 'refresh() did not cast again')
        inside = [_eval_losses(m, batches[3]) for _ in range(3)]
        with pytest.raises(RuntimeError, match='nest'):
            with opt.ema_weights():
                pass
        with pytest.raises(RuntimeError, match='inside ema_weights'):
            opt.step()
    torch.cuda.synchronize()
    assert_bits_equal(ar.master, raw['p'], 'master after the context')
    assert_bits_equal(ar.w16, raw['w'], 'bf16 copy after the context')
    assert_bits_equal(ent['ema'], raw['e'], 'EMA after the context')
    ar.refresh()
    torch.cuda.synchronize()
    assert_bits_equal(ar.wt[('qkv', 0)], raw['t'], 'transposed qkv copy after the context')
    # a second model that loads the EMA
    m2, _, _ = _build(CFG)
    m2.load_state_dict(saved)
    assert_bits_equal(m2.embeddings.weight.data.cpu(), saved['embeddings.weight'], 'the second model holds the EMA')
    other = _eval_losses(m2, batches[3])
    noise = max(float((inside[0].double() - x.double()).abs().max()) for x in inside[1:])
    diff = float((inside[0].double() - other.double()).abs().max())
    print('eval losses inside ema_weights(): %s; second model: %s; repeat noise %.3e, difference %.3e'
          % (inside[0].tolist(), other.tolist(), noise, diff))
    raw_losses = _eval_losses(m, batches[3])
    assert not torch.equal(raw_losses, inside[0]), 'the averaged weights score differently from the raw ones'
    if noise == 0.0:
        assert_bits_equal(other, inside[0], 'losses of the second model against the context')
    else:
        assert diff <= noise
    # training goes on, and the update uses the raw weights
    m.train()
    before = _host(ent['ema'])
    _step(m, opt, batches[3], 5.0)
    _assert_follows_twin(ent, ar, before, 'the step after the context')
    # gradients pending: refused
    out, mlm, rel, bce = _losses(m, batches[0], CFG['R'])
    (mlm + bce).backward()
    with pytest.raises(RuntimeError, match='gradients are pending'):
        with opt.ema_weights():
            pass
    assert opt._ema['inside'] is False
    opt.zero_grad()
    with opt.ema_weights():
        pass


# ---- 13. a forced one-rank data-parallel world (M3P_DP_FORCE=1), both exchange modes, in a fresh child process -----------------
def _dp_worker(port, q, mode, dump):
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
            P.ema_decay, P.dump_path = DECAY, dump
            return P
        D._params = params
        tr, m = D._build('pretrain', True)
        opt = tr.optimizers['model']
        assert opt._ema is not None and tr.model.mode == mode and tr.ema_eval
        wrapped = not tr.model.single
        ent = next(iter(opt._arenas.values()))
        ar = m.arena()
        full, extra = D._batches(0)
        tup = D._slice(full, extra, slice(0, D.CFG['B']), slice(0, D.CFG['B'] // 2))
        D._run_step(tr, 'pretrain', tup)                     # call 0: the copy
        tr.model.materialize_master()
        opt.materialize_ema()
        torch.cuda.synchronize()
        assert_bits_equal(ent['ema'], ar.master, 'one-rank world (%s): the first update is a copy' % mode)
        before = _host(ent['ema'])
        D._run_step(tr, 'pretrain', tup)                     # call 1: the update
        assert ent['ema_partial'] is (mode == 'zero1')
        tr.model.materialize_master()
        opt.materialize_ema()
        assert ent['ema_partial'] is False
        _assert_follows_twin(ent, ar, before, 'one-rank world (%s): EMA after the second step' % mode)
        raw = dict(p=ar.master.clone(), w=ar.w16.clone(), e=ent['ema'].clone())
        with tr.ema_weights():
            torch.cuda.synchronize()
            assert_bits_equal(ar.master, raw['e'], 'master inside the context (%s)' % mode)
            assert_bits_equal(ar.w16, raw['e'].to(torch.bfloat16), 'bf16 copy inside the context (%s)' % mode)
        torch.cuda.synchronize()
        for c, t in (('p', ar.master), ('w', ar.w16), ('e', ent['ema'])):
            assert_bits_equal(t, raw[c], '%s after the context (%s)' % (c, mode))
        path = tr.save_checkpoint('ck')
        ck = torch.load(path, map_location='cpu', weights_only=False)
        ok = all(torch.equal(ck['model_ema'][k], opt._ema_of(p).detach().cpu()) for k, p in m.state_dict(keep_vars=True).items())
        D._run_step(tr, 'pretrain', tup)                     # and training goes on
        torch.cuda.synchronize()
        q.put(('ok', wrapped, ok and list(ck['model_ema']) == list(ck['model'])))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        q.put(('err', traceback.format_exc(), False))
        raise


@pytest.mark.parametrize('mode', ['zero1', 'allreduce'])
def test_one_rank_world(mode, tmp_path):
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    proc = ctx.Process(target=_dp_worker, args=(_free_port(), q, mode, str(tmp_path)))
    proc.start()
    status, wrapped, ck_ok = q.get(timeout=600)
    proc.join(timeout=120)
    assert status == 'ok', wrapped
    assert wrapped, 'M3P_DP_FORCE=1 did not put the one-rank world on the data-parallel path'
    assert ck_ok, 'the checkpoint carries the materialised EMA under model_ema, in state-dict form'
