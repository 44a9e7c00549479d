"""Exponential moving average of the weights, the CPU side: the NumPy twin that specifies m3p_ema_update's arithmetic, the
optimizer's schedule / context / state on a CPU model (parameters outside an arena: the torch form, three roundings),
the trainer's parameters and checkpoints, and DataParallel.materialize_ema on the two-rank gloo harness of
tests/test_distributed_cpu.py."""
import logging
import os
import traceback
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from m3p_amd import optim as Om
from m3p_amd import synth


def fma32(a, b, c):
    """fp32(a * b + c) with ONE rounding, for float32 arrays.  In fp64 the product of two fp32 values is exact; the sum with c
    rounds to 53 bits, and rounding that again to 24 could land on the wrong side of a tie.  So the fp64 sum is first made a
    round-to-odd sum - where it was inexact (TwoSum's error term) and its last bit is even, it steps to its neighbour on the
    side of the error - which no later rounding to fewer than 52 bits can tell from the exact value."""
    a, b, c = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c))
    prod = a * b
    s = prod + c
    with np.errstate(invalid='ignore'):
        bb = s - prod
        err = (prod - (s - bb)) + (c - bb)
        even = (s.view(np.int64) & 1) == 0
        step = np.isfinite(s) & np.isfinite(err) & (err != 0) & even
        s = np.where(step, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def ema_twin(e, p, w, contract=False):
    """The EMA rule e + w (p - e) in fp32.  e, p: float32 arrays; w: the fp32 value of 1 - decay.
    contract=False: the difference, the product and the sum are each rounded, in that order - what the torch form for
    parameters outside an arena does.  contract=True: the difference is rounded, then product and sum are one fused
    multiply-add - the rule of m3p_ema_update (include/m3p_hip.h), to the bit."""
    e, p, w = np.asarray(e, dtype=np.float32), np.asarray(p, dtype=np.float32), np.float32(w)
    d = p - e
    if contract:
        return fma32(np.broadcast_to(w, d.shape), d, e)
    s = d * w
    out = e + s
    assert d.dtype == s.dtype == out.dtype == np.float32
    return out


def w_of(decay):
    """1 - decay formed in double, rounded to fp32 once: what enable_ema hands the kernel."""
    return np.float32(1.0 - float(decay))


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


def same_bits(t, ref):
    return np.array_equal(bits(t.detach().cpu().numpy() if torch.is_tensor(t) else t), bits(ref.detach().cpu().numpy() if torch.is_tensor(ref) else ref))


# ---- 1. the twin against fp64 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('contract', [False, True], ids=['three_roundings', 'fused'])
@pytest.mark.parametrize('decay', [0.5, 0.9, 0.999, 0.9999, 1e-3])
def test_twin_is_within_five_roundings_of_fp64(decay, contract):
    """|twin - fp64| <= 2^-21 max(|e|, |p|) per element: the difference is off by at most 2^-24 |p - e| <= 2^-23 max, the
    product (w < 1) carries that and adds 2^-24 |s| <= 2^-23 max, the sum adds 2^-24 |e + s| <= 2^-24 max - five units of
    2^-24 max, and 2^-21 is eight.  Contraction takes the product's own rounding away."""
    rs = np.random.RandomState(7)
    n = 1 << 16
    e = (rs.standard_normal(n) * np.exp(rs.uniform(-12, 6, n))).astype(np.float32)
    p = (e * (1 + rs.standard_normal(n) * np.exp(rs.uniform(-14, 0, n)))).astype(np.float32)
    p[::7] = (rs.standard_normal(n) * np.exp(rs.uniform(-12, 6, n))).astype(np.float32)[::7]      # unrelated pairs, both signs
    p[::11], e[::13] = 0.0, 0.0
    w = w_of(decay)
    got = ema_twin(e, p, w, contract).astype(np.float64)
    ref = e.astype(np.float64) + np.float64(w) * (p.astype(np.float64) - e.astype(np.float64))
    bound = 2.0 ** -21 * np.maximum(np.abs(e), np.abs(p)).astype(np.float64)
    err = np.abs(got - ref)
    assert (err <= bound).all(), 'worst error / bound %.3f' % float((err / np.maximum(bound, 1e-300)).max())
    assert float((err / np.maximum(bound, 1e-300)).max()) > 0.01        # (the bound is not vacuous: roundings do happen)


def test_fma32_rounds_once():
    """Against exact rational arithmetic, on pairs built to sit next to ties of the final rounding."""
    from fractions import Fraction
    rs = np.random.RandomState(3)
    n = 4000
    a = rs.standard_normal(n).astype(np.float32)
    b = rs.standard_normal(n).astype(np.float32)
    c = (rs.standard_normal(n) * np.exp(rs.uniform(-3, 12, n))).astype(np.float32)       # c often far above a * b: ties and near-ties
    # a * b = 2^-24 (1 + 2^-24 - 2^-47): rounded on its own it is 2^-24 and 1 + 2^-24 is a tie that goes to 1; fused, the sum
    # lies above the tie and goes to 1 + 2^-23.  Both signs.
    sign = np.where(np.arange(50) % 2 == 0, 1.0, -1.0).astype(np.float32)
    a[:50] = np.float32(1.0 + 2.0 ** -23)
    b[:50] = sign * np.float32((1.0 - 2.0 ** -24) * 2.0 ** -24)
    c[:50] = sign
    got = fma32(a, b, c)
    assert np.array_equal(got[:50], sign * np.float32(1.0 + 2.0 ** -23))
    for i in range(n):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = sorted((np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))))
        dist = abs(Fraction(float(got[i])) - exact)
        for other in (lo, hi):
            d2 = abs(Fraction(float(other)) - exact)
            assert dist < d2 or (dist == d2 and (int(bits(got[i:i + 1])[0]) & 1) == 0), (i, a[i], b[i], c[i], got[i])
    assert np.array_equal(a[:50] * b[:50] + c[:50], sign), 'the cases tell one rounding from two'


@pytest.mark.parametrize('contract', [False, True])
def test_w_equal_one_is_not_a_copy(contract):
    """Why the first update is a copy and not a launch with w = 1: e + (p - e) is not p in fp32."""
    e = np.float32([1.0, 3.0])
    p = np.float32([1e-8, 1.0000001])
    assert not np.array_equal(bits(ema_twin(e, p, 1.0, contract)), bits(p))


# ---- 2. the optimizer on a CPU model (the loose path) --------------------------------------------------------------------
def _cpu_model(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3))


def _cpu_step(model, opt, k):
    g = torch.Generator().manual_seed(100 + k)
    x = torch.randn(4, 7, generator=g)
    opt.zero_grad()
    model(x).pow(2).sum().backward()
    opt.step()


@pytest.mark.parametrize('spec', ['adam,lr=0.01', 'lamb,lr=0.01', 'adam_inverse_sqrt,lr=0.01,warmup_updates=2', 'lamb_cosine,lr=0.01,warmup_updates=2'])
def test_three_steps_follow_the_twin(spec):
    model = _cpu_model()
    opt = Om.get_optimizer(model.parameters(), spec)
    params = list(model.parameters())
    start_bits = [p.detach().clone() for p in params]
    opt.enable_ema(0.5)
    for p, s in zip(params, start_bits):
        assert same_bits(opt.state[p]['ema'], s) and opt.state[p]['ema'].data_ptr() != p.data_ptr()
    w = w_of(0.5)
    prev = None
    for k in range(3):
        _cpu_step(model, opt, k)
        now = [p.detach().numpy().copy() for p in params]
        want = now if k == 0 else [ema_twin(e, p, w) for e, p in zip(prev, now)]      # call 0 = start: a bit copy
        for p, ref in zip(params, want):
            assert same_bits(opt.state[p]['ema'], ref), 'call %d' % k
        prev = [opt.state[p]['ema'].numpy().copy() for p in params]
    assert not same_bits(opt.state[params[0]]['ema'], params[0]), 'after three steps the EMA lags the weights'


@pytest.mark.parametrize('every,start', [(2, 1), (1, 0), (3, 0), (1, 2)])
def test_schedule_updates_on_exactly_the_calls_the_rule_names(every, start):
    model = _cpu_model()
    opt = Om.get_optimizer(model.parameters(), 'adam,lr=0.01')
    params = list(model.parameters())
    opt.enable_ema(0.5, every=every, start=start)
    w = w_of(0.5)
    ema = [p.detach().numpy().copy() for p in params]          # until `start` the EMA holds the weights of enable_ema
    for k in range(6):
        _cpu_step(model, opt, k)
        now = [p.detach().numpy().copy() for p in params]
        if k == start:
            ema = now                                          # the first update: a bit copy
        elif k > start and (k - start) % every == 0:
            ema = [ema_twin(e, p, w) for e, p in zip(ema, now)]
        for p, ref in zip(params, ema):
            assert same_bits(opt.state[p]['ema'], ref), 'call %d (every %d, start %d)' % (k, every, start)


def test_enable_ema_validates():
    model = _cpu_model()
    opt = Om.get_optimizer(model.parameters(), 'adam,lr=0.01')
    assert opt._ema is None and all('ema' not in opt.state[p] for p in model.parameters())
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            opt.enable_ema(bad)
    with pytest.raises(ValueError):
        opt.enable_ema(0.9, every=0)
    with pytest.raises(ValueError):
        opt.enable_ema(0.9, start=-1)
    for what in (opt.ema_state, opt.materialize_ema, lambda: opt.load_ema_state({})):
        with pytest.raises(RuntimeError):
            what()
    with pytest.raises(RuntimeError):
        with opt.ema_weights():
            pass
    opt.enable_ema(0.9)
    with pytest.raises(RuntimeError):
        opt.enable_ema(0.9)


# ---- 3. ema_weights() ----------------------------------------------------------------------------------------------------
def test_ema_weights_swaps_and_restores_to_the_bit():
    model = _cpu_model()
    opt = Om.get_optimizer(model.parameters(), 'adam,lr=0.05')
    params = list(model.parameters())
    opt.enable_ema(0.5)
    for k in range(3):
        _cpu_step(model, opt, k)
    raw = [p.detach().clone() for p in params]
    ema = [opt.state[p]['ema'].clone() for p in params]
    versions = [p._version for p in params]
    assert not any(same_bits(r, e) for r, e in zip(raw, ema))
    with opt.ema_weights() as inside:
        assert inside is opt
        for p, r, e, v in zip(params, raw, ema, versions):
            assert same_bits(p.data, e) and same_bits(opt.state[p]['ema'], r) and p._version > v
        with pytest.raises(RuntimeError, match='nest'):
            with opt.ema_weights():
                pass
        with pytest.raises(RuntimeError, match='inside ema_weights'):
            opt.step()
        with pytest.raises(RuntimeError):
            opt.ema_state()
        for p, e in zip(params, ema):          # the refusals changed nothing
            assert same_bits(p.data, e)
    for p, r, e in zip(params, raw, ema):
        assert same_bits(p.data, r) and same_bits(opt.state[p]['ema'], e)
    _cpu_step(model, opt, 3)                   # training goes on, and the update uses the raw weights
    w = w_of(0.5)
    for p, e in zip(params, ema):
        assert same_bits(opt.state[p]['ema'], ema_twin(e.numpy(), p.detach().numpy(), w))


def test_an_exception_inside_still_swaps_back():
    model = _cpu_model()
    opt = Om.get_optimizer(model.parameters(), 'adam,lr=0.05')
    opt.enable_ema(0.5)
    for k in range(2):
        _cpu_step(model, opt, k)
    raw = [p.detach().clone() for p in model.parameters()]
    with pytest.raises(KeyError):
        with opt.ema_weights():
            raise KeyError('boom')
    assert all(same_bits(p.data, r) for p, r in zip(model.parameters(), raw)) and opt._ema['inside'] is False


def test_ema_state_round_trip_and_missing_names(caplog):
    model = _cpu_model()
    opt = Om.get_optimizer(model.parameters(), 'adam,lr=0.05')
    opt.enable_ema(0.5)
    for k in range(3):
        _cpu_step(model, opt, k)
    named = list(model.state_dict(keep_vars=True).items())
    sd = opt.ema_state(named)
    assert list(sd) == [k for k, _ in named] and all(v.dtype == torch.float32 and v.device.type == 'cpu' for v in sd.values())
    for k, p in named:
        assert same_bits(sd[k], opt.state[p]['ema']) and sd[k].data_ptr() != opt.state[p]['ema'].data_ptr()
    assert sorted(opt.ema_state()) == sorted('group0.%d' % i for i in range(4))
    other = _cpu_model(seed=1)
    other.load_state_dict(sd)                                  # state-dict form: it loads into a model
    opt2 = Om.get_optimizer(other.parameters(), 'adam,lr=0.05')
    opt2.enable_ema(0.9)
    named2 = list(other.state_dict(keep_vars=True).items())
    partial = {k: v + 1 for k, v in list(sd.items())[:2]}
    with caplog.at_level(logging.WARNING):
        opt2.load_ema_state(partial, named2)
    assert len([r for r in caplog.records if 'load_ema_state' in r.getMessage()]) == 1
    for i, (k, p) in enumerate(named2):
        assert same_bits(opt2.state[p]['ema'], partial[k] if i < 2 else p.data)


# ---- 4. the trainer ---------------------------------------------------------------------------------------------------------
def _trainer(tmp_path, **over):
    from m3p_amd.model.transformer import TransformerModel
    from m3p_amd.trainer import XTrainer
    P = synth.model_params(64, 2, 2, 120)
    for k, v in dict(optimizer='adam_inverse_sqrt,beta1=0.9,beta2=0.98,lr=0.01,warmup_updates=1', clip_grad_norm=5, amp=-1, fp16=False,
                     accumulate_gradients=1, multi_gpu=False, local_rank=0, epoch_size=10, batch_size=2, is_master=True,
                     dump_path=str(tmp_path), reload_checkpoint='', validation_metrics='_valid_loss',
                     stopping_criterion='', save_periodic=0, langs=['en'], cross_rel_steps=[('coco', 'img')], cross_mlm_steps=[]).items():
        setattr(P, k, v)
    for k, v in over.items():
        setattr(P, k, v)
    torch.manual_seed(3)
    m = TransformerModel(P, is_encoder=True, with_output=True, is_crossModal=True)
    return XTrainer(m, {}, P), m, P


def _fake_steps(tr, m, n, seed=0):
    """n optimizer steps on hand-made gradients (the CPU model has no forward: the hot path is the GPU's)."""
    g = torch.Generator().manual_seed(seed)
    opt = tr.optimizers['model']
    for _ in range(n):
        for p in m.parameters():
            p.grad = torch.randn(p.shape, generator=g) * 0.1
        opt.step()


def test_trainer_without_ema_decay_is_as_before(tmp_path):
    tr, m, P = _trainer(tmp_path)
    assert tr.ema_decay == 0 and tr.ema_eval is False and tr.optimizers['model']._ema is None
    _fake_steps(tr, m, 2)
    assert not any('ema' in st for st in tr.optimizers['model'].state.values())
    tr.save_checkpoint('ck')
    tr.save_best_model({'valid_loss': 1.0})
    for name in ('ck.pth', 'best-valid_loss.pth'):
        ck = torch.load(os.path.join(str(tmp_path), name), map_location='cpu', weights_only=False)
        assert not any('ema' in k for k in ck), sorted(ck)
        assert not any('ema' in st for st in ck['model_optimizer']['state'].values())
    with pytest.raises(RuntimeError):
        with tr.ema_weights():
            pass


def test_trainer_checkpoint_restores_the_ema_bit_for_bit(tmp_path, caplog):
    tr, m, P = _trainer(tmp_path, ema_decay=0.5, ema_every=1, ema_start=0)
    opt = tr.optimizers['model']
    assert tr.ema_decay == 0.5 and tr.ema_eval is True and opt._ema['decay'] == 0.5
    _fake_steps(tr, m, 3)
    named = list(m.state_dict(keep_vars=True).items())
    ema = {k: opt._ema_of(p).clone() for k, p in named}
    raw = {k: p.detach().clone() for k, p in named}
    assert not same_bits(ema['embeddings.weight'], raw['embeddings.weight'])
    tr.save_checkpoint('checkpoint')
    tr.save_model('plain')
    ck = torch.load(os.path.join(str(tmp_path), 'checkpoint.pth'), map_location='cpu', weights_only=False)
    assert 'model_ema' in ck and list(ck['model_ema']) == list(ck['model'])
    assert all(same_bits(ck['model_ema'][k], ema[k]) and same_bits(ck['model'][k], raw[k]) for k in ema)
    assert not any('ema' in st for st in ck['model_optimizer']['state'].values()), 'the EMA travels once'
    assert all('ema' in opt.state[p] for p in m.parameters()), 'saving took nothing out of the live state'
    plain = torch.load(os.path.join(str(tmp_path), 'plain.pth'), map_location='cpu', weights_only=False)
    assert 'model_ema' not in plain and all(same_bits(plain['model'][k], raw[k]) for k in raw)      # save_model: the raw weights
    # a fresh trainer on the same dump_path resumes with the EMA's bits
    tr2, m2, _ = _trainer(tmp_path, ema_decay=0.5)
    opt2 = tr2.optimizers['model']
    for k, p in m2.state_dict(keep_vars=True).items():
        assert same_bits(p.data, raw[k]) and same_bits(opt2._ema_of(p), ema[k]), k
    # best-<metric>.pth is written from inside the context: it holds the averaged weights, the ones that scored
    tr.save_best_model({'valid_loss': 1.0})
    best = torch.load(os.path.join(str(tmp_path), 'best-valid_loss.pth'), map_location='cpu', weights_only=False)
    assert all(same_bits(best['model'][k], ema[k]) and same_bits(best['model_ema'][k], ema[k]) for k in ema)
    assert all(same_bits(p.data, raw[k]) and same_bits(opt._ema_of(p), ema[k]) for k, p in named), 'and everything is back'
    # ema_eval off: the best model is the raw one
    tr3, m3, _ = _trainer(tmp_path / 'raw', ema_decay=0.5, ema_eval=False)
    os.makedirs(str(tmp_path / 'raw'), exist_ok=True)
    _fake_steps(tr3, m3, 2)
    tr3.save_best_model({'valid_loss': 1.0})
    best3 = torch.load(os.path.join(str(tmp_path / 'raw'), 'best-valid_loss.pth'), map_location='cpu', weights_only=False)
    assert all(same_bits(best3['model'][k], p.data) for k, p in m3.state_dict(keep_vars=True).items())
    # a checkpoint without the key: the EMA starts at the loaded weights, with one log line
    del ck['model_ema']
    os.makedirs(str(tmp_path / 'old'), exist_ok=True)
    torch.save(ck, os.path.join(str(tmp_path / 'old'), 'checkpoint.pth'))
    with caplog.at_level(logging.WARNING):
        caplog.clear()
        tr4, m4, _ = _trainer(tmp_path / 'old', ema_decay=0.5)
    assert len([r for r in caplog.records if 'ema' in r.getMessage().lower()]) == 1
    for k, p in m4.state_dict(keep_vars=True).items():
        assert same_bits(p.data, raw[k]) and same_bits(tr4.optimizers['model']._ema_of(p), raw[k]), k
    # and an EMA checkpoint loads into a trainer without EMA (the key is ignored)
    tr5, m5, _ = _trainer(tmp_path)
    assert tr5.optimizers['model']._ema is None and same_bits(m5.embeddings.weight.data, raw['embeddings.weight'])


def test_trainer_ema_weights_context(tmp_path):
    tr, m, P = _trainer(tmp_path, ema_decay=0.5, ema_every=2, ema_start=1)
    opt = tr.optimizers['model']
    assert opt._ema['every'] == 2 and opt._ema['start'] == 1
    _fake_steps(tr, m, 4)
    raw = m.embeddings.weight.detach().clone()
    ema = opt._ema_of(m.embeddings.weight).clone()
    from m3p_amd.evaluation import run_all_evals
    seen = []

    def get_iterator(*a):
        raise AssertionError('no data set is configured')
    Q = SimpleNamespace(is_master=True)
    with tr.ema_weights():
        assert same_bits(m.embeddings.weight.data, ema)
    assert same_bits(m.embeddings.weight.data, raw)
    import m3p_amd.evaluation as E
    real = E._run_all_evals
    E._run_all_evals = lambda *a: (seen.append(m.embeddings.weight.detach().clone()), real(*a))[1]
    try:
        assert run_all_evals(m, Q, get_iterator, 4, ema=tr.ema_weights()) == {'epoch': 4}
        assert run_all_evals(m, Q, get_iterator, 5) == {'epoch': 5}
    finally:
        E._run_all_evals = real
    assert same_bits(seen[0], ema) and same_bits(seen[1], raw) and same_bits(m.embeddings.weight.data, raw)


def test_trainer_refuses_an_optimizer_without_ema(tmp_path):
    with pytest.raises(ValueError, match='ema_decay needs one of the fused optimizers'):
        _trainer(tmp_path, ema_decay=0.9, optimizer='sgd,lr=0.1')


# ---- 5. the spec syntax is untouched ------------------------------------------------------------------------------------------
def test_optimizer_specs_do_not_know_ema():
    assert Om.parse_optimizer_spec('adam,lr=0.001') == ('adam', {'lr': 0.001})
    with pytest.raises(Exception, match='Unexpected parameters'):
        Om.get_optimizer(_cpu_model().parameters(), 'adam,lr=0.001,ema_decay=0.9')
    for name in ('adam', 'lamb', 'adam_cosine', 'lamb_inverse_sqrt'):
        opt = Om.get_optimizer(_cpu_model().parameters(), name + ',lr=0.001')
        assert opt._ema is None and hasattr(opt, 'enable_ema')


def test_abi_has_the_two_symbols():
    from m3p_amd import lib as L
    from tests.test_lib_abi import _declared
    assert {'m3p_ema_update', 'm3p_ema_swap'} <= set(_declared()) and {'m3p_ema_update', 'm3p_ema_swap'} <= set(L.SIGNATURES)
    assert L.SIGNATURES['m3p_ema_update'][1][5] is L.C.c_float and len(L.SIGNATURES['m3p_ema_swap'][1]) == 7


# ---- DataParallel.materialize_ema on the two-rank gloo harness (a fake arena: the optimizer's arena path needs the device) --
def _gather_worker(rank, world, port, q, mode):
    import torch.distributed as dist
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        torch.set_num_threads(1)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        from m3p_amd.distributed import DataParallel
        from tests.test_distributed_cpu import _FakeModel
        model = _FakeModel()
        dp = DataParallel(model, mode=mode)
        total = model.arena().total
        # every rank holds its own shards of the "true" EMA (element i = i + 0.5) and rubbish elsewhere
        ema = torch.full((total,), -1000.0 - rank)
        truth = torch.arange(total, dtype=torch.float32) + 0.5
        for a, b in dp.owned(0, total):
            ema[a:b] = truth[a:b]
        owned = sum(b - a for a, b in dp.owned(0, total))
        dp.materialize_ema(ema)
        q.put((rank, 'ok', owned, bool(torch.equal(ema, truth)) if mode == 'zero1' else int((ema == truth).sum())))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        q.put((rank, 'err', traceback.format_exc(), False))
        raise


@pytest.mark.parametrize('mode', ['zero1', 'allreduce'])
def test_materialize_ema_two_ranks(mode):
    import torch.multiprocessing as mp
    from tests.test_distributed_cpu import _FakeModel, _free_port
    total = _FakeModel().arena().total
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gather_worker, args=(r, 2, port, q, mode)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    for rank, status, owned, full in got:
        assert status == 'ok', owned
        if mode == 'zero1':
            assert owned == total // 2 and full is True, 'rank %d holds the whole EMA after the gather' % rank
        else:
            assert owned == total and full == total, 'replicated: every rank owns and keeps everything'
