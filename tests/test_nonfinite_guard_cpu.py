"""Host side of the non-finite guard (m3p_amd/optim.py roll_back, Adam.reconcile; Trainer's refusal of fp8 + guard), without a
GPU.  The roll-back arithmetic is checked against replaying the schedule WITHOUT the skipped attempts: the host bumps step
counts, num_updates and lr on every attempt (it cannot know the verdict), `roll_back` takes the skipped ones back out, and the
result must be what a run that never saw those batches holds."""
import types

import pytest

from m3p_amd import optim as Om

SEQUENCES = {
    'ok bad bad ok': [0, 1, 1, 0],
    'all bad': [1, 1, 1, 1, 1],
    'bad first': [1, 0, 0],
    '64 with skips at 0 and 63': [1] + [0] * 62 + [1],
}
SCHEDULES = {
    'adam_inverse_sqrt': Om.inverse_sqrt_schedule(peak_lr=1e-3, warmup=3, floor_lr=1e-7, power=0.5),
    # the warm-up ends at update 2, the first period at update 2 + 4: the run of 64 crosses both, the short ones the warm-up's end
    'adam_cosine': Om.cosine_schedule(peak_lr=1e-3, warmup=2, floor_lr=1e-7, min_lr=1e-9, period=4, period_mult=2, lr_shrink=0.75),
    'adam': None,
}


def _attempt_all(verdicts, lr_at, start_steps, start_updates, active=None):
    """What the host does over the attempts (every one bumps) -> (log, flags, steps, num_updates, lr)."""
    steps, updates = dict(start_steps), dict(start_updates)
    log, flags = [], {}
    for index, bad in enumerate(verdicts):
        keys = list(steps) if active is None else active[index]
        bumped = []
        for k in keys:
            steps[k] += 1
            bumped.append((k, steps[k]))
        for g in updates:
            updates[g] += 1
        log.append((index, bumped, list(updates)))
        flags[index] = bad
    return log, flags, steps, updates


def _replay_without(verdicts, start_steps, start_updates, active=None):
    """The run in which the skipped batches never existed."""
    steps, updates = dict(start_steps), dict(start_updates)
    for index, bad in enumerate(verdicts):
        if bad:
            continue
        for k in (list(steps) if active is None else active[index]):
            steps[k] += 1
        for g in updates:
            updates[g] += 1
    return steps, updates


@pytest.mark.parametrize('schedule', sorted(SCHEDULES))
@pytest.mark.parametrize('name', sorted(SEQUENCES))
def test_roll_back_equals_replaying_without_the_skipped_attempts(name, schedule):
    verdicts, lr_at = SEQUENCES[name], SCHEDULES[schedule]
    start_steps = {'w': 0, 'b': 0}
    start_updates = {'g0': 0} if lr_at is not None else {}
    log, flags, steps, updates = _attempt_all(verdicts, lr_at, start_steps, start_updates)
    before = (dict(steps), dict(updates))
    got_steps, got_updates = Om.roll_back(log, flags, steps, updates)
    assert (steps, updates) == before, 'roll_back changed its arguments'
    ref_steps, ref_updates = _replay_without(verdicts, start_steps, start_updates)
    assert got_steps == ref_steps and got_updates == ref_updates
    n_ok = len(verdicts) - sum(verdicts)
    assert all(v == n_ok for v in got_steps.values())
    if lr_at is not None:
        # the lr the optimizer resets is the schedule at the rolled-back count: the replay's lr after its last update
        lr_replay = lr_at(0)
        count = 0
        for bad in verdicts:
            if not bad:
                count += 1
                lr_replay = lr_at(count)
        assert lr_at(got_updates['g0']) == lr_replay
        if sum(verdicts) and n_ok >= 1:
            assert lr_at(len(verdicts)) != lr_replay, 'the case does not tell the rolled-back lr from the attempted one'


def test_two_parameters_with_different_counts_one_active_in_the_skipped_attempt():
    """A head that sat out steps lags behind; the skipped attempt touched the body only: the head's count stays."""
    start = {'body': 7, 'head': 3}
    verdicts = [0, 1, 0]
    active = [['body', 'head'], ['body'], ['body', 'head']]
    log, flags, steps, updates = _attempt_all(verdicts, None, start, {'g0': 7}, active)
    assert steps == {'body': 10, 'head': 5} and updates == {'g0': 10}
    got_steps, got_updates = Om.roll_back(log, flags, steps, updates)
    assert (got_steps, got_updates) == _replay_without(verdicts, start, {'g0': 7}, active) == ({'body': 9, 'head': 5}, {'g0': 9})


def test_roll_back_refuses_more_skips_than_counts():
    with pytest.raises(AssertionError):
        Om.roll_back([(0, [('w', 1)], [])], {0: 1}, {'w': 0}, {})


@pytest.mark.parametrize('spec', ['adam_inverse_sqrt,lr=0.001,warmup_updates=3', 'adam_cosine,lr=0.001,warmup_updates=2,init_period=4',
                                  'adam,lr=0.001', 'lamb_cosine,lr=0.001,warmup_updates=2,init_period=4'])
def test_reconcile_on_a_stub_guard_resets_counts_and_lr(spec):
    """Adam.reconcile with the device read replaced by a stub: the log made by hand as step() makes it."""
    import torch
    p, q = torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(3))
    opt = Om.get_optimizer([p, q], spec)
    assert opt.guard_nonfinite is False and isinstance(opt, Om.Adam)
    verdicts = [0, 1, 1, 0, 0, 0, 1, 0]
    scheduled = hasattr(opt, '_lr_at')
    for index, bad in enumerate(verdicts):             # what step() + _Scheduled.step() leave behind, attempt by attempt
        bumped = []
        for t in ((p, q) if index != 1 else (p,)):
            opt.state[t]['step'] += 1
            bumped.append((t, opt.state[t]['step']))
        opt._guard_log.append((index, bumped, [g for g in opt.param_groups if 'num_updates' in g]))
        opt._attempts += 1
        if scheduled:
            for g in opt.param_groups:
                g['num_updates'] += 1
                g['lr'] = opt._lr_at(g['num_updates'])
    ring = verdicts + [0] * (64 - len(verdicts))
    norms = [float(i + 1) if not bad else float('nan') for i, bad in enumerate(verdicts)] + [0.0] * (64 - len(verdicts))
    reads = []
    opt._guard = types.SimpleNamespace(read=lambda: (reads.append(1), ([8, 3, 0], norms, ring))[1])
    sd = opt.state_dict()                              # reconciles first
    assert set(sd) == {'state', 'param_groups'} and len(reads) == 1
    assert opt.state[p]['step'] == 5 and opt.state[q]['step'] == 5 + 1 - 1     # q sat out the skipped attempt 1
    if scheduled:
        g = opt.param_groups[0]
        assert g['num_updates'] == 5 and g['lr'] == opt.get_lr_for_step(5) and sd['param_groups'][0]['num_updates'] == 5
    assert opt._guard_log == []
    out = opt.reconcile()                              # nothing logged: counters only
    assert out == dict(attempts=8, skipped_total=3, skipped_in_a_row=0, norms=[]) and len(reads) == 2


def _trainer_params(**kw):
    return types.SimpleNamespace(epoch_size=10, **kw)


def test_trainer_refuses_fp8_with_the_guard():
    from m3p_amd.trainer import Trainer
    with pytest.raises(ValueError, match='fp8_gemm'):
        Trainer({}, _trainer_params(skip_nonfinite_updates=True, fp8_gemm=True))
    # either one alone gets past the refusal (and fails later, on what this stub lacks - not with the ValueError)
    for kw in (dict(skip_nonfinite_updates=True), dict(fp8_gemm=True), dict()):
        with pytest.raises(AttributeError):
            Trainer({}, _trainer_params(**kw))
