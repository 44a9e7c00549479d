"""Optimizers of the hot path: drop-in for ``M3P/src/optim.py`` (Adam :16-86,
AdamInverseSqrtWithWarmup :89-139, get_optimizer :211-270) with the per-tensor Python
loop replaced by fused HIP kernels over the model's flat arenas
(csrc/optim.hip: m3p_sumsq_f32 + m3p_adam_step = clip + Adam + bf16 refresh + zero_grad in
one pass over p, g, m, v).

Semantics kept from the reference:
  * state is allocated eagerly in the constructor; ``state[p]`` holds ``step`` (int),
    ``exp_avg``, ``exp_avg_sq`` (here: views into flat moment arenas);
  * parameters that received no gradient in a step are skipped entirely (optim.py:55-56);
  * eps is added to sqrt(v) before the bias-corrected step size is applied;
    weight decay is the decoupled ``p -= wd * lr * p`` (:81-82);
  * AdamInverseSqrtWithWarmup is constructed with lr = warmup_init_lr and moves the lr
    *after* each step (:135-139); ``param_groups[*]['num_updates']`` is checkpoint-visible.
    AdamCosineWithWarmup (:142-209) likewise.

Beyond the reference: Lamb and its two scheduled forms - Adam's moments with a per-tensor trust ratio, on the same arenas and
state, three launches per step (m3p_lamb_update / _norms / _apply; the rule is written out in include/m3p_hip.h).  And the
opt-in non-finite guard (`Adam.guard_nonfinite`, `reconcile`, `roll_back`): a step whose global gradient norm is NaN or
infinite is skipped on the device, counted there, and taken back out of the host's counts at the next reconcile.  And the
opt-in exponential moving average of the weights (`Adam.enable_ema`, `ema_weights`, `ema_state`): one more fp32 arena,
one streaming launch per arena at the end of a step, and a swap of master and bf16 copy for evaluation.
"""
import contextlib
import inspect
import math
import re
from logging import getLogger

import torch
from torch import optim

import os

from . import ops

logger = getLogger()

# developer switch for A/B runs: 0 = the fused Adam pass zeroes the vocabulary gradient like every other range (round 4)
_LAZY_VOCAB_ZERO = os.environ.get('M3P_LAZY_VOCAB_ZERO', '1') != '0'


def roll_back(log, flags, steps, num_updates):
    """The host side of the non-finite guard as pure arithmetic.  log: the attempts since the last reconcile, oldest first,
    each (attempt index, [(parameter key, the step count the attempt gave it)], [group key]); flags: attempt index -> the
    device's verdict (1 = skipped); steps: parameter key -> current step count; num_updates: group key -> current count.
    -> (steps, num_updates) as they would stand had the skipped attempts never been made: every skipped attempt takes one off
    the step count of the parameters it bumped and one off the update count of its groups (new dicts; the arguments are
    left alone).  Counts only ever moved by +1 per attempt, so the order of the attempts does not matter to the result."""
    steps, num_updates = dict(steps), dict(num_updates)
    for index, bumped, groups in log:
        if not flags[index]:
            continue
        for key, _new in bumped:
            steps[key] -= 1
        for g in groups:
            num_updates[g] -= 1
    bad = [k for k, v in list(steps.items()) + list(num_updates.items()) if v < 0]
    if bad:
        raise AssertionError('roll_back: more skipped attempts than counted ones for %s' % bad[:3])
    return steps, num_updates


class Adam(optim.Optimizer):
    # Opt-in non-finite guard (Lamb and the scheduled classes inherit it): a step whose global gradient norm is NaN or
    # +-inf leaves master, moments and the bf16 copy as they were and zeroes the gradients - decided, counted and logged on
    # the device (ops.step_guard + the _guarded launches), with no host read in step().  The host cannot know the verdict,
    # so state[p]['step'], num_updates and the lr move with every attempt; reconcile() - the one host read - takes the
    # skipped attempts back out.  Until then bias corrections and schedule run one attempt ahead per unreconciled skip.
    guard_nonfinite = False
    # Opt-in exponential moving average of the weights (`enable_ema`; Lamb and the scheduled classes inherit it): None = off,
    # and then step() does nothing but test this attribute.  Else the schedule and its counters (see enable_ema).
    _ema = None

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        if not 0.0 <= lr:
            raise ValueError('Invalid learning rate: {}'.format(lr))
        if not 0.0 <= eps:
            raise ValueError('Invalid epsilon value: {}'.format(eps))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError('Invalid beta parameter at index 0: {}'.format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError('Invalid beta parameter at index 1: {}'.format(betas[1]))
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self._arenas = {}        # id(arena) -> dict(arena, m, v)
        self._pending_clip = None
        self.grad_scale = 1.0    # 1/world_size under data parallelism (gradient averaging)
        self._guard = None       # ops.StepGuard, made by the first guarded step
        self._skip = None        # the guard's device word while a guarded step() launches, else None
        self._attempts = 0       # guarded step() calls so far = the next attempt index
        self._guard_log = []     # unreconciled attempts: (index, [(parameter, new step)], [group])
        for group in self.param_groups:
            for p in group['params']:
                state = self.state[p]
                state['step'] = 0
                tag = getattr(p, '_m3p_arena', None)
                if tag is not None:
                    arena, name = tag
                    ent = self._arenas.get(id(arena))
                    if ent is None:
                        ent = dict(arena=arena, m=torch.zeros_like(arena.master), v=torch.zeros_like(arena.master),
                                   gnorm=torch.zeros(1, dtype=torch.float64, device=arena.device))
                        self._arenas[id(arena)] = ent
                    o, cnt, shape = arena.offsets[name]
                    state['exp_avg'] = ent['m'][o:o + cnt].view(shape)
                    state['exp_avg_sq'] = ent['v'][o:o + cnt].view(shape)
                else:
                    state['exp_avg'] = torch.zeros_like(p.data)
                    state['exp_avg_sq'] = torch.zeros_like(p.data)

    # ------------------------------------------------------------------ helpers
    def _active_ranges(self, arena):
        """Contiguous arena ranges of the parameters touched by backward since the last
        zero_grad, split where the per-parameter step counts differ."""
        by_param = {}
        for group in self.param_groups:
            for p in group['params']:
                tag = getattr(p, '_m3p_arena', None)
                if tag is not None and tag[0] is arena:
                    by_param[tag[1]] = (p, group)
        ranges = []
        cur = None
        for name in arena.names:
            if name not in by_param or name not in arena.touched:
                cur = None
                continue
            p, group = by_param[name]
            o, cnt, _ = arena.offsets[name]
            end = o + (cnt + 63) // 64 * 64
            step = self.state[p]['step']
            # (the arena pads to 512 elements in front of a gradient bucket: a gap between two consecutive touched
            #  parameters is that padding - zeros in every arena, a no-op for Adam - and does not split the range)
            if cur is not None and cur['next'] == name and cur['step'] == step and cur['group'] is group:
                cur['end'] = end
                cur['params'].append(p)
            else:
                cur = dict(start=o, end=end, step=step, group=group, params=[p])
                ranges.append(cur)
            cur['next'] = self._next_name(arena, name)
        return ranges

    @staticmethod
    def _next_name(arena, name):
        order = getattr(arena, '_name_after', None)
        if order is None:
            order = arena._name_after = dict(zip(arena.names, arena.names[1:] + [None]))
        return order[name]

    @staticmethod
    def _hook(arena):
        return getattr(arena.model, 'ddp_hook', None)

    def _owned(self, arena, start, end):
        """[start, end) restricted to what this rank steps: all of it, or - under the sharded data-parallel exchange
        (distributed.py, zero1) - its intersections with this rank's bucket shards."""
        hook = self._hook(arena)
        return hook.owned(start, end) if hook is not None else [(start, end)]

    def clip_grad_norm(self, max_norm):
        """clip_grad_norm_(parameters, max_norm) of xtrainer.py:225, deferred: the global
        sum of squares is reduced on the device now, the scaling is applied inside the Adam
        kernel (no host sync, no extra pass over the gradients)."""
        self._reduce_norm()
        self._pending_clip = float(max_norm)

    def _reduce_norm(self):
        """ent['gnorm'] of every arena = the global sum of squares of its active gradients (all ranks' shards)."""
        for ent in self._arenas.values():
            arena = ent['arena']
            if arena.model.ddp_hook is not None:
                arena.model.ddp_hook.finish()
            ent['gnorm'].zero_()
            pieces = []
            for r in self._active_ranges(arena):
                pieces.extend(self._owned(arena, r['start'], r['end']))
            ops.sumsq_ranges(arena.grad, pieces, ent['gnorm'])      # (one launch however many shards this rank owns)
            if arena.model.ddp_hook is not None:
                arena.model.ddp_hook.all_reduce_scalar(ent['gnorm'])     # sharded gradients: the norm is the sum over ranks

    def grad_norm(self):
        """Host value of the last reduced global norm (synchronises; for logging/tests)."""
        tot = sum(float(ent['gnorm'].item()) for ent in self._arenas.values())
        return math.sqrt(tot) * self.grad_scale

    def zero_grad(self, set_to_none=True):
        for ent in self._arenas.values():
            ent['arena'].zero_grad()
        for group in self.param_groups:
            for p in group['params']:
                if getattr(p, '_m3p_arena', None) is None:
                    p.grad = None

    # ------------------------------------------------------------------ step
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        if self._ema is not None and self._ema['inside']:
            raise RuntimeError('step() inside ema_weights(): the parameters hold the averaged weights - leave the context first')
        if self.guard_nonfinite:
            self._open_guarded_step()
        max_norm = self._pending_clip or 0.0
        self._pending_clip = None
        bumped = []
        for ent in self._arenas.values():
            arena = ent['arena']
            if arena.model.ddp_hook is not None:
                arena.model.ddp_hook.finish()
            active = self._active_ranges(arena)
            # this step's MLM head stored its weight gradient over the tied vocabulary matrix (it will again next step): that
            # range is not zeroed here - Arena.defer_vocab_zero, functional.py.  The range may span several active ranges
            # (per-parameter step counts differ after a step without an MLM head): every piece is cut at its borders.
            # Under data parallelism too (round 6: the wrapped step paid 0.3 ms for these zeros, profiles/r06_dp_overhead.txt):
            # the bucket collectives work on the arena in place after the store, the exchanged token rows enter through
            # Arena.g() (which zeroes a still-stale range first), and a sharded rank leaves its foreign shards of the range
            # un-zeroed as well (after_sharded_step(keep=...)) - the store covers them.
            lazy = None
            if getattr(arena, 'vocab_stored', False) and _LAZY_VOCAB_ZERO:
                v0, vc = arena.vocab_range()
                covered = sum(max(0, min(r['end'], v0 + vc) - max(r['start'], v0)) for r in active)
                if covered == vc:
                    lazy = (v0, v0 + vc)
                    arena.defer_vocab_zero()
            bump = self._launch_arena(arena, ent, active, lazy, max_norm)
            for p, step in bump:
                self.state[p]['step'] = step
            bumped.extend(bump)
            # sharded exchange: the other ranks' shards of the updated master come back through an all-gather that the
            # next forward waits for bucket by bucket (distributed.DataParallel.after_sharded_step)
            hook = arena.model.ddp_hook
            gathered = hook is not None and hook.after_sharded_step([(r['start'], r['end']) for r in active], keep=lazy)
            # untouched ranges may still hold stale values only if someone wrote them by hand
            arena.after_fused_step(copies_scheduled=gathered)
        self._step_loose(max_norm)
        if self._ema is not None:
            self._ema_step()
        if self._skip is not None:
            self._guard_log.append((self._attempts, bumped, [g for g in self.param_groups if 'num_updates' in g]))
            self._attempts += 1
            self._skip = None
        return loss

    # ------------------------------------------------------------------ exponential moving average of the weights
    def enable_ema(self, decay, every=1, start=0):
        """Keep ema = decay * ema + (1 - decay) * p of every parameter, updated at the end of the step() calls with index
        start, start + every, start + 2 * every, ... (calls are counted from this call on, skipped attempts of the non-finite
        guard included: the host does not know the verdict).  The update is `ema += w * (p - ema)` with w = fp32(1 - decay) in
        fp32 (include/m3p_hip.h, m3p_ema_update: product and sum fused on the arenas, each rounded for a parameter outside
        one); the first one, at `start`, is a copy.  Until then
        the EMA holds the weights as they are now.

        Costs 4 bytes per parameter: one more fp32 arena (`ent['ema']`) beside master, gradient and the two moments, and a
        clone of every parameter outside an arena.  state[p]['ema'] is a view of it, as exp_avg is of the moment arena.  The
        WHOLE arena is averaged in one launch per arena, not the active ranges: a parameter that sat out a step still decays
        towards its value.  Under the sharded data-parallel exchange a rank averages its own shards; `materialize_ema`
        gathers.  With the guard on, the launch takes the guard's device word: a skipped step leaves the EMA's bits alone."""
        decay, every, start = float(decay), int(every), int(start)
        if not 0.0 < decay < 1.0:
            raise ValueError('Invalid EMA decay: {} (0 < decay < 1)'.format(decay))
        if every < 1 or start < 0:
            raise ValueError('Invalid EMA schedule: every = {} (>= 1), start = {} (>= 0)'.format(every, start))
        if self._ema is not None:
            raise RuntimeError('enable_ema: already enabled')
        w = torch.tensor(1.0 - decay, dtype=torch.float64).to(torch.float32).item()      # exactly the fp32 the kernel is given
        for ent in self._arenas.values():
            ent['ema'] = ent['arena'].master.clone()
            # sharded exchange: are the other ranks' shards of the EMA out of date?  (Now: exactly where the master's are.)
            ent['ema_partial'] = bool(getattr(self._hook(ent['arena']), 'master_partial', False))
        for group in self.param_groups:
            for p in group['params']:
                tag = getattr(p, '_m3p_arena', None)
                if tag is not None:
                    arena, name = tag
                    o, cnt, shape = arena.offsets[name]
                    self.state[p]['ema'] = self._arenas[id(arena)]['ema'][o:o + cnt].view(shape)
                else:
                    self.state[p]['ema'] = p.data.clone()
        self._ema = dict(decay=decay, w=w, every=every, start=start, calls=0, inside=False)

    def _ema_step(self):
        """The end of step(): this call's EMA update, if the schedule names it.  One launch per arena over what this rank
        owns of [0, total); the plain torch form of the same rule for the parameters outside an arena."""
        st = self._ema
        index = st['calls']
        st['calls'] = index + 1
        if index < st['start'] or (index - st['start']) % st['every'] != 0:
            return
        first = index == st['start']
        for ent in self._arenas.values():
            arena = ent['arena']
            pieces = self._owned(arena, 0, arena.total)
            if first:
                # (a copy, not a launch with w = 1: e + (p - e) is not p in fp32.  A skipped first step copies the master it
                #  left alone)
                for a, b in pieces:
                    ent['ema'][a:b].copy_(arena.master[a:b])
            else:
                ops.ema_update(arena.master, ent['ema'], pieces, st['w'], skip=self._skip)
            hook = self._hook(arena)
            ent['ema_partial'] = hook is not None and getattr(hook, 'mode', None) == 'zero1'
        for group in self.param_groups:
            for p in group['params']:
                if getattr(p, '_m3p_arena', None) is not None:
                    continue
                e = self._ema_of(p)
                if first:
                    e.copy_(p.data)
                else:
                    e.add_((p.data - e).mul_(st['w']))

    def materialize_ema(self):
        """Collective under the sharded data-parallel exchange (every rank): gather the EMA's shards so that every rank holds
        all of it.  Nothing to do in the replicated modes, or when no update ran since the last gather."""
        if self._ema is None:
            raise RuntimeError('materialize_ema: call enable_ema first')
        for ent in self._arenas.values():
            hook = self._hook(ent['arena'])
            if hook is not None and ent['ema_partial']:
                hook.materialize_ema(ent['ema'])
            ent['ema_partial'] = False

    def _ema_swap(self):
        """Weights <-> EMA, everywhere they live: fp32 master and bf16 working copy in one pass (ops.ema_swap), the transposed
        copies marked stale and the arena's epoch moved (8-bit weight copies and vocab_mean() key on it), parameters outside an
        arena through copy_ (their _version moves: decoder.ArenaCrossWeights re-makes its copies)."""
        self.materialize_ema()
        for ent in self._arenas.values():
            arena = ent['arena']
            hook = self._hook(arena)
            if hook is not None:
                hook.materialize_master()
                hook.params_ready(None)
            ops.ema_swap(arena.master, ent['ema'], arena.w16, [(0, arena.total)])
            arena.mark_updated_by_fused_optimizer()       # master and w16 written together: only the transposes are stale
        for group in self.param_groups:
            for p in group['params']:
                if getattr(p, '_m3p_arena', None) is None:
                    e = self._ema_of(p)
                    raw = p.data.clone()
                    with torch.no_grad():
                        p.copy_(e)           # (on the parameter itself, not on .data: p._version moves)
                    e.copy_(raw)

    @contextlib.contextmanager
    def ema_weights(self):
        """Context manager (a collective under data parallelism: every rank enters and leaves): inside it the model computes
        with the averaged weights - master, bf16 copy, transposes and everything keyed on Arena.epoch - and state[p]['ema']
        holds the raw ones; leaving swaps back, to the bit.  Evaluate and save inside it; do not train: step() raises, and
        entering with gradients pending (a backward without its step) is refused."""
        st = self._ema
        if st is None:
            raise RuntimeError('ema_weights: call enable_ema first')
        if st['inside']:
            raise RuntimeError('ema_weights does not nest')
        for ent in self._arenas.values():
            if ent['arena'].touched:
                raise RuntimeError('ema_weights: gradients are pending (%d parameters touched since the last step or zero_grad): '
                                   'step or zero_grad first' % len(ent['arena'].touched))
        self._ema_swap()
        st['inside'] = True
        try:
            yield self
        finally:
            st['inside'] = False
            self._ema_swap()

    def _ema_of(self, p):
        """The EMA of a parameter of this optimizer, else None: the view of the EMA arena (made afresh - whoever detached
        state[p]['ema'] for a checkpoint did not detach this), or the clone kept for a parameter outside an arena."""
        tag = getattr(p, '_m3p_arena', None)
        if tag is not None:
            ent = self._arenas.get(id(tag[0]))
            if ent is None or 'ema' not in ent or p not in self.state:
                return None
            o, cnt, shape = tag[0].offsets[tag[1]]
            return ent['ema'][o:o + cnt].view(shape)
        return self.state[p].get('ema') if p in self.state else None

    def _ema_named(self, named):
        if named is not None:
            return list(named)
        out = []
        for gi, group in enumerate(self.param_groups):
            for pi, p in enumerate(group['params']):
                tag = getattr(p, '_m3p_arena', None)
                out.append((tag[1] if tag is not None else 'group%d.%d' % (gi, pi), p))
        return out

    def ema_state(self, named=None):
        """{name: fp32 CPU tensor} of the materialised EMA, for checkpoints (a collective under the sharded exchange).
        named: (name, tensor) pairs that give the keys - e.g. ``model.state_dict(keep_vars=True).items()``, which makes the
        result load into a model; entries that are not parameters of this optimizer are copied as they are.  Default: the
        arena's names, and 'group<g>.<i>' for a parameter outside an arena."""
        if self._ema is None:
            raise RuntimeError('ema_state: call enable_ema first')
        if self._ema['inside']:
            raise RuntimeError('ema_state inside ema_weights(): the buffers are exchanged')
        self.materialize_ema()
        out = {}
        for name, t in self._ema_named(named):
            e = self._ema_of(t)
            out[name] = (t if e is None else e).detach().float().cpu().clone()
        return out

    def load_ema_state(self, d, named=None, warn=True):
        """Write an `ema_state` back (names as there).  A parameter whose name is missing starts its EMA at its current
        weights; one warning names how many.  A collective under the sharded exchange."""
        if self._ema is None:
            raise RuntimeError('load_ema_state: call enable_ema first')
        if self._ema['inside']:
            raise RuntimeError('load_ema_state inside ema_weights(): the buffers are exchanged')
        for ent in self._arenas.values():
            hook = self._hook(ent['arena'])
            if hook is not None:
                hook.materialize_master()        # (a missing name copies the master: all of it must be current here)
                hook.params_ready(None)
        missing, seen = [], set()
        for name, t in self._ema_named(named):
            e = self._ema_of(t)
            if e is None or id(t) in seen:
                continue
            if name in d:
                seen.add(id(t))
                e.copy_(d[name].to(e.device, torch.float32).view_as(e))
            else:
                missing.append((name, t))
        missing = [(name, t) for name, t in missing if id(t) not in seen]
        for name, t in missing:
            self._ema_of(t).copy_(t.data)
        if missing and warn:
            logger.warning('load_ema_state: %d parameters are not in the saved EMA and start from their current weights (%s ...)'
                           % (len(missing), missing[0][0]))
        for ent in self._arenas.values():
            ent['ema_partial'] = False

    # ------------------------------------------------------------------ non-finite guard
    def _open_guarded_step(self):
        """In front of a guarded step's launches: the reduced norm (clip_grad_norm's, or reduced here by the same launch and
        the same all-reduce - without clipping), then the one-thread decision every launch of this step reads."""
        if not self._arenas or any(getattr(p, '_m3p_arena', None) is None and p.grad is not None
                                   for group in self.param_groups for p in group['params']):
            raise RuntimeError('guard_nonfinite covers the fused arena path only: this optimizer holds parameters outside an arena')
        if len(self._guard_log) >= ops.StepGuard.RING:         # the ring is full: this attempt would overwrite an unread verdict
            self.reconcile()
        if self._pending_clip is None:
            self._reduce_norm()
        if self._guard is None:
            self._guard = ops.StepGuard(next(iter(self._arenas.values()))['arena'].device)
        ops.step_guard([ent['gnorm'] for ent in self._arenas.values()], self.grad_scale, self._attempts, self._guard)
        self._skip = self._guard.skip

    def reconcile(self):
        """The guard's ONE host read (it synchronises): ring, norms and counters.  Every logged attempt the device skipped is
        taken back out of state[p]['step'], of num_updates and of the lr (`roll_back`), and the log is cleared; after it
        master, moments, bf16 copy, step counts, num_updates and lr are what they would be had the skipped batches not existed.
        -> dict(attempts, skipped_total, skipped_in_a_row, norms=[the finite global norms since the last call])."""
        if self._guard is None:
            return dict(attempts=0, skipped_total=0, skipped_in_a_row=0, norms=[])
        counters, norm_ring, ring = self._guard.read()
        flags = {index: ring[index % ops.StepGuard.RING] for index, _, _ in self._guard_log}
        norms = [norm_ring[index % ops.StepGuard.RING] for index, _, _ in self._guard_log if not flags[index]]
        log = [(index, [(id(p), step) for p, step in bumped], [id(g) for g in groups]) for index, bumped, groups in self._guard_log]
        params = {id(p): p for _, bumped, _ in self._guard_log for p, _ in bumped}
        groups = {id(g): g for _, _, gs in self._guard_log for g in gs}
        steps, updates = roll_back(log, flags, {k: self.state[p]['step'] for k, p in params.items()},
                                   {k: g['num_updates'] for k, g in groups.items()})
        for k, p in params.items():
            self.state[p]['step'] = steps[k]
        for k, g in groups.items():
            if g['num_updates'] != updates[k]:
                g['num_updates'] = updates[k]
                g['lr'] = self._lr_at(updates[k])
        del self._guard_log[:]
        return dict(attempts=counters[0], skipped_total=counters[1], skipped_in_a_row=counters[2], norms=norms)

    def state_dict(self):
        if self._guard_log:             # checkpoints carry exact counts
            self.reconcile()
        return super().state_dict()

    def _launch_arena(self, arena, ent, active, lazy, max_norm):
        """The update of one arena's active ranges (lazy = the [start, end) this step leaves un-zeroed, or None).
        -> [(parameter, new step count)], which step() applies only once every launch has been accepted."""
        # every piece of every active range of a parameter group goes into ONE launch (ops.adam_step_ranges): a sharded rank
        # steps fifteen bucket shards, and fifteen launches streamed the same bytes 24 % slower than one
        batches = {}
        bump = []          # (parameter, new step count): applied only once every launch below has been accepted
        for r in active:
            group = r['group']
            beta1, beta2 = group['betas']
            step = r['step'] + 1
            bc1 = 1 - beta1 ** step
            bc2 = 1 - beta2 ** step
            step_size = group['lr'] * math.sqrt(bc2) / bc1
            pieces = batches.setdefault(id(group), (group, []))[1]
            for s, e in self._owned(arena, r['start'], r['end']):
                pieces.extend((a, b, step_size, z) for a, b, z in self._cut_lazy(s, e, lazy))
            bump.extend((p, step) for p in r['params'])
        for group, pieces in batches.values():
            # (the kernel takes pieces whose borders are multiples of four elements: a bad one is refused HERE, before any
            #  launch of this step has changed a parameter or a step counter)
            bad = [(a, b) for a, b, _, _ in pieces if (a | b) & 3]
            if bad:
                raise ValueError('fused Adam: piece borders must be multiples of 4 elements, got %s' % bad[:3])
        for group, pieces in batches.values():
            beta1, beta2 = group['betas']
            ops.adam_step_ranges(arena.master, arena.grad, ent['m'], ent['v'], arena.w16, pieces, group['lr'], beta1, beta2,
                                 group['eps'], group['weight_decay'], gnorm_sq=ent['gnorm'] if max_norm > 0 else None,
                                 max_norm=max_norm, grad_scale=self.grad_scale, skip=self._skip)
        return bump

    @staticmethod
    def _cut_lazy(s, e, lazy):
        """[s, e) cut at the borders of the lazily zeroed range -> [(start, end, zero_grad)]: the parts inside it are not zeroed."""
        if lazy is None or e <= lazy[0] or s >= lazy[1]:
            return [(s, e, True)]
        cuts = sorted({s, e, min(max(lazy[0], s), e), min(max(lazy[1], s), e)})
        return [(a, b, not (lazy[0] <= a and b <= lazy[1])) for a, b in zip(cuts, cuts[1:]) if b > a]

    def _step_loose(self, max_norm):
        # parameters outside any arena (never the case on the hot path) — reference loop
        for group in self.param_groups:
            for p in group['params']:
                if getattr(p, '_m3p_arena', None) is not None or p.grad is None:
                    continue
                grad = p.grad.data
                state = self.state[p]
                beta1, beta2 = group['betas']
                state['step'] += 1
                state['exp_avg'].mul_(beta1).add_(grad, alpha=1 - beta1)
                state['exp_avg_sq'].mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
                denom = state['exp_avg_sq'].sqrt().add_(group['eps'])
                bc1 = 1 - beta1 ** state['step']
                bc2 = 1 - beta2 ** state['step']
                step_size = group['lr'] * math.sqrt(bc2) / bc1
                if group['weight_decay'] != 0:
                    p.data.add_(p.data, alpha=-group['weight_decay'] * group['lr'])
                p.data.addcdiv_(state['exp_avg'], denom, value=-step_size)


def inverse_sqrt_schedule(peak_lr, warmup, floor_lr, power):
    """lr(t) of optim.py:116-133 as one closed form: a straight line from `floor_lr` (t = 0) to `peak_lr` (t = warmup),
    then peak_lr * (warmup / t) ** power.  Returned as a function of the update count."""
    def lr_at(t):
        if t < warmup:
            return floor_lr + (peak_lr - floor_lr) * t / warmup
        return peak_lr * (warmup / t) ** power
    return lr_at


def cosine_schedule(peak_lr, warmup, floor_lr, min_lr, period, period_mult, lr_shrink):
    """lr(t) of optim.py:186-202: the warm-up line from `floor_lr` to `peak_lr`, then cosine periods (arXiv 1608.03983) from
    the peak down to `min_lr`; period i is `period * period_mult ** i` updates long and both ends shrink by `lr_shrink ** i`.
    Stated like `inverse_sqrt_schedule`, as a function of the update count: the periods are walked from the first one on
    (equal periods are skipped in one division; growing ones are few - their lengths add up geometrically), so a period
    border is decided by the integer arithmetic of the counts and not by a rounded logarithm."""
    if period <= 0 or period_mult < 1:
        raise ValueError('cosine schedule: init_period must be positive and period_mult >= 1 (periods that shrink add up to a '
                         'finite number of updates), got %r, %r' % (period, period_mult))

    def lr_at(t):
        if t < warmup:
            return floor_lr + (peak_lr - floor_lr) * t / warmup
        into, length, done = t - warmup, period, 0       # updates into the current period, its length, periods completed
        if period_mult == 1:
            done, into = divmod(into, length)
        else:
            while into >= length:
                into, length, done = into - length, length * period_mult, done + 1
        scale = lr_shrink ** done
        descent = (1 + math.cos(math.pi * into / length)) / 2      # 1 at the start of a period, 0 at its end
        return scale * (min_lr + (peak_lr - min_lr) * descent)
    return lr_at


class _Scheduled:
    """The schedule, apart from the update rule: mixed in FRONT of an optimizer class whose constructor was given the floor
    rate.  Every `step()` counts one update per parameter group (`num_updates`, which checkpoints carry) and moves the
    group's lr along `self._lr_at`; `get_lr_for_step` is what Trainer.reload_checkpoint asks after restoring the count."""

    def _start_schedule(self, make, **schedule):
        self.schedule = schedule
        self._lr_at = make(**schedule)
        for group in self.param_groups:
            group['num_updates'] = 0

    def get_lr_for_step(self, num_updates):
        return self._lr_at(num_updates)

    def step(self, closure=None):
        out = super().step(closure)
        for group in self.param_groups:
            group['num_updates'] += 1
            group['lr'] = self._lr_at(group['num_updates'])
        return out


class AdamInverseSqrtWithWarmup(_Scheduled, Adam):
    """Adam whose lr follows `inverse_sqrt_schedule` (optim.py:89-139): built at the floor rate, every `step()` counts
    one update per parameter group (`num_updates`, which checkpoints carry) and moves the group's lr along the curve."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, warmup_updates=4000,
                 warmup_init_lr=1e-7, exp_factor=0.5):
        super().__init__(params, lr=warmup_init_lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self._start_schedule(inverse_sqrt_schedule, peak_lr=lr, warmup=warmup_updates, floor_lr=warmup_init_lr, power=exp_factor)


class AdamCosineWithWarmup(_Scheduled, Adam):
    """Adam whose lr follows `cosine_schedule` (optim.py:142-209), constructor arguments as there."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, warmup_updates=4000,
                 warmup_init_lr=1e-7, min_lr=1e-9, init_period=1000000, period_mult=1, lr_shrink=0.75):
        super().__init__(params, lr=warmup_init_lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self._start_schedule(cosine_schedule, peak_lr=lr, warmup=warmup_updates, floor_lr=warmup_init_lr, min_lr=min_lr,
                             period=init_period, period_mult=period_mult, lr_shrink=lr_shrink)


class Lamb(Adam):
    """LAMB (arXiv 1904.00962) on the fused arena path: Adam's moments and a per-tensor trust ratio ||p|| / ||r|| on the
    update r = m_hat / (sqrt(v_hat) + eps) + wd p - the rule is written out in include/m3p_hip.h.  Everything around the
    launch is Adam's: the touched rule, the deferred clip, the lazily zeroed vocabulary range, the shards of the sharded
    exchange, the state keys (`step`, `exp_avg`, `exp_avg_sq`: the same views of the moment arenas, so checkpoints are
    interchangeable).  exclude_1d: tensors with fewer than two dimensions (biases, LayerNorm weights, the ITM score vector)
    neither decay nor adapt - the BERT convention."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, exclude_1d=True):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self.exclude_1d = bool(exclude_1d)
        self._tables = {}        # (id(arena), id(group)) -> {pieces: ops.LambTable}: one per set of active pieces (step type)

    def _tensor_rule(self, p, group):
        """(wd_t, adapt_t) of a parameter."""
        plain = self.exclude_1d and p.dim() < 2
        return (0.0 if plain else group['weight_decay']), not plain

    def _table(self, arena, group, pieces, n_tensors, n_classes):
        cache = self._tables.setdefault((id(arena), id(group)), {})
        key = (tuple(pieces), n_tensors, n_classes)
        table = cache.get(key)
        if table is None:
            if len(cache) >= 64:         # (a training run alternates between a handful of step types)
                cache.clear()
            table = cache[key] = ops.LambTable(pieces, n_tensors, n_classes, arena.total, device=arena.device)
        return table

    def _launch_arena(self, arena, ent, active, lazy, max_norm):
        chunks = {}           # id(group) -> [chunk]: the tensors of a group in arena order, cut where a launch's classes are full
        bump = []
        for r in active:
            group = r['group']
            beta1, beta2 = group['betas']
            step = r['step'] + 1
            run = chunks.setdefault(id(group), [])
            for p in r['params']:
                o, cnt, _ = arena.offsets[p._m3p_arena[1]]
                end = o + (cnt + 63) // 64 * 64          # (the zero padding behind a tensor adds nothing to either norm)
                wd_t, adapt_t = self._tensor_rule(p, group)
                # class = the scalars tensors may differ in; numbered in order of appearance, so that the same step type
                # finds its cached table again although the step counts have moved on.  A launch carries LAMB_MAX_CLASSES of
                # them by value: a group whose tensors hold more distinct (step count, wd_t, adapt_t) than that - more than
                # ~16 heads that have sat out different numbers of steps - goes on in another table and three more launches.
                # (Every rank cuts alike: the cut depends on the tensors and their step counts only.)
                key = (step, wd_t, adapt_t)
                if not run or (key not in run[-1]['class_ids'] and len(run[-1]['classes']) == ops.LAMB_MAX_CLASSES):
                    run.append(dict(group=group, pieces=[], class_ids={}, classes=[], n_tensors=0))
                b = run[-1]
                cls = b['class_ids'].setdefault(key, len(b['classes']))
                if cls == len(b['classes']):
                    b['classes'].append((1.0 / (1 - beta1 ** step), 1.0 / (1 - beta2 ** step), wd_t, adapt_t))
                tid = b['n_tensors']                       # every rank numbers the tensors alike, whatever it owns of them
                b['n_tensors'] += 1
                for s, e in self._owned(arena, o, end):
                    b['pieces'].extend((a, c, tid, z, cls) for a, c, z in self._cut_lazy(s, e, lazy))
            bump.extend((p, step) for p in r['params'])
        batches = [b for run in chunks.values() for b in run]
        # (tables are validated when they are built: a piece the kernels cannot take is refused HERE, before any launch of
        #  this step has changed a parameter or a step counter)
        for b in batches:
            b['table'] = self._table(arena, b['group'], b['pieces'], b['n_tensors'], len(b['classes'])) if b['pieces'] else None
        hook = self._hook(arena)
        for b in batches:
            group, table, classes = b['group'], b['table'], b['classes']
            beta1, beta2 = group['betas']
            if table is None:
                # a sharded rank that owns nothing of this group still takes part in the sum of the norms
                if hook is not None:
                    hook.all_reduce_scalar(torch.zeros((b['n_tensors'], 2), dtype=torch.float64, device=arena.device))
                continue
            ops.lamb_update(arena.master, arena.grad, ent['m'], ent['v'], table, classes, beta1, beta2, group['eps'],
                            gnorm_sq=ent['gnorm'] if max_norm > 0 else None, max_norm=max_norm, grad_scale=self.grad_scale,
                            skip=self._skip)
            ops.lamb_norms(table, skip=self._skip)
            if hook is not None:
                hook.all_reduce_scalar(table.norms)      # sharded exchange: a tensor's norms are the sums over the ranks' shards
            ops.lamb_apply(arena.master, arena.grad, arena.w16, table, classes, group['lr'], skip=self._skip)
        return bump

    def _step_loose(self, max_norm):
        # parameters outside any arena (CPU models): the same rule as a plain torch loop
        loose = [(group, p) for group in self.param_groups for p in group['params']
                 if getattr(p, '_m3p_arena', None) is None and p.grad is not None]
        if not loose:
            return
        coef = self.grad_scale
        if max_norm > 0:
            norm = math.sqrt(sum(float(p.grad.data.double().pow(2).sum()) for _, p in loose)) * self.grad_scale
            coef *= min(1.0, max_norm / (norm + 1e-6))
        for group, p in loose:
            grad = p.grad.data * coef
            state = self.state[p]
            beta1, beta2 = group['betas']
            wd_t, adapt_t = self._tensor_rule(p, group)
            state['step'] += 1
            state['exp_avg'].mul_(beta1).add_(grad, alpha=1 - beta1)
            state['exp_avg_sq'].mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
            bc1 = 1 - beta1 ** state['step']
            bc2 = 1 - beta2 ** state['step']
            r = (state['exp_avg'] / bc1) / ((state['exp_avg_sq'] / bc2).sqrt() + group['eps'])
            if wd_t != 0:
                r = r.add(p.data, alpha=wd_t)
            phi = 1.0
            if adapt_t:
                pn, rn = float(p.data.double().norm()), float(r.double().norm())
                if pn > 0 and rn > 0:
                    phi = pn / rn
            p.data.add_(r, alpha=-group['lr'] * phi)


class LambInverseSqrtWithWarmup(_Scheduled, Lamb):
    """Lamb whose lr follows `inverse_sqrt_schedule`, arguments as AdamInverseSqrtWithWarmup's."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, exclude_1d=True, warmup_updates=4000,
                 warmup_init_lr=1e-7, exp_factor=0.5):
        super().__init__(params, lr=warmup_init_lr, betas=betas, eps=eps, weight_decay=weight_decay, exclude_1d=exclude_1d)
        self._start_schedule(inverse_sqrt_schedule, peak_lr=lr, warmup=warmup_updates, floor_lr=warmup_init_lr, power=exp_factor)


class LambCosineWithWarmup(_Scheduled, Lamb):
    """Lamb whose lr follows `cosine_schedule`, arguments as AdamCosineWithWarmup's."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, exclude_1d=True, warmup_updates=4000,
                 warmup_init_lr=1e-7, min_lr=1e-9, init_period=1000000, period_mult=1, lr_shrink=0.75):
        super().__init__(params, lr=warmup_init_lr, betas=betas, eps=eps, weight_decay=weight_decay, exclude_1d=exclude_1d)
        self._start_schedule(cosine_schedule, peak_lr=lr, warmup=warmup_updates, floor_lr=warmup_init_lr, min_lr=min_lr,
                             period=init_period, period_mult=period_mult, lr_shrink=lr_shrink)


def clip_grad_norm_(parameters, max_norm, optimizer):
    """Fused stand-in for torch.nn.utils.clip_grad_norm_ at xtrainer.py:225/237 (see
    Adam.clip_grad_norm)."""
    optimizer.clip_grad_norm(max_norm)


# optimizer spec names -> (class, whether the "beta1=..,beta2=.." pair folds into betas=(b1, b2))
_METHODS = {
    'adam': (Adam, True),
    'adam_inverse_sqrt': (AdamInverseSqrtWithWarmup, True),
    'adam_cosine': (AdamCosineWithWarmup, True),
    'lamb': (Lamb, True),
    'lamb_inverse_sqrt': (LambInverseSqrtWithWarmup, True),
    'lamb_cosine': (LambCosineWithWarmup, True),
    'adadelta': (optim.Adadelta, False),
    'adagrad': (optim.Adagrad, False),
    'adamax': (optim.Adamax, False),
    'asgd': (optim.ASGD, False),
    'rmsprop': (optim.RMSprop, False),
    'rprop': (optim.Rprop, False),
    'sgd': (optim.SGD, False),
}
_NUMBER = re.compile(r'^[+-]?(\d+(\.\d*)?|\.\d+)$')


def parse_optimizer_spec(spec):
    """'adam_inverse_sqrt,beta1=0.9,beta2=0.98,lr=0.0001' -> ('adam_inverse_sqrt', {'beta1': 0.9, ...}).
    The string format is the contract of ``--optimizer`` (optim.py:211-229): a method name followed by
    comma-separated ``key=<plain decimal>`` pairs."""
    method, *pairs = spec.split(',')
    kwargs = {}
    for pair in pairs:
        key, eq, val = pair.partition('=')
        if not eq or '=' in val or _NUMBER.match(val) is None:
            raise AssertionError('optimizer option %r is not key=<number>' % pair)
        kwargs[key] = float(val)
    return method, kwargs


def get_optimizer(parameters, s):
    """Drop-in for optim.py:211-270.  adam / adam_inverse_sqrt / adam_cosine and lamb / lamb_inverse_sqrt / lamb_cosine
    (``exclude_1d=0|1`` in the same number-only syntax) run on the fused kernels; the torch.optim names the reference also
    accepts pass through (they then see ordinary fp32 parameters).  Unknown methods and options the optimizer's
    constructor does not take raise, like the reference."""
    method, kwargs = parse_optimizer_spec(s)
    if method not in _METHODS:
        raise Exception('Unknown optimization method: "%s"' % method)
    cls, fold_betas = _METHODS[method]
    if fold_betas:
        kwargs['betas'] = (kwargs.pop('beta1', 0.9), kwargs.pop('beta2', 0.999))
    if method == 'sgd':
        assert 'lr' in kwargs
    accepted = list(inspect.signature(cls.__init__).parameters)
    assert accepted[:2] == ['self', 'params']
    unknown = [k for k in kwargs if k not in accepted[2:]]
    if unknown:
        raise Exception('Unexpected parameters: expected "%s", got "%s"' % (str(accepted[2:]), str(list(kwargs))))
    return cls(parameters, **kwargs)
