import math

import numpy as np
import pytest
import torch

from tests.util import randn_bf16, randn_f32, rel_l2, max_abs
from tests.util import (ATTN_CTX_RTOL, ATTN_DS_FLOOR, ATTN_DS_RTOL, F32_OUT, GLOBAL_ATTN_CTX, GLOBAL_ATTN_GRAD, KAPPA, ROW_FLOOR, U32,
                        assert_block_bound, assert_exact_zero, assert_gemm_bound, poison_outputs)  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu


def _ref_attention(qkv, keylen, B, S, H, dh, keep=None, p=0.0):
    """fp32 restatement of transformer.py:197-205 on an already-projected, q-prescaled qkv."""
    d = H * dh
    q, k, v = qkv.view(B, S, 3, H, dh).permute(2, 0, 3, 1, 4)      # (B,H,S,dh)
    scores = q @ k.transpose(2, 3)
    mask = torch.arange(S)[None, :] < keylen[:, None]
    scores = scores.masked_fill(~mask[:, None, None, :], float('-inf'))
    w = torch.softmax(scores, dim=-1)
    lse = torch.logsumexp(scores, dim=-1)
    if keep is not None:
        w = w * keep / (1 - p)
    ctx = (w @ v).transpose(1, 2).reshape(B * S, d)
    return ctx, lse


def _ref64(qkv, keylen, dctx, B, S, H, dh, keep=None, p=0.0):
    """fp64 attention forward and backward on the device, the reference of the per-row bounds: -> dict of ctx, dq, dk, dv
    as [B, H, S, dh] (dq = the gradient of the unscaled q projection, as the kernel returns it), lse [B, H, S] and, for the
    lse bound, the largest sum_d |q_d k_d| over the valid keys of each query."""
    q, k, v = qkv.cuda().double().view(B, S, 3, H, dh).permute(2, 0, 3, 1, 4)
    valid = torch.arange(S, device='cuda')[None, :] < keylen.cuda().long()[:, None]
    s = (q @ k.transpose(-1, -2)).masked_fill(~valid[:, None, None, :], float('-inf'))
    lse = torch.logsumexp(s, -1)
    pr = torch.exp(s - lse[..., None])
    del s
    z = 1.0 if keep is None else keep.cuda().double() / (1 - p)
    pd = pr * z
    do = dctx.cuda().double().view(B, S, H, dh).transpose(1, 2)
    dp = (do @ v.transpose(-1, -2)) * z
    ds = pr * (dp - (dp * pr).sum(-1, keepdim=True))
    del dp
    sabs = (q.abs() @ k.abs().transpose(-1, -2)).masked_fill(~valid[:, None, None, :], 0).amax(-1)
    return {'ctx': pd @ v, 'dq': ds @ k / math.sqrt(dh), 'dk': ds.transpose(-1, -2) @ q, 'dv': pd.transpose(-1, -2) @ do,
            'lse': lse, 'sabs': sabs}


def _heads(t, B, S, H, dh):
    """[B*S, H*dh] (a column slice of dqkv included) -> [B, H, S, dh]."""
    return t.reshape(B, S, H, dh).transpose(1, 2)


WORST = {}                        # kernel form and quantity -> the largest normalised error seen (1 = the bar)


def _note(form, what, worst):
    if form:
        key = '%-34s %s' % (form, what)
        WORST[key] = max(WORST.get(key, 0.0), float(worst))


def _check_rows(ref, B, S, H, dh, keylen, ctx=None, lse=None, dqkv=None, what='', skip_ds=(), form=None):
    """The per-(b, h, row) bounds of tests/util.py (bars derived there from the kernel's bf16 P and dS operands and bf16
    outputs), lse elementwise, and exact zeros in the dK / dV rows of keys >= keylen[b] (P = 0 and dS = 0 there exactly).
    lse: the scores' fp32 accumulation over dh, and __logf / exp of a sum of positive O(1) terms, 2^-20 absolute.
    skip_ds: batch entries left out of the dq / dk row bound (a single key: their reference is identically 0, see
    _check_single_key); form = (forward form, backward form) to note the worst errors under."""
    d = H * dh
    names = ('b', 'h', 'row')
    if ctx is not None:
        w = assert_block_bound(_heads(ctx, B, S, H, dh), ref['ctx'], names, ATTN_CTX_RTOL, ROW_FLOOR, what + ' ctx')
        _note(form and form[0], 'ctx / ATTN_CTX_RTOL', w / ATTN_CTX_RTOL)
    if lse is not None:
        w = assert_gemm_bound(lse.view(B * H, S), ref['lse'].view(B * H, S), ref['sabs'].view(B * H, S), dh, F32_OUT, 2.0 ** -20,
                              what + ' lse')
        _note(form and form[0], 'lse', w)
    if dqkv is None:
        return
    some = [b for b in range(B) if b not in skip_ds]
    assert all(int(keylen[b]) == 1 for b in skip_ds) and 11 * len(skip_ds) <= B      # one entry of eleven at the most
    gall = math.sqrt(sum(float(ref[n].norm()) ** 2 for n in ('dq', 'dk', 'dv')))
    for i, (name, rtol, floor) in enumerate((('dq', ATTN_DS_RTOL, ATTN_DS_FLOOR), ('dk', ATTN_DS_RTOL, ATTN_DS_FLOOR),
                                             ('dv', ATTN_CTX_RTOL, ROW_FLOOR))):
        if float(ref[name].norm()) < 1e-6 * gall:     # a single key: dq = dk = 0 exactly (the existing asserts cover it)
            continue
        got, want = _heads(dqkv[:, i * d:(i + 1) * d], B, S, H, dh), ref[name]
        if skip_ds and name != 'dv':
            got, want = got[some], want[some]
        worst = assert_block_bound(got, want, names, rtol, floor, what + ' ' + name)
        _note(form and form[1], '%s / %s' % (name, 'ATTN_CTX_RTOL' if name == 'dv' else 'ATTN_DS_RTOL'), worst / rtol)
        print('attention %s %s (B=%d S=%d H=%d): worst row %.3g of the bar %.3g' % (what, name, B, S, H, worst, rtol))
    rows = dqkv.view(B, S, 3, H, dh)
    for b in range(B):
        kl = int(keylen[b])
        if kl < S:
            assert_exact_zero(rows[b, kl:, 1:], '%s dK / dV of the keys past keylen[%d] = %d' % (what, b, kl))


# --- the launchers' rules (m3p_amd/csrc/attention.hip: launch_fwd, launch_bwd), restated -------------------------------------
ATTN_LDS_TWO_WORKGROUPS = 160 * 1024      # launch_fwd / launch_bwd: `wide` = twice the workgroup's LDS does not fit in this
ATTN_MAX_S = 512                          # m3p_attn_fwd / m3p_attn_bwd: S <= 512
FORMS_BWD = {0: 'attn_bwd_p_kernel (persistent)', 1: 'attn_bwd<6, 11> two-phase', 2: 'attn_bwd<6, 11, 12> one-pass'}


def fwd_band(S, dh, p=0.0):
    """launch_fwd: (nt, nk, the attn_fwd_kernel instantiation) for this sequence length and head width."""
    nt, nk = (S + 15) // 16, (S + 31) // 32
    wide = 2 * (nt * 16 + nk * 32) * dh * 2 > ATTN_LDS_TWO_WORKGROUPS
    kt = 6 if nk <= 6 else 12 if nk <= 12 else 16
    if wide:
        return nt, nk, 'attn_fwd<KT = %d> eight waves (wide)' % kt
    if nt == 11 and kt == 6:
        return nt, nk, 'attn_fwd<6, 11>%s' % ('' if p == 0 else ' odd S' if S & 1 else ' EVENS')
    return nt, nk, 'attn_fwd<KT = %d> %s waves' % (kt, 'eight' if kt == 16 else 'four')


def bwd_band(S, dh):
    """launch_bwd with the default variant and the keep words handed over: (nk, the backward form)."""
    nk = (S + 31) // 32
    wide = 2 * (2 * nk * 32 * dh * 2) > ATTN_LDS_TWO_WORKGROUPS
    m3p_seq = nk == 6 and (S + 15) // 16 == 11
    if m3p_seq:
        return nk, 'one-pass / persistent' if dh == 64 else 'attn_bwd<6, 11> two-phase'
    if nk == 6:
        return nk, 'attn_bwd<6, 0> unrolled'
    return nk, 'attn_bwd<0, 0> eight waves (wide)' if wide else 'attn_bwd<0, 0> four waves'


def _forms(S, dh, p):
    f, b = fwd_band(S, dh, p)[2], bwd_band(S, dh)[1]
    return '%s dh=%d' % (f, dh), '%s dh=%d' % (FORMS_BWD[0] if b == 'one-pass / persistent' else b, dh)


def _check_single_key(ref, qkv, ctx, dctx, dqkv, keep, B, S, H, dh, p, entries, what):
    """dq and dk of the batch entries with keylen = 1: P = 1 for the one key, so dS = P (dP - D) = 0 and both are identically
    zero in exact arithmetic; the RMS floor of the row bound is zero with them.  What the kernel's documented arithmetic
    leaves instead, with z = keep / (1 - p) the dropout factor of (query, key 0):
        dS_q = z_q (dO_q . V_0) - dO_q . O_q,      dq_q = dS_q K_0 / sqrt(dh),      dk_0 = sum_q dS_q Q_q,
    where O is the bf16 context the forward kernel stored (D = rowsum(dO * O)).
    - p > 0: O_q = bf16(bf16(z_q) V_0) - the dropped probability enters the P V product in bf16, 1.109375 for 1 / 0.9, and the
      product is rounded again - so dS_q is a 2^-8 residue of dO_q . V_0.  dq and dk are held to that restatement, in fp64 from
      the stored O, by the row bound of every other entry (ATTN_DS_RTOL of the head's RMS row); dq also to the bar of the
      single-position case of test_attention_fwd_bwd, |dq| < 1e-2 |dv of the entry|.  That bar does not hold for dk: the
      restatement itself reaches 1.015e-2 |dv| at (11, 356, 2, 64) (tests/test_parity_bounds.py, where the kernels' 2.28 against
      225 is reproduced to three digits), so dk is held to the restatement alone.
    - p = 0: O = V exactly, and dP_q = sum_d dO_qd V_d and D_q are the same sum of 16-bit products - but the kernel takes dP
      from the MFMA's accumulator and D from a row sum over lanes (attention.hip: "D[q] = rowsum(dO * O)"), two fp32 summation
      orders, so they are not exactly zero (|dq| ~ 3e-6, |dk| ~ 3e-5 against |dv| ~ 150).  Each sum is within KAPPA sqrt(dh)
      2^-24 sum_d |dO_qd V_d| =: e_q / 2 of the exact one (the accumulation model of gemm_bound), so |dS_q| <= e_q, and
      elementwise |dq_q| <= e_q |K_0| / sqrt(dh), |dk_0| <= sum_q e_q |Q_q|, with 2^-7 on top for the bf16 roundings of dS and
      of the outputs."""
    d = H * dh
    for b in entries:
        rows = dqkv[b * S:(b + 1) * S].double()
        dq, dk = rows[:, :d].view(S, H, dh), rows[:, d:2 * d]
        n_dv = float(ref['dv'][b].norm())
        n_dq, n_dk = float(dq.norm()), float(dk.norm())
        print('attention %s: single-key entry %d (S=%d dh=%d): |dq| = %.3g, |dk| = %.3g, |dv ref| = %.3g' % (what, b, S, dh, n_dq, n_dk, n_dv))
        assert_exact_zero(dk[1:], '%s dk past the single key of entry %d' % (what, b))
        dk0 = dk[0].view(H, dh)
        x = qkv[b * S:(b + 1) * S].double().view(S, 3, H, dh)
        q, k0, v0 = x[:, 0], x[0, 1], x[0, 2]                                    # [S, H, dh], [H, dh], [H, dh]
        do = dctx[b * S:(b + 1) * S].double().view(S, H, dh)
        if p > 0:
            z = keep[b, :, :, 0].t().cuda().double() / (1 - p)                   # [S, H]
            ds = z * (do * v0).sum(-1) - (do * ctx[b * S:(b + 1) * S].double().view(S, H, dh)).sum(-1)
            dq_ref, dk_ref = ds[..., None] * k0 / math.sqrt(dh), (ds[..., None] * q).sum(0)
            wq = assert_block_bound(dq.transpose(0, 1), dq_ref.transpose(0, 1), ('h', 'row'), ATTN_DS_RTOL, ATTN_DS_FLOOR,
                                    '%s dq of single-key entry %d against the restatement' % (what, b))
            wk = assert_block_bound(dk0[:, None], dk_ref[:, None], ('h', 'row'), ATTN_DS_RTOL, ATTN_DS_FLOOR,
                                    '%s dk of single-key entry %d against the restatement' % (what, b))
            print('    p = %g: dq within %.3g and dk within %.3g of the restatement from the stored O; |dk restated| = %.3g'
                  % (p, wq, wk, float(dk_ref.norm())))
            assert n_dq < 1e-2 * n_dv, (what, b, n_dq, n_dv)
            continue
        e = 2 * KAPPA * math.sqrt(dh) * U32 * (do.abs() * v0.abs()).sum(-1)      # [S, H]
        lim_dq = (1 + 2.0 ** -7) * e[..., None] * k0.abs() / math.sqrt(dh)
        lim_dk = (1 + 2.0 ** -7) * (e[..., None] * q.abs()).sum(0)
        over_q = float((dq.abs() / (lim_dq + 1e-300)).max())
        over_k = float((dk0.abs() / (lim_dk + 1e-300)).max())
        print('    p = 0: dq reaches %.3g and dk %.3g of the bound of two fp32 sums of dO V in different orders' % (over_q, over_k))
        assert over_q <= 1.0 and over_k <= 1.0, (what, b, over_q, over_k)


CASES = [(2, 74, 4, 32), (3, 164, 12, 64), (2, 16, 2, 64), (1, 116, 12, 64), (2, 200, 2, 64), (1, 356, 16, 64), (2, 33, 1, 32),
         (1, 512, 2, 64), (2, 1, 2, 64), (1, 500, 3, 32)]     # the maximum sequence, a single position, long with dh = 32


@pytest.mark.usefixtures('poison_outputs')
@pytest.mark.parametrize('B,S,H,dh', CASES)
@pytest.mark.parametrize('p', [0.0, 0.1])
def test_attention_fwd_bwd(B, S, H, dh, p):
    rs = np.random.RandomState(3)
    keylen = torch.from_numpy(rs.randint(max(S // 2, 1), S + 1, size=B).astype(np.int32))
    keylen[0] = S
    _fwd_bwd(B, S, H, dh, p, keylen)


def _fwd_bwd(B, S, H, dh, p, keylen, single_key=(), form=None):
    """Forward and backward with dbias_qkv at these key lengths: the global bars against the fp32 reference, the per-row
    bounds against fp64, lse, the exact zeros and the bias gradient.  single_key: the batch entries with keylen = 1, whose dq
    and dk are held by _check_single_key instead of the row bound."""
    from m3p_amd import ops, rng
    d = H * dh
    seed = 4242
    qkv, qkvc = randn_bf16((B * S, 3 * d), 1, 0.7)
    ctx, lse = ops.attn_fwd(qkv, keylen.cuda(), B, S, H, dh, seed=seed, p_drop=p)
    keep = None
    if p > 0:
        keep = torch.from_numpy(rng.keep_mask(B * H * S * S, seed, p, (B, H, S, S))).float()
    x = qkvc.clone().requires_grad_(True)
    ctx_ref, lse_ref = _ref_attention(x, keylen.long(), B, S, H, dh, keep, p)
    assert rel_l2(ctx.float(), ctx_ref) < GLOBAL_ATTN_CTX
    assert max_abs(lse, lse_ref) < 2e-3
    dctx, dctxc = randn_bf16((B * S, d), 7)
    dbias = torch.zeros(3 * d, device='cuda')
    kmask = None
    if p > 0:
        # the keep words the forward pass leaves for backward (required with dropout on since round 6): same outputs as without
        ctx2, lse2, kmask = ops.attn_fwd(qkv, keylen.cuda(), B, S, H, dh, seed=seed, p_drop=p, want_mask=True)
        assert torch.equal(ctx2, ctx) and torch.equal(lse2, lse)
        with pytest.raises(AssertionError):
            ops.attn_bwd(qkv, keylen.cuda(), ctx, dctx, lse, B, S, H, dh, dbias_qkv=dbias, seed=seed, p_drop=p)
    dqkv = ops.attn_bwd(qkv, keylen.cuda(), ctx, dctx, lse, B, S, H, dh, dbias_qkv=dbias, seed=seed, p_drop=p, keepmask=kmask)
    ctx_ref.backward(dctxc)
    g = x.grad.clone()
    g[:, :d] *= 1.0 / math.sqrt(dh)       # kernel returns the gradient of the unscaled q projection
    gall = float(g.norm())
    for name, sl in (('dq', slice(0, d)), ('dk', slice(d, 2 * d)), ('dv', slice(2 * d, 3 * d))):
        if float(g[:, sl].norm()) < 1e-6 * gall:      # a single key: softmax is constant, dq = dk = 0 exactly
            # (ours: D = rowsum(dO * O) uses the bf16-rounded O, so with dropout's 1/(1-p) scale a 2^-9 residue remains)
            assert float(dqkv[:, sl].float().norm()) < 1e-2 * gall, name
            continue
        assert rel_l2(dqkv[:, sl].float(), g[:, sl]) < GLOBAL_ATTN_GRAD, name
    ref64 = _ref64(qkv, keylen, dctx, B, S, H, dh, keep, p)
    _check_rows(ref64, B, S, H, dh, keylen, ctx=ctx, lse=lse, dqkv=dqkv, what='p=%g' % p, skip_ds=single_key, form=form)
    _check_single_key(ref64, qkv, ctx, dctx, dqkv, keep, B, S, H, dh, p, single_key, 'p=%g' % p)
    cs = dqkv.float().sum(0)
    assert rel_l2(dbias[:d], cs[:d]) < 1e-4 and rel_l2(dbias[2 * d:], cs[2 * d:]) < 1e-4   # column sums of the rows it wrote
    # k-bias: softmax shift invariance makes the true gradient 0 (the fp32 reference gives ~1e-7 noise);
    # the kernel writes exact zeros rather than the bf16 rounding noise of its dK rows
    assert bool((dbias[d:2 * d] == 0).all())
    assert float(g[:, d:2 * d].sum(0).abs().max()) <= 1e-3 * float(g[:, d:2 * d].abs().sum(0).max())


def test_attention_perf_smoke():
    from m3p_amd import ops
    B, S, H, dh = 256, 164, 12, 64
    d = H * dh
    qkv, _ = randn_bf16((B * S, 3 * d), 1, 0.7)
    keylen = torch.full((B,), S, dtype=torch.int32, device='cuda')
    for p in (0.0, 0.1):
        ctx, lse, km = ops.attn_fwd(qkv, keylen, B, S, H, dh, seed=1, p_drop=p, want_mask=True)
        dctx = torch.randn_like(ctx); dbias = torch.zeros(3 * d, device="cuda")
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            ops.attn_fwd(qkv, keylen, B, S, H, dh, seed=1, p_drop=p)
        e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 10
        fl = 4.0 * B * H * S * S * dh
        print('attn_fwd p=%.1f: %.3f ms  %.1f TF' % (p, ms, fl / ms / 1e9))
        e0.record()
        for _ in range(10):
            ops.attn_bwd(qkv, keylen, ctx, dctx, lse, B, S, H, dh, dbias_qkv=dbias, seed=1, p_drop=p, keepmask=km)
        e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 10
        print('attn_bwd p=%.1f: %.3f ms  %.1f TF (algorithmic 2x fwd)' % (p, ms, 2 * fl / ms / 1e9))


@pytest.mark.usefixtures('poison_outputs')
@pytest.mark.parametrize('B,S', [(32, 164), (5, 161), (4, 176), (3, 170), (256, 164)])      # 11 tiles / 6 steps: every length from 161 to 176; (256, 164) = the benchmarked launch, twelve heads per persistent workgroup
@pytest.mark.parametrize('p', [0.0, 0.1])
def test_attention_bwd_forms_for_the_m3p_sequence(p, B, S):
    """The three backward forms for 36 regions + 128 tokens (m3p_debug_attn_variant: 1 = two phases with the scores recomputed,
    2 = one pass - dS^T handed from phase A to phase B through LDS - as one twelve-wave workgroup per head, 0 = the same as a
    persistent kernel, the default) on MORE heads than CUs, so that persistent workgroups walk several heads: each against
    the fp32 reference at the kernel's usual bar, and against each other to bf16 rounding."""
    rs = np.random.RandomState(5)
    keylen = torch.from_numpy(rs.randint(S // 2, S + 1, size=B).astype(np.int32))
    keylen[0] = S
    _three_forms(B, S, 12, p, keylen)


def _three_forms(B, S, H, p, keylen, single_key=()):
    from m3p_amd import ops, rng, lib as L
    dh = 64
    assert bwd_band(S, dh)[1] == 'one-pass / persistent'
    d = H * dh
    seed = 99
    qkv, qkvc = randn_bf16((B * S, 3 * d), 11, 0.7)
    kw = dict(seed=seed, p_drop=p)
    if p > 0:
        ctx, lse, kmask = ops.attn_fwd(qkv, keylen.cuda(), B, S, H, dh, want_mask=True, **kw)
        keep = torch.from_numpy(rng.keep_mask(B * H * S * S, seed, p, (B, H, S, S))).float()
    else:
        (ctx, lse), kmask, keep = ops.attn_fwd(qkv, keylen.cuda(), B, S, H, dh, **kw), None, None
    x = qkvc.clone().requires_grad_(True)
    ctx_ref, _ = _ref_attention(x, keylen.long(), B, S, H, dh, keep, p)
    dctx, dctxc = randn_bf16((B * S, d), 13)
    ctx_ref.backward(dctxc)
    g = x.grad.clone()
    g[:, :d] *= 1.0 / math.sqrt(dh)
    ref64 = _ref64(qkv, keylen, dctx, B, S, H, dh, keep, p)
    _check_rows(ref64, B, S, H, dh, keylen, ctx=ctx, lse=lse, what='forward')
    outs = {}
    lib = L.load()
    try:
        for variant in (1, 2, 0):
            lib.m3p_debug_attn_variant(variant)
            dbias = torch.zeros(3 * d, device='cuda')
            dqkv = ops.attn_bwd(qkv, keylen.cuda(), ctx, dctx, lse, B, S, H, dh, dbias_qkv=dbias, keepmask=kmask, **kw)
            torch.cuda.synchronize()
            for name, sl in (('dq', slice(0, d)), ('dk', slice(d, 2 * d)), ('dv', slice(2 * d, 3 * d))):
                assert rel_l2(dqkv[:, sl].float(), g[:, sl]) < GLOBAL_ATTN_GRAD, (variant, name)
            cs = dqkv.float().sum(0)
            assert rel_l2(dbias[:d], cs[:d]) < 1e-4 and rel_l2(dbias[2 * d:], cs[2 * d:]) < 1e-4 and bool((dbias[d:2 * d] == 0).all()), variant
            _check_rows(ref64, B, S, H, dh, keylen, dqkv=dqkv, what='variant %d' % variant, skip_ds=single_key,
                        form=(None, FORMS_BWD[variant]))
            _check_single_key(ref64, qkv, ctx, dctx, dqkv, keep, B, S, H, dh, p, single_key, 'variant %d' % variant)
            outs[variant] = dqkv.float()
    finally:
        lib.m3p_debug_attn_variant(0)
    assert torch.equal(outs[2], outs[0])                                 # same arithmetic, different schedule
    assert torch.equal(outs[1][:, d:], outs[0][:, d:])                   # dK, dV: phase A is the same code in all three
    assert rel_l2(outs[1][:, :d], outs[0][:, :d]) < 2e-3                 # dQ: from recomputed scores against from the handed-over dS


# (B, S, H, dh) -> (nt, nk, forward instantiation at p = 0 and at p = 0.1, backward form): every band of the two launchers
# that CASES leaves out, and both sides of every band edge
BANDS = [
    # backward, S = 177 .. 192: the unrolled six-step form without the 11-tile constant
    ((2, 177, 2, 64), (12, 6, 'attn_fwd<KT = 6> four waves', None, 'attn_bwd<6, 0> unrolled')),
    ((2, 192, 3, 64), (12, 6, 'attn_fwd<KT = 6> four waves', None, 'attn_bwd<6, 0> unrolled')),
    ((1, 185, 2, 32), (12, 6, 'attn_fwd<KT = 6> four waves', None, 'attn_bwd<6, 0> unrolled')),
    # the M3P band (S = 161 .. 176) with 32-wide heads: never one-pass
    ((2, 164, 3, 32), (11, 6, 'attn_fwd<6, 11>', 'attn_fwd<6, 11> EVENS', 'attn_bwd<6, 11> two-phase')),
    ((2, 163, 2, 32), (11, 6, 'attn_fwd<6, 11>', 'attn_fwd<6, 11> odd S', 'attn_bwd<6, 11> two-phase')),
    ((1, 176, 2, 32), (11, 6, 'attn_fwd<6, 11>', 'attn_fwd<6, 11> EVENS', 'attn_bwd<6, 11> two-phase')),
    # band edges
    ((1, 160, 2, 64), (10, 5, 'attn_fwd<KT = 6> four waves', None, 'attn_bwd<0, 0> four waves')),
    ((1, 193, 2, 64), (13, 7, 'attn_fwd<KT = 12> four waves', None, 'attn_bwd<0, 0> four waves')),
    ((1, 320, 2, 64), (20, 10, 'attn_fwd<KT = 12> four waves', None, 'attn_bwd<0, 0> four waves')),
    ((1, 321, 2, 64), (21, 11, 'attn_fwd<KT = 12> eight waves (wide)', None, 'attn_bwd<0, 0> eight waves (wide)')),
    ((1, 384, 2, 32), (24, 12, 'attn_fwd<KT = 12> four waves', None, 'attn_bwd<0, 0> four waves')),
    ((1, 385, 2, 32), (25, 13, 'attn_fwd<KT = 16> eight waves', None, 'attn_bwd<0, 0> four waves')),
    ((1, 385, 1, 64), (25, 13, 'attn_fwd<KT = 16> eight waves (wide)', None, 'attn_bwd<0, 0> eight waves (wide)')),
    # forward, KT = 12 on four waves with 32-wide heads
    ((1, 300, 3, 32), (19, 10, 'attn_fwd<KT = 12> four waves', None, 'attn_bwd<0, 0> four waves')),
]


@pytest.mark.usefixtures('poison_outputs')
@pytest.mark.parametrize('shape,band', BANDS, ids=['%d-%d-%d-%d' % b[0] for b in BANDS])
@pytest.mark.parametrize('p', [0.0, 0.1])
def test_attention_launch_bands(shape, band, p):
    B, S, H, dh = shape
    nt, nk, fwd0, fwd_drop, bwd = band
    assert fwd_band(S, dh, p) == (nt, nk, (fwd_drop or fwd0) if p > 0 else fwd0), fwd_band(S, dh, p)
    assert bwd_band(S, dh) == (nk, bwd), bwd_band(S, dh)
    rs = np.random.RandomState(3)
    keylen = torch.from_numpy(rs.randint(max(S // 2, 1), S + 1, size=B).astype(np.int32))
    keylen[0] = S
    _fwd_bwd(B, S, H, dh, p, keylen, form=_forms(S, dh, p))


@pytest.mark.usefixtures('poison_outputs')
@pytest.mark.parametrize('p', [0.0, 0.1])
def test_attention_bwd_persistent_with_one_head_more_than_cus(p):
    """B * H = the CU count + 1: exactly one persistent workgroup walks a second head, every other one a single head."""
    S = 164
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    B, H = n_cu + 1, 1
    assert B * H == n_cu + 1 and bwd_band(S, 64) == (6, 'one-pass / persistent')
    rs = np.random.RandomState(5)
    keylen = torch.from_numpy(rs.randint(S // 2, S + 1, size=B).astype(np.int32))
    keylen[0] = S
    keylen[-1] = S - 3           # the head that is walked second
    _three_forms(B, S, H, p, keylen)


SHORT = [((11, 164, 2, 64), 'one-pass / persistent'), ((11, 74, 2, 32), 'attn_bwd<0, 0> four waves'),
         ((11, 180, 2, 64), 'attn_bwd<6, 0> unrolled'), ((11, 200, 2, 32), 'attn_bwd<0, 0> four waves'),
         ((11, 356, 2, 64), 'attn_bwd<0, 0> eight waves (wide)')]


@pytest.mark.usefixtures('poison_outputs')
@pytest.mark.parametrize('shape,bwd', SHORT, ids=['%d-%d-%d-%d' % b[0] for b in SHORT])
@pytest.mark.parametrize('p', [0.0, 0.1])
def test_attention_short_key_lengths(shape, bwd, p):
    """keylen far below S, as in text-only batches padded to the batch maximum: whole 16-key tiles and whole 32-key MFMA steps
    behind keylen are masked, in the forward kernel and in both phases of every backward form, and the wave-uniform test
    16 t + 16 > keylen decides which tiles get per-element compares."""
    B, S, H, dh = shape
    assert bwd_band(S, dh)[1] == bwd
    want = [S, 1, 2, 15, 16, 17, 31, 32, 33, S // 2 - 1, S - 1]
    kl = [min(v, S) for v in want]
    assert len(kl) == B and any(v < 16 for v in kl) and any(17 <= v <= 31 for v in kl) and min(kl) >= 1
    keylen = torch.tensor(kl, dtype=torch.int32)
    single = tuple(b for b in range(B) if kl[b] == 1)
    assert single == (1,)
    _fwd_bwd(B, S, H, dh, p, keylen, single_key=single, form=_forms(S, dh, p))
    if S == 164:
        _three_forms(B, S, H, p, keylen, single_key=single)


def test_zz_report_attention():
    """Not a check: the largest normalised error (1 = the bar) each kernel form reached in this module's tests."""
    for key in sorted(WORST):
        print('attention  %s  %.3g' % (key, WORST[key]))
