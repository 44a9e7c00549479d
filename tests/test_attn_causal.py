"""Tiled causal self-attention of the causal language-model pass (csrc/attn_tiled.hip: m3p_attn_causal_fwd / _bwd) against
fp64 torch autograd on the same bf16 operands, with the position-only causal mask and the dropout keep mask of the RNG twin
(the stream index of the rows kernels, so the two implementations are interchangeable under one seed).

Shapes are the smallest that reach each path of the kernels (blocks of 64 queries / keys, 16 per wave): one key, less than
a tile, exactly one block, one row over, a ragged third block, the workload's T = 256, one short of the cap and the cap.
Outputs live inside larger poisoned buffers: an unwritten element reads NaN, and the guard rows around them must keep their
bits.  (The compiler's resource summary of every instantiation is read in test_attn_tiled.py.)"""
import numpy as np
import pytest
import torch

from tests.util import (ATTN_CTX_RTOL, ATTN_DS_FLOOR, ATTN_DS_RTOL, GLOBAL_ATTN_CTX, GLOBAL_ATTN_GRAD, ROW_FLOOR,
                        assert_bits_equal, assert_block_bound, assert_guards, guarded, heads, poisoned_outputs, rel_l2)

BF16 = torch.bfloat16
SEED = 4242
SHAPES = [(2, 1, 2, 32, 0.0), (3, 17, 4, 32, 0.1), (2, 64, 2, 64, 0.1), (2, 65, 12, 64, 0.1), (1, 130, 4, 64, 0.0),
          (2, 256, 12, 64, 0.1), (1, 511, 2, 64, 0.1), (1, 512, 2, 32, 0.1)]


def _inputs(B, T, H, dh):
    d = H * dh
    g = torch.Generator(device='cuda').manual_seed(7)
    qkv = torch.randn(B * T, 3 * d, device='cuda', generator=g)
    qkv[:, :d] *= 1.0 / np.sqrt(dh)                          # the q columns as the projection's epilogue leaves them
    dctx = torch.randn(B * T, d, device='cuda', generator=g).to(BF16)
    return qkv.to(BF16), dctx


def _reference(qkv, dctx, B, T, H, dh, p):
    """fp64 autograd -> ctx, lse, dq (of the unscaled projection), dk, dv as [B, H, T, dh] / [B, H, T]."""
    from m3p_amd import rng
    d = H * dh
    qf, kf, vf = (heads(qkv[:, i * d:(i + 1) * d].double(), B, T, H, dh).clone().requires_grad_(True) for i in range(3))
    s = qf @ kf.transpose(2, 3)
    j = torch.arange(T, device='cuda')
    s = s.masked_fill(~(j[None, :] <= j[:, None])[None, None], float('-inf'))
    pr = torch.softmax(s, -1)
    if p > 0:
        pr = pr * torch.from_numpy(rng.keep_mask(B * H * T * T, SEED, p, (B, H, T, T))).cuda() / (1 - p)
    ctx = pr @ vf
    ctx.backward(heads(dctx.double(), B, T, H, dh))
    return ctx.detach(), torch.logsumexp(s, -1).detach(), qf.grad / np.sqrt(dh), kf.grad, vf.grad


def _tiled(qkv, dctx, B, T, H, dh, p):
    """The tiled kernels into guarded buffers -> ctx, lse, dqkv."""
    from m3p_amd import ops
    d = H * dh
    cbuf, ctx = guarded(B * T, d, BF16)
    lbuf, lse = guarded(B * H, T, torch.float32)
    gbuf, dqkv = guarded(B * T, 3 * d, BF16)
    with poisoned_outputs():
        out = ops.attn_causal_fwd(qkv, B, T, H, dh, seed=SEED, p_drop=p, out=(ctx, lse.view(B, H, T)))
        assert out is not None and out[0] is ctx
        got = ops.attn_causal_bwd(qkv, dctx, lse.view(B, H, T), B, T, H, dh, 1.0 / np.sqrt(dh), seed=SEED, p_drop=p, out=dqkv)
        assert got is dqkv
    torch.cuda.synchronize()
    for buf, name in ((cbuf, 'ctx'), (lbuf, 'lse'), (gbuf, 'dqkv')):
        assert_guards(buf, name)
    return ctx, lse.view(B, H, T), dqkv


def _check(ctx, lse, dqkv, ref, B, T, H, dh, what):
    d = H * dh
    r_ctx, r_lse, r_dq, r_dk, r_dv = ref
    dq, dk, dv = (heads(dqkv[:, i * d:(i + 1) * d], B, T, H, dh) for i in range(3))
    for t, name in ((ctx, 'ctx'), (lse, 'lse'), (dq, 'dq'), (dk, 'dk'), (dv, 'dv')):
        assert bool(torch.isfinite(t.float()).all()), '%s: %s holds an element that is not finite (never written?)' % (what, name)
    ctx_h = heads(ctx, B, T, H, dh)
    figures = dict(ctx=rel_l2(ctx_h, r_ctx), lse=rel_l2(lse, r_lse), dq=rel_l2(dq, r_dq), dk=rel_l2(dk, r_dk), dv=rel_l2(dv, r_dv))
    print(what, ' '.join('%s %.3g' % kv for kv in figures.items()))
    assert figures['ctx'] < GLOBAL_ATTN_CTX, (what, figures)
    assert figures['lse'] < 1e-4, (what, figures)
    for k in ('dq', 'dk', 'dv'):
        assert figures[k] < GLOBAL_ATTN_GRAD, (what, figures)
    assert_block_bound(ctx_h, r_ctx, ('b', 'h', 'row'), ATTN_CTX_RTOL, ROW_FLOOR, what + ' ctx')
    assert_block_bound(dv, r_dv, ('b', 'h', 'key'), ATTN_CTX_RTOL, ROW_FLOOR, what + ' dv')
    assert_block_bound(dq, r_dq, ('b', 'h', 'row'), ATTN_DS_RTOL, ATTN_DS_FLOOR, what + ' dq')
    assert_block_bound(dk, r_dk, ('b', 'h', 'key'), ATTN_DS_RTOL, ATTN_DS_FLOOR, what + ' dk')


@pytest.mark.gpu
@pytest.mark.parametrize('B,T,H,dh,p', SHAPES)
def test_attn_causal_kernels_vs_autograd(B, T, H, dh, p):
    qkv, dctx = _inputs(B, T, H, dh)
    ref = _reference(qkv, dctx, B, T, H, dh, p)
    ctx, lse, dqkv = _tiled(qkv, dctx, B, T, H, dh, p)
    _check(ctx, lse, dqkv, ref, B, T, H, dh, 'attn_causal %s' % ((B, T, H, dh, p),))


@pytest.mark.gpu
def test_rows_and_tiled_kernels_share_one_dropout_stream():
    """Under one seed the rows kernels and the tiled ones drop the same probabilities: both meet the bars against ONE
    reference built from one keep mask, and each other within them."""
    from m3p_amd import ops
    B, T, H, dh, p = 2, 65, 12, 64, 0.1
    d = H * dh
    qkv, dctx = _inputs(B, T, H, dh)
    ref = _reference(qkv, dctx, B, T, H, dh, p)
    ctx, lse, dqkv = _tiled(qkv, dctx, B, T, H, dh, p)
    kv = qkv.view(B, T, 3 * d)[:, :, d:]
    with poisoned_outputs():
        r_ctx, r_lse = ops.attn_rows_fwd(qkv, kv, None, B, T, H, dh, T, causal=True, seed=SEED, p_drop=p)
        r_dqkv = torch.empty_like(qkv)
        _, dkv = ops.attn_rows_bwd(qkv, kv, None, dctx, r_lse, B, T, H, dh, T, 1.0 / np.sqrt(dh), causal=True, seed=SEED, p_drop=p,
                                   dq_out=r_dqkv)
    r_dqkv.view(B, T, 3 * d)[:, :, d:] = dkv
    _check(r_ctx, r_lse, r_dqkv, ref, B, T, H, dh, 'rows kernels against the reference')
    rows = (heads(r_ctx.double(), B, T, H, dh), r_lse.double()) + tuple(
        heads(r_dqkv[:, i * d:(i + 1) * d].double(), B, T, H, dh) for i in range(3))
    _check(ctx, lse, dqkv, rows, B, T, H, dh, 'tiled against rows kernels')


@pytest.mark.gpu
def test_strided_qkv_and_dqkv_give_the_packed_results_bit_for_bit():
    """qkv as the first 3d columns of a NaN-filled [B*T, 3d + 16] buffer, dqkv out into the same kind of slice: the pitch is
    not the packed one.  Two query blocks, the second ragged: the smallest shape where a diagonal and an off-diagonal tile
    run."""
    from m3p_amd import ops
    B, T, H, dh, p = 2, 65, 4, 64, 0.1
    d = H * dh
    qkv, dctx = _inputs(B, T, H, dh)
    packed = _tiled(qkv, dctx, B, T, H, dh, p)
    wide = torch.full((B * T, 3 * d + 16), float('nan'), dtype=BF16, device='cuda')
    wide[:, :3 * d] = qkv
    qkv_s = wide[:, :3 * d]
    gbuf, gwide = guarded(B * T, 3 * d + 16, BF16)
    dqkv_s = gwide[:, :3 * d]
    assert qkv_s.stride(0) == 3 * d + 16 and dqkv_s.stride(0) == 3 * d + 16
    with poisoned_outputs():
        ctx, lse = ops.attn_causal_fwd(qkv_s, B, T, H, dh, seed=SEED, p_drop=p)
        got = ops.attn_causal_bwd(qkv_s, dctx, lse, B, T, H, dh, 1.0 / np.sqrt(dh), seed=SEED, p_drop=p, out=dqkv_s)
        assert got is dqkv_s
    torch.cuda.synchronize()
    assert_guards(gbuf, 'strided dqkv')
    poison = torch.empty_like(gwide)
    poison.untyped_storage().fill_(0xFF)
    assert_bits_equal(gwide[:, 3 * d:], poison[:, 3 * d:], 'strided dqkv: columns behind the slice')
    for a, b, name in zip((ctx, lse, dqkv_s), packed, ('ctx', 'lse', 'dqkv')):
        assert_bits_equal(a, b, 'strided qkv / dqkv: ' + name)


@pytest.mark.gpu
def test_two_launches_give_the_same_bits():
    """(The D value parked in the dq slot must not leak from one launch into the next.)"""
    B, T, H, dh, p = 1, 130, 4, 64, 0.1
    qkv, dctx = _inputs(B, T, H, dh)
    first = _tiled(qkv, dctx, B, T, H, dh, p)
    second = _tiled(qkv, dctx, B, T, H, dh, p)
    for a, b, name in zip(first, second, ('ctx', 'lse', 'dqkv')):
        assert_bits_equal(a, b, 'second launch: ' + name)


@pytest.mark.gpu
@pytest.mark.parametrize('B,T,H,dh', [(1, 513, 2, 64), (2, 40, 2, 48)])
def test_shapes_outside_the_tiled_kernels_are_declined(B, T, H, dh):
    from m3p_amd import ops
    qkv, dctx = _inputs(B, T, H, dh)
    lse = torch.zeros((B, H, T), dtype=torch.float32, device='cuda')
    assert ops.attn_causal_fwd(qkv, B, T, H, dh, seed=SEED, p_drop=0.1) is None
    assert ops.attn_causal_bwd(qkv, dctx, lse, B, T, H, dh, 1.0 / np.sqrt(dh), seed=SEED, p_drop=0.1) is None
