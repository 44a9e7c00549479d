"""Tiled attention over a source encoding (csrc/attn_tiled.hip: m3p_attn_cross_fwd / _bwd) against fp64 torch autograd on
the same bf16 operands, with per-sequence key counts and the dropout keep mask of the RNG twin under the stream index of
the rows kernels (so the two implementations are interchangeable under one seed).

Shapes are the smallest that reach each path of the kernels (blocks of 64 queries / keys, 16 per wave).  Key / value rows
at or past klen[b] hold NaN before the launch: nothing of them may reach an output, and their dk / dv rows are exact
zeros.  Outputs live inside larger poisoned buffers: an unwritten element reads NaN, and the guard rows around them must
keep their bits.  (The compiler's resource summary of every instantiation is read in test_attn_tiled.py.)"""
import numpy as np
import pytest
import torch

from tests.util import (ATTN_CTX_RTOL, ATTN_DS_FLOOR, ATTN_DS_RTOL, GLOBAL_ATTN_CTX, GLOBAL_ATTN_GRAD, ROW_FLOOR,
                        assert_bits_equal, assert_block_bound, assert_exact_zero, assert_guards, guarded, heads, poisoned_outputs,
                        rel_l2)

BF16 = torch.bfloat16
SEED = 4242
# (B, Tq, H, dh, Lk, p): one query and one key; under a tile on both sides; exactly one block each; one row over and one key
# short; caption-shaped with a ragged third key tile; three query blocks over short keys; 100 regions; the translation shape;
# both caps
SHAPES = [(2, 1, 2, 32, 1, 0.0), (3, 17, 4, 32, 9, 0.1), (2, 64, 2, 64, 64, 0.1), (2, 65, 12, 64, 63, 0.1),
          (2, 5, 4, 64, 130, 0.0), (1, 130, 4, 64, 37, 0.1), (2, 40, 12, 64, 100, 0.1), (1, 256, 2, 64, 256, 0.1),
          (1, 512, 2, 32, 1024, 0.1)]


def _klen(B, Lk, g):
    """Random on [1, Lk]; pinned where B and Lk allow: klen[0] = Lk, then one sequence at 1, one at a multiple of 64 and one
    at a multiple of 64 plus 1."""
    klen = torch.randint(1, Lk + 1, (B,), device='cuda', generator=g).to(torch.int32)
    pins = [Lk, 1]
    if Lk >= 64:
        pins.append(Lk // 64 * 64)
    if Lk >= 65:
        pins.append((Lk - 1) // 64 * 64 + 1)
    for b, v in zip(range(B), pins):
        klen[b] = v
    return klen


def _inputs(B, Tq, H, dh, Lk, klen=None):
    """q (scaled, as the projection's epilogue leaves it), kv with NaN in every row at or past klen[b], klen, dctx."""
    d = H * dh
    g = torch.Generator(device='cuda').manual_seed(7)
    q = (torch.randn(B * Tq, d, device='cuda', generator=g) / np.sqrt(dh)).to(BF16)
    kv = torch.randn(B, Lk, 2 * d, device='cuda', generator=g).to(BF16)
    dctx = torch.randn(B * Tq, d, device='cuda', generator=g).to(BF16)
    if klen is None:
        klen = _klen(B, Lk, g)
    past = torch.arange(Lk, device='cuda')[None, :] >= klen[:, None]
    kv[past] = float('nan')
    return q, kv, klen, dctx


def _reference(q, kv, klen, dctx, B, Tq, H, dh, Lk, p):
    """fp64 autograd -> ctx, lse, dq (of the unscaled projection) as [B, H, Tq, dh] / [B, H, Tq], dk, dv as [B, H, Lk, dh].
    (The NaN rows past klen are replaced by zeros here: the kernels may not read them.)  A sequence without keys has
    ctx = lse = 0 and no gradient."""
    from m3p_amd import rng
    d = H * dh
    past = torch.arange(Lk, device='cuda')[None, :] >= klen[:, None]
    kvc = kv.double().masked_fill(past[:, :, None], 0.0)
    qf = heads(q.double(), B, Tq, H, dh).clone().requires_grad_(True)
    kf = heads(kvc[:, :, :d], B, Lk, H, dh).clone().requires_grad_(True)
    vf = heads(kvc[:, :, d:], B, Lk, H, dh).clone().requires_grad_(True)
    s = (qf @ kf.transpose(2, 3)).masked_fill(past[:, None, None, :], float('-inf'))
    empty = (klen == 0)[:, None, None, None]
    pr = torch.softmax(s.masked_fill(empty, 0.0), -1).masked_fill(empty | past[:, None, None, :], 0.0)
    if p > 0:
        pr = pr * torch.from_numpy(rng.keep_mask(B * H * Tq * Lk, SEED, p, (B, H, Tq, Lk))).cuda() / (1 - p)
    ctx = pr @ vf
    ctx.backward(heads(dctx.double(), B, Tq, H, dh))
    lse = torch.logsumexp(s.masked_fill(empty, 0.0), -1).masked_fill(empty[..., 0], 0.0)
    return ctx.detach(), lse.detach(), qf.grad / np.sqrt(dh), kf.grad, vf.grad


def _tiled(q, kv, klen, dctx, B, Tq, H, dh, Lk, p):
    """The tiled kernels into guarded buffers -> ctx, lse, dq, dkv."""
    from m3p_amd import ops
    d = H * dh
    cbuf, ctx = guarded(B * Tq, d, BF16)
    lbuf, lse = guarded(B * H, Tq, torch.float32)
    qbuf, dq = guarded(B * Tq, d, BF16)
    kbuf, dkv = guarded(B * Lk, 2 * d, BF16)
    with poisoned_outputs():
        out = ops.attn_cross_fwd(q, kv, klen, B, Tq, H, dh, Lk, seed=SEED, p_drop=p, out=(ctx, lse.view(B, H, Tq)))
        assert out is not None and out[0] is ctx
        got = ops.attn_cross_bwd(q, kv, klen, dctx, lse.view(B, H, Tq), B, Tq, H, dh, Lk, 1.0 / np.sqrt(dh), seed=SEED, p_drop=p,
                                 out=(dq, dkv.view(B, Lk, 2 * d)))
        assert got is not None and got[0] is dq
    torch.cuda.synchronize()
    for buf, name in ((cbuf, 'ctx'), (lbuf, 'lse'), (qbuf, 'dq'), (kbuf, 'dkv')):
        assert_guards(buf, name)
    return ctx, lse.view(B, H, Tq), dq, dkv.view(B, Lk, 2 * d)


def _check(ctx, lse, dq, dkv, ref, klen, B, Tq, H, dh, Lk, what, seqs=None):
    """The bars of tests/util.py over the sequences ``seqs`` (all of them by default)."""
    d = H * dh
    for t, name in ((ctx, 'ctx'), (lse, 'lse'), (dq, 'dq'), (dkv, 'dkv')):
        assert bool(torch.isfinite(t.float()).all()), '%s: %s holds an element that is not finite' % (what, name)
    if klen is not None:
        past = torch.arange(Lk, device='cuda')[None, :] >= klen[:, None]
        assert_exact_zero(dkv[past], what + ' dk, dv of keys past the sequence')
    sel = slice(None) if seqs is None else seqs
    got = (heads(ctx, B, Tq, H, dh), lse, heads(dq, B, Tq, H, dh), heads(dkv[:, :, :d].reshape(B * Lk, d), B, Lk, H, dh),
           heads(dkv[:, :, d:].reshape(B * Lk, d), B, Lk, H, dh))
    g_ctx, g_lse, g_dq, g_dk, g_dv = (t[sel] for t in got)
    r_ctx, r_lse, r_dq, r_dk, r_dv = (t[sel] for t in ref)
    figures = dict(ctx=rel_l2(g_ctx, r_ctx), lse=rel_l2(g_lse, r_lse), dq=rel_l2(g_dq, r_dq), dk=rel_l2(g_dk, r_dk),
                   dv=rel_l2(g_dv, r_dv))
    print(what, ' '.join('%s %.3g' % kv for kv in figures.items()))
    assert figures['ctx'] < GLOBAL_ATTN_CTX, (what, figures)
    assert figures['lse'] < 1e-4, (what, figures)
    for k in ('dq', 'dk', 'dv'):
        assert figures[k] < GLOBAL_ATTN_GRAD, (what, figures)
    assert_block_bound(g_ctx, r_ctx, ('b', 'h', 'row'), ATTN_CTX_RTOL, ROW_FLOOR, what + ' ctx')
    assert_block_bound(g_dv, r_dv, ('b', 'h', 'key'), ATTN_CTX_RTOL, ROW_FLOOR, what + ' dv')
    assert_block_bound(g_dq, r_dq, ('b', 'h', 'row'), ATTN_DS_RTOL, ATTN_DS_FLOOR, what + ' dq')
    assert_block_bound(g_dk, r_dk, ('b', 'h', 'key'), ATTN_DS_RTOL, ATTN_DS_FLOOR, what + ' dk')


@pytest.mark.gpu
@pytest.mark.parametrize('B,Tq,H,dh,Lk,p', SHAPES)
def test_attn_cross_kernels_vs_autograd(B, Tq, H, dh, Lk, p):
    q, kv, klen, dctx = _inputs(B, Tq, H, dh, Lk)
    ref = _reference(q, kv, klen, dctx, B, Tq, H, dh, Lk, p)
    ctx, lse, dq, dkv = _tiled(q, kv, klen, dctx, B, Tq, H, dh, Lk, p)
    _check(ctx, lse, dq, dkv, ref, klen, B, Tq, H, dh, Lk, 'attn_cross %s klen %s' % ((B, Tq, H, dh, Lk, p), klen.tolist()))


@pytest.mark.gpu
def test_strided_operands_give_the_packed_results_bit_for_bit():
    """q as a column slice of a wider buffer (ld_q > d), kv as big[:, :Lk] of a [B, Lk + 5, 2d + 16] tensor: neither the
    batch stride nor the pitch is the packed one."""
    B, Tq, H, dh, Lk, p = 2, 40, 4, 64, 100, 0.1
    d = H * dh
    q, kv, klen, dctx = _inputs(B, Tq, H, dh, Lk)
    packed = _tiled(q, kv, klen, dctx, B, Tq, H, dh, Lk, p)
    wide = torch.full((B * Tq, 3 * d), float('nan'), dtype=BF16, device='cuda')
    wide[:, d:2 * d] = q
    big = torch.full((B, Lk + 5, 2 * d + 16), float('nan'), dtype=BF16, device='cuda')
    big[:, :Lk, :2 * d] = kv
    q_s, kv_s = wide[:, d:2 * d], big[:, :Lk]
    assert q_s.stride(0) == 3 * d and kv_s.stride(0) == (Lk + 5) * (2 * d + 16) and kv_s.stride(1) == 2 * d + 16
    strided = _tiled(q_s, kv_s, klen, dctx, B, Tq, H, dh, Lk, p)
    for a, b, name in zip(strided, packed, ('ctx', 'lse', 'dq', 'dkv')):
        assert_bits_equal(a, b, 'strided operands: ' + name)


@pytest.mark.gpu
def test_a_sequence_without_keys_gives_exact_zeros():
    B, Tq, H, dh, Lk, p = 3, 70, 4, 64, 100, 0.1
    klen = torch.tensor([100, 0, 65], dtype=torch.int32, device='cuda')
    q, kv, klen, dctx = _inputs(B, Tq, H, dh, Lk, klen=klen)
    ref = _reference(q, kv, klen, dctx, B, Tq, H, dh, Lk, p)
    ctx, lse, dq, dkv = _tiled(q, kv, klen, dctx, B, Tq, H, dh, Lk, p)
    assert_exact_zero(ctx.view(B, Tq, -1)[1], 'ctx of the sequence without keys')
    assert_exact_zero(lse[1], 'lse of the sequence without keys')
    assert_exact_zero(dq.view(B, Tq, -1)[1], 'dq of the sequence without keys')
    assert_exact_zero(dkv[1], 'dkv of the sequence without keys')
    _check(ctx, lse, dq, dkv, ref, klen, B, Tq, H, dh, Lk, 'attn_cross beside a sequence without keys', seqs=[0, 2])


@pytest.mark.gpu
def test_rows_and_tiled_cross_kernels_share_one_dropout_stream():
    """Under one seed the rows kernels and the tiled ones drop the same probabilities: both meet the bars against ONE
    reference built from one keep mask, and each other within them."""
    from m3p_amd import ops
    B, Tq, H, dh, Lk, p = 2, 65, 12, 64, 100, 0.1
    d = H * dh
    q, kv, klen, dctx = _inputs(B, Tq, H, dh, Lk)
    ref = _reference(q, kv, klen, dctx, B, Tq, H, dh, Lk, p)
    ctx, lse, dq, dkv = _tiled(q, kv, klen, dctx, B, Tq, H, dh, Lk, p)
    with poisoned_outputs():
        r_ctx, r_lse = ops.attn_rows_fwd(q, kv, klen, B, Tq, H, dh, Lk, seed=SEED, p_drop=p)
        r_dq, r_dkv = ops.attn_rows_bwd(q, kv, klen, dctx, r_lse, B, Tq, H, dh, Lk, 1.0 / np.sqrt(dh), seed=SEED, p_drop=p)
    _check(r_ctx, r_lse, r_dq, r_dkv, ref, klen, B, Tq, H, dh, Lk, 'rows kernels against the reference')
    rows = (heads(r_ctx.double(), B, Tq, H, dh), r_lse.double(), heads(r_dq.double(), B, Tq, H, dh),
            heads(r_dkv[:, :, :d].double().reshape(B * Lk, d), B, Lk, H, dh),
            heads(r_dkv[:, :, d:].double().reshape(B * Lk, d), B, Lk, H, dh))
    _check(ctx, lse, dq, dkv, rows, klen, B, Tq, H, dh, Lk, 'tiled against rows kernels')


@pytest.mark.gpu
def test_two_launches_give_the_same_bits():
    B, Tq, H, dh, Lk, p = 2, 130, 4, 64, 200, 0.1
    q, kv, klen, dctx = _inputs(B, Tq, H, dh, Lk)
    first = _tiled(q, kv, klen, dctx, B, Tq, H, dh, Lk, p)
    second = _tiled(q, kv, klen, dctx, B, Tq, H, dh, Lk, p)
    for a, b, name in zip(first, second, ('ctx', 'lse', 'dq', 'dkv')):
        assert_bits_equal(a, b, 'second launch: ' + name)


@pytest.mark.gpu
@pytest.mark.parametrize('B,Tq,H,dh,Lk', [(2, 40, 2, 48, 40), (1, 8, 2, 64, 1025)])
def test_shapes_outside_the_tiled_cross_kernels_are_declined(B, Tq, H, dh, Lk):
    from m3p_amd import ops
    q, kv, klen, dctx = _inputs(B, Tq, H, dh, Lk)
    lse = torch.zeros((B, H, Tq), dtype=torch.float32, device='cuda')
    assert ops.attn_cross_fwd(q, kv, klen, B, Tq, H, dh, Lk, seed=SEED, p_drop=0.1) is None
    assert ops.attn_cross_bwd(q, kv, klen, dctx, lse, B, Tq, H, dh, Lk, 1.0 / np.sqrt(dh), seed=SEED, p_drop=0.1) is None
