"""The prefill kernel (csrc/attn_tiled.hip: m3p_attn_prefix_fwd, the prefix mask of the tiled forward body) against fp64
torch on the same bf16 operands: Tq new queries behind pos0 cached positions, query t sees keys 0 .. pos0 + t.

Shapes are the smallest that reach each path: the diagonal inside one 16-key sub-tile, across two of them, across two key
tiles, tile-aligned, several query blocks, both caps.  The cache has spare capacity behind pos0 + Tq, and every row there
holds NaN before the launch: nothing of it may reach an output.  Outputs live inside larger poisoned buffers: an unwritten
element reads NaN, and the guard rows around them must keep their bits."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests.util import (ATTN_CTX_RTOL, GLOBAL_ATTN_CTX, ROW_FLOOR, assert_bits_equal, assert_block_bound, assert_guards, guarded,
                        heads, poisoned_outputs, rel_l2)

BF16 = torch.bfloat16
SPARE = 7           # cache rows behind pos0 + Tq (NaN)
# (B, Tq, H, dh, pos0): the smallest case; a small offset; the diagonal across two sub-tiles; sub-tile aligned; the diagonal
# across two key tiles; tile aligned with a second query block of one row; three query blocks, unaligned; both caps
SHAPES = [(2, 1, 2, 32, 0), (2, 8, 4, 32, 1), (3, 17, 4, 64, 15), (2, 16, 2, 64, 16), (2, 64, 12, 64, 63), (2, 65, 2, 64, 64),
          (1, 130, 4, 64, 100), (1, 512, 2, 32, 512)]


@functools.lru_cache(maxsize=None)
def _case(B, Tq, H, dh, pos0):
    """q (scaled), the cache kv [B, pos0 + Tq + SPARE, 2d] with NaN behind pos0 + Tq, and the fp64 reference (ctx, lse) as
    [B, H, Tq, dh] / [B, H, Tq] - computed once per shape and left unchanged."""
    d, Lk = H * dh, pos0 + Tq
    g = torch.Generator(device='cuda').manual_seed(11)
    q = (torch.randn(B * Tq, d, device='cuda', generator=g) / np.sqrt(dh)).to(BF16)
    kv = torch.randn(B, Lk + SPARE, 2 * d, device='cuda', generator=g).to(BF16)
    kv[:, Lk:] = float('nan')
    qf = heads(q.double(), B, Tq, H, dh)
    kf = heads(kv[:, :Lk, :d].double().reshape(B * Lk, d), B, Lk, H, dh)
    vf = heads(kv[:, :Lk, d:].double().reshape(B * Lk, d), B, Lk, H, dh)
    hidden = torch.arange(Lk, device='cuda')[None, :] > pos0 + torch.arange(Tq, device='cuda')[:, None]
    s = (qf @ kf.transpose(2, 3)).masked_fill(hidden[None, None], float('-inf'))
    return q, kv, torch.softmax(s, -1) @ vf, torch.logsumexp(s, -1)


def _prefix(q, kv, B, Tq, H, dh, pos0):
    """The kernel into guarded buffers -> ctx, lse."""
    from m3p_amd import ops
    cbuf, ctx = guarded(B * Tq, H * dh, BF16)
    lbuf, lse = guarded(B * H, Tq, torch.float32)
    with poisoned_outputs():
        out = ops.attn_prefix_fwd(q, kv, B, Tq, H, dh, pos0, out=(ctx, lse.view(B, H, Tq)))
        assert out is not None and out[0] is ctx
    torch.cuda.synchronize()
    assert_guards(cbuf, 'ctx')
    assert_guards(lbuf, 'lse')
    return ctx, lse.view(B, H, Tq)


def _check(ctx, lse, r_ctx, r_lse, B, Tq, H, dh, what):
    assert bool(torch.isfinite(ctx.float()).all()) and bool(torch.isfinite(lse).all()), what + ': an element is not finite'
    figures = dict(ctx=rel_l2(heads(ctx, B, Tq, H, dh), r_ctx), lse=rel_l2(lse, r_lse))
    print(what, ' '.join('%s %.3g' % kv for kv in figures.items()))
    assert figures['ctx'] < GLOBAL_ATTN_CTX, (what, figures)
    assert figures['lse'] < 1e-4, (what, figures)
    assert_block_bound(heads(ctx, B, Tq, H, dh), r_ctx, ('b', 'h', 'row'), ATTN_CTX_RTOL, ROW_FLOOR, what + ' ctx')


HIPCC = '/opt/rocm/bin/hipcc'


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not installed')
def test_prefix_kernels_use_no_scratch_and_keep_the_causal_forwards_occupancy(tmp_path):
    """The two instantiations as the compiler leaves them (the ca_waves comment of csrc/attn_tiled.hip and DESIGN.md 4 state
    these): four waves per SIMD at dh = 64, five at dh = 32, no scratch."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / 'attn_tiled.s')
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-munsafe-fp-atomics', '-ffp-contract=fast', '-S',
                    '--cuda-device-only', os.path.join(root, 'm3p_amd', 'csrc', 'attn_tiled.hip'), '-o', out], check=True,
                   capture_output=True)
    seen = {}
    for m in re.finditer(r'^(_Z\w*attn_prefix_fwd_kernelILi(\d+)E\w*):.*?^; Kernel info:(.*?)^; COMPUTE_PGM_RSRC2', open(out).read(),
                         re.S | re.M):
        info = m.group(3)
        seen[int(m.group(2))] = (int(re.search(r'ScratchSize: (\d+)', info).group(1)), int(re.search(r'Occupancy: (\d+)', info).group(1)))
    assert seen == {64: (0, 4), 32: (0, 5)}, seen


@pytest.mark.gpu
@pytest.mark.parametrize('B,Tq,H,dh,pos0', SHAPES)
def test_attn_prefix_kernel_vs_fp64(B, Tq, H, dh, pos0):
    q, kv, r_ctx, r_lse = _case(B, Tq, H, dh, pos0)
    ctx, lse = _prefix(q, kv, B, Tq, H, dh, pos0)
    _check(ctx, lse, r_ctx, r_lse, B, Tq, H, dh, 'attn_prefix %s' % ((B, Tq, H, dh, pos0),))


@pytest.mark.gpu
@pytest.mark.parametrize('B,Tq,H,dh,pos0', SHAPES)
def test_rows_kernel_agrees_within_the_same_bars(B, Tq, H, dh, pos0):
    """m3p_attn_query_fwd(causal = 1, pos0) - the fallback - meets the bars against the same reference, and the tiled kernel
    meets them against the rows kernel's context."""
    from m3p_amd import ops
    q, kv, r_ctx, r_lse = _case(B, Tq, H, dh, pos0)
    with poisoned_outputs():
        rows = ops.attn_query_fwd(q, kv, None, B, Tq, H, dh, pos0 + Tq, causal=True, pos0=pos0)
    ctx, lse = _prefix(q, kv, B, Tq, H, dh, pos0)
    what = 'rows / tiled %s' % ((B, Tq, H, dh, pos0),)
    assert_block_bound(heads(rows, B, Tq, H, dh), r_ctx, ('b', 'h', 'row'), ATTN_CTX_RTOL, ROW_FLOOR, what + ' rows ctx')
    assert rel_l2(heads(rows, B, Tq, H, dh), r_ctx) < GLOBAL_ATTN_CTX
    _check(ctx, lse, heads(rows.double(), B, Tq, H, dh), r_lse, B, Tq, H, dh, what)


@pytest.mark.gpu
@pytest.mark.parametrize('T', [1, 17, 64, 65, 130])
@pytest.mark.parametrize('dh', [32, 64])
def test_pos0_zero_over_the_packed_buffer_equals_the_causal_kernel_bit_for_bit(T, dh):
    from m3p_amd import ops
    B, H = 2, 4
    d = H * dh
    g = torch.Generator(device='cuda').manual_seed(3)
    qkv = torch.randn(B * T, 3 * d, device='cuda', generator=g).to(BF16)
    qkv[:, :d] = (qkv[:, :d].float() / np.sqrt(dh)).to(BF16)
    with poisoned_outputs():
        c_ctx, c_lse = ops.attn_causal_fwd(qkv, B, T, H, dh, seed=0, p_drop=0.0)
    kv = qkv.view(B, T, 3 * d)[:, :, d:]
    assert kv.stride(0) == T * 3 * d and kv.stride(1) == 3 * d
    ctx, lse = _prefix(qkv[:, :d], kv, B, T, H, dh, 0)
    assert_bits_equal(ctx, c_ctx, 'ctx at pos0 = 0, T = %d' % T)
    assert_bits_equal(lse, c_lse, 'lse at pos0 = 0, T = %d' % T)


@pytest.mark.gpu
def test_strided_cache_and_two_launches_give_the_same_bits():
    """The cache as a slice of a larger tensor with another pitch and batch stride, q as a column slice."""
    B, Tq, H, dh, pos0 = 2, 40, 4, 64, 30
    d, Lk = H * dh, pos0 + Tq
    q, kv, _, _ = _case(B, Tq, H, dh, pos0)
    first = _prefix(q, kv, B, Tq, H, dh, pos0)
    wide = torch.full((B * Tq, 3 * d), float('nan'), dtype=BF16, device='cuda')
    wide[:, d:2 * d] = q
    big = torch.full((B, Lk + 9, 2 * d + 16), float('nan'), dtype=BF16, device='cuda')
    big[:, :Lk, :2 * d] = kv[:, :Lk]
    second = _prefix(wide[:, d:2 * d], big[:, :, :2 * d], B, Tq, H, dh, pos0)
    for a, b, name in zip(second, first, ('ctx', 'lse')):
        assert_bits_equal(a, b, 'strided operands: ' + name)
    for a, b, name in zip(_prefix(q, kv, B, Tq, H, dh, pos0), first, ('ctx', 'lse')):
        assert_bits_equal(a, b, 'second launch: ' + name)


@pytest.mark.gpu
@pytest.mark.parametrize('B,Tq,H,dh,pos0', [(2, 40, 2, 48, 3), (1, 513, 2, 64, 0), (1, 8, 2, 64, 1017)])
def test_shapes_outside_the_prefix_kernel_are_declined(B, Tq, H, dh, pos0):
    """dh = 48, Tq = 513 and pos0 + Tq = 1025: None from the wrapper, the caller keeps the rows kernel."""
    from m3p_amd import ops
    d = H * dh
    q = torch.zeros((B * Tq, d), dtype=BF16, device='cuda')
    kv = torch.zeros((B, pos0 + Tq, 2 * d), dtype=BF16, device='cuda')
    assert ops.attn_prefix_fwd(q, kv, B, Tq, H, dh, pos0) is None
