"""Fault injection for the elementwise and per-row bounds of tests/util.py, on the CPU.

The GPU parity tests bound every element of a GEMM output and every row of an attention output with the helpers and bar
constants of tests/util.py.  Here the very same helpers and constants meet a clean restatement of a kernel's arithmetic -
the bf16 rounding of the exact product; attention with P and dS rounded to bf16 where the kernel feeds them to its matrix
products - which they must accept, and faults a kernel could make, which they must reject.  Each fault also passes the
global relative L2 bar the GPU tests applied alone before, at the size of the output they compare: that is why the bounds
exist.  If a bar is ever loosened until a fault slips through, these tests fail."""
import math

import pytest
import torch

from tests import util as U

M, N, K = 2048, 768, 768
GEMM_BENCH = 167936 * 3072          # the largest output test_gemm.py holds to the global bar (M = 167936, N = 3072)
B, S, H, DH = 2, 164, 4, 64
KEYLEN = torch.tensor([164, 101])
ATTN_BENCH = 256 * 164 * 768        # the benchmarked attention output (B = 256, S = 164, H x dh = 768)


def _bf16(x):
    return x.to(torch.bfloat16).double()


def _global_at(got, clean, ref, n_bench):
    """Global relative L2 error of ``got`` had the output n_bench elements whose other elements carry the clean rounding
    error: the fault's excess squared error stays, the reference's squared norm and the clean error grow with the size."""
    e_clean = float((clean - ref).pow(2).sum())
    e_fault = float((got - ref).pow(2).sum()) - e_clean
    return math.sqrt((e_clean + e_fault * ref.numel() / n_bench) / float(ref.pow(2).sum()))


@pytest.fixture(scope='module')
def gemm():
    g = torch.Generator().manual_seed(5)
    a = _bf16(torch.randn((M, K), generator=g, dtype=torch.float64))
    w = _bf16(torch.randn((N, K), generator=g, dtype=torch.float64) * 0.05)
    ref = a @ w.t()
    return a, w, ref, a.abs() @ w.abs().t(), _bf16(ref)


def test_gemm_bound_accepts_the_rounded_exact_product(gemm):
    a, w, ref, absref, clean = gemm
    worst = U.assert_gemm_bound(clean, ref, absref, K, U.BF16_OUT, what='bf16(exact product)')
    assert worst > 0.4                                      # (round-to-nearest reaches half of out_rounding)
    assert U.rel_l2(clean, ref) < U.GLOBAL_GEMM


@pytest.mark.parametrize('fault', ['zero_fragment', 'row_2_percent', 'tile_without_last_k_chunk', 'element_4_ulps'])
def test_gemm_bound_rejects_what_the_global_bar_lets_through(gemm, fault):
    a, w, ref, absref, clean = gemm
    c = clean.clone()
    if fault == 'zero_fragment':
        c[1040:1056, 320:336] = 0
        where = ('frag16', (65, 20))
    elif fault == 'row_2_percent':
        c[777] = _bf16(ref[777] * 1.02)
        where = ('row', 777)
    elif fault == 'tile_without_last_k_chunk':
        rows, cols = slice(512, 768), slice(256, 512)
        c[rows, cols] = _bf16(a[rows, :K - 32] @ w[cols, :K - 32].t())
        where = ('tile256', (2, 1))
    else:
        i, j = divmod(int(ref[:, :N // 2].abs().argmax()), N // 2)
        x = float(clean[i, j])
        c[i, j] = x + math.copysign(4 * 2.0 ** (math.floor(math.log2(abs(x))) - 7), x)
        where = ('row', i)
    assert _global_at(c, clean, ref, GEMM_BENCH) < U.GLOBAL_GEMM
    worst, at = U.gemm_bound(c, ref, absref, K, U.BF16_OUT)
    assert worst > 2.0 and at[where[0]] == where[1], (worst, at)
    with pytest.raises(AssertionError, match='elementwise bound'):
        U.assert_gemm_bound(c, ref, absref, K, U.BF16_OUT, what=fault)


def _attention(qkv, dctx, rounded):
    """fp64 attention forward and backward on a q-prescaled qkv [B*S, 3*H*dh] with keys >= KEYLEN[b] masked.  With
    ``rounded`` P and dS are rounded to bf16 where the kernel feeds them to its matrix products, D = rowsum(dO * O) is taken
    from the bf16 O, and the outputs are rounded to bf16 as the kernel stores them.  -> {ctx, dq, dk, dv} as [B, H, S, dh]
    (dq = the gradient of the prescaled q)."""
    r = _bf16 if rounded else (lambda t: t)
    q, k, v = qkv.view(B, S, 3, H, DH).permute(2, 0, 3, 1, 4)
    valid = torch.arange(S)[None, :] < KEYLEN[:, None]
    s = (q @ k.transpose(-1, -2)).masked_fill(~valid[:, None, None, :], float('-inf'))
    p = torch.exp(s - torch.logsumexp(s, -1, keepdim=True))
    p16 = r(p)
    ctx = p16 @ v
    do = dctx.view(B, S, H, DH).transpose(1, 2)
    dp = do @ v.transpose(-1, -2)
    ds = r(p * (dp - (do * r(ctx)).sum(-1, keepdim=True)))
    out = {'ctx': ctx, 'dq': ds @ k, 'dk': ds.transpose(-1, -2) @ q, 'dv': p16.transpose(-1, -2) @ do}
    return {n: r(t) for n, t in out.items()}


@pytest.fixture(scope='module')
def attention():
    g = torch.Generator().manual_seed(7)
    qkv = _bf16(torch.randn((B * S, 3 * H * DH), generator=g, dtype=torch.float64) * 0.7)
    dctx = _bf16(torch.randn((B * S, H * DH), generator=g, dtype=torch.float64))
    return _attention(qkv, dctx, False), _attention(qkv, dctx, True)


def _rtol(name):
    return U.ATTN_DS_RTOL if name in ('dq', 'dk') else U.ATTN_CTX_RTOL


def _floor(name):
    return U.ATTN_DS_FLOOR if name in ('dq', 'dk') else U.ROW_FLOOR


def _global_bar(name):
    return U.GLOBAL_ATTN_CTX if name == 'ctx' else U.GLOBAL_ATTN_GRAD


def test_row_bounds_accept_attention_with_bf16_operands(attention):
    exact, kern = attention
    for name in ('ctx', 'dq', 'dk', 'dv'):
        U.assert_block_bound(kern[name], exact[name], ('b', 'h', 'row'), _rtol(name), _floor(name), what=name)
        assert U.rel_l2(kern[name], exact[name]) < _global_bar(name), name
    for name in ('dk', 'dv'):
        U.assert_exact_zero(kern[name][1, :, int(KEYLEN[1]):], name + ' of masked keys')


@pytest.mark.parametrize('name', ['ctx', 'dv'])
def test_row_bounds_reject_one_head_3_percent_off(attention, name):
    exact, kern = attention
    got = kern[name].clone()
    got[1, 2] = _bf16(got[1, 2] * 1.03)
    assert _global_at(got, kern[name], exact[name], ATTN_BENCH) < _global_bar(name)
    worst, at, _ = U.block_bound(got, exact[name], ('b', 'h', 'row'), _rtol(name), _floor(name))
    assert worst > _rtol(name) and (at['b'], at['h']) == (1, 2), (worst, at)


def test_row_bounds_reject_the_last_20_query_rows_of_a_head_zeroed(attention):
    exact, kern = attention
    got = kern['dq'].clone()
    got[0, 1, S - 20:] = 0
    assert _global_at(got, kern['dq'], exact['dq'], ATTN_BENCH) < U.GLOBAL_ATTN_GRAD
    worst, at, _ = U.block_bound(got, exact['dq'], ('b', 'h', 'row'), U.ATTN_DS_RTOL, U.ATTN_DS_FLOOR)
    assert worst > 4 * U.ATTN_DS_RTOL and (at['b'], at['h']) == (0, 1) and at['row'] >= S - 20, (worst, at)


@pytest.mark.parametrize('name', ['dk', 'dv'])
def test_exact_zero_rejects_noise_in_the_rows_of_masked_keys(attention, name):
    exact, kern = attention
    got = kern[name].clone()
    kl = int(KEYLEN[1])
    noise = torch.randn(got[1, :, kl:].shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    got[1, :, kl:] += 1e-3 * noise
    assert _global_at(got, kern[name], exact[name], ATTN_BENCH) < U.GLOBAL_ATTN_GRAD
    with pytest.raises(AssertionError, match='exactly 0'):
        U.assert_exact_zero(got[1, :, kl:], name + ' of masked keys')


def test_bounds_count_nan_as_a_failure():
    ref = torch.ones((4, 4), dtype=torch.float64)
    got = ref.clone()
    got[2, 3] = float('nan')
    worst, at = U.gemm_bound(got, ref, ref, 4, U.BF16_OUT)
    assert worst == math.inf and (at['row'], at['col']) == (2, 3)
    assert U.block_bound(got, ref, ('row',), U.ROW_RTOL_BF16, U.ROW_FLOOR)[1] == {'row': 2}
    with pytest.raises(AssertionError):
        U.assert_exact_zero(torch.tensor([0.0, float('nan')]), 'nan')
