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


# ---------------------------------------------------------------------------------------------------------------------
# Streaming kernels: fused Adam update, sum of squares, elementwise bf16 functions, embedding rows.
# ---------------------------------------------------------------------------------------------------------------------
import numpy as np  # noqa: E402

F32 = np.float32
ADAM_GLOBAL_PM, ADAM_GLOBAL_V = 2e-6, 5e-6      # the rel_l2 bars of test_adam_step_matches_oracle
FAULT_QUAD = 2_000_001                          # the quad the Adam faults hit (elements 4 q .. 4 q + 3)


def _adam_f32(p, g, m, v, hp, swap=False, clip_v_once=False, no_wd=False):
    """adam_kernel of csrc/optim.hip restated in NumPy fp32, one rounding per operation in the kernel's order (no FMA).  The
    keyword faults are what the rejecting tests inject on one quad."""
    b1, b2, eps, lr = F32(hp['beta1']), F32(hp['beta2']), F32(hp['eps']), F32(hp['lr'])
    if swap:
        b1, b2 = b2, b1
    gs = F32(hp['grad_scale']) if hp['grad_scale'] else F32(1)
    coef = gs
    if hp.get('gnorm_sq') is not None and hp['max_norm'] > 0:
        norm = F32(math.sqrt(hp['gnorm_sq'])) * gs
        c = F32(hp['max_norm']) / (norm + F32(1e-6))
        coef = coef * (c if c < 1 else F32(1))
    ob1, ob2 = F32(1) - b1, F32(1) - b2
    wdl = F32(0) if no_wd else F32(hp['weight_decay']) * lr
    gc = g * coef
    mn = m * b1 + gc * ob1
    vn = v * b2 + (gc * (g * gs if clip_v_once else gc)) * ob2
    den = np.sqrt(vn) + eps
    pn = p - wdl * p if wdl != 0 else p
    pn = pn - F32(hp['step_size']) * (mn / den)
    assert pn.dtype == mn.dtype == vn.dtype == F32
    return pn, mn, vn


def _adam_state(n, seed, zeros=True):
    """Gradient scales 1e-4 .. 30 and second moments 1e-10 .. 1, log-uniform per element, with zero g, m, v entries."""
    rs = np.random.RandomState(seed)
    gscale = 10.0 ** rs.uniform(-4, math.log10(30), n)
    p = rs.standard_normal(n).astype(F32)
    g = (gscale * rs.standard_normal(n)).astype(F32)
    m = (0.5 * gscale * rs.standard_normal(n)).astype(F32)
    v = (10.0 ** rs.uniform(-10, 0, n)).astype(F32)
    if zeros:
        for k, a in enumerate((g, m, v)):
            a[rs.randint(0, n, n // 64)] = 0
            a[1000 * (k + 1):1000 * (k + 1) + 64] = 0
        g[5000:5064] = 0; m[5000:5064] = 0; v[5000:5064] = 0          # all three at once: the update is 0 / eps
    return p, g, m, v


def _hp(g, clip, wd, grad_scale=1.0, step=3):
    gn = float((g.astype(np.float64) ** 2).sum())
    b1, b2, lr = 0.9, 0.98, 1e-2
    return dict(lr=lr, beta1=b1, beta2=b2, eps=1e-8, weight_decay=wd, step_size=lr * math.sqrt(1 - b2 ** step) / (1 - b1 ** step),
                gnorm_sq=gn, max_norm=(0.5 if clip else 2.0) * math.sqrt(gn) * grad_scale, grad_scale=grad_scale)


def _t(*arrays):
    return tuple(torch.from_numpy(a) for a in arrays)


@pytest.mark.parametrize('clip', [True, False])
@pytest.mark.parametrize('wd', [0.0, 0.01])
def test_adam_bound_accepts_the_fp32_restatement(clip, wd):
    """4 M elements.  The restatement reaches 2.4 u (m), 3.7 u (v) and 5.1 u (p) of the 8, 12 and 16 u of the bounds."""
    state = _adam_state(1 << 22, 11 + clip + 2 * (wd > 0))
    hp = _hp(state[1], clip, wd, grad_scale=0.5 if clip else 1.0)
    out = _adam_f32(*state, hp)
    worst = U.assert_adam_bound(_t(*out), _t(*state), hp, what='fp32 restatement')
    assert worst['m'] > 0.15 and worst['v'] > 0.15 and worst['p'] > 0.15, worst       # (the bounds are not vacuous)


@pytest.fixture(scope='module')
def adam12m():
    n = 12 << 20
    state = _adam_state(n, 5, zeros=False)
    q = slice(4 * FAULT_QUAD, 4 * FAULT_QUAD + 4)
    # the faulted quad belongs to a parameter with small gradients and moments: its errors vanish in a global norm that
    # the parameters with large ones dominate
    state[1][q] = F32(1e-3) * np.array([1.0, -2.0, 0.5, 3.0], dtype=F32)
    state[2][q] = F32(1e-3) * np.array([-0.7, 1.5, 2.0, -0.4], dtype=F32)
    state[3][q] = F32(1e-4) * np.array([1.0, 0.3, 2.0, 0.8], dtype=F32)
    hp = _hp(state[1], True, 0.01)
    clean = _adam_f32(*state, hp)
    refs, _ = U.adam_ref64(*_t(*state), hp)
    return state, hp, clean, refs


@pytest.mark.parametrize('fault', ['quad_not_updated', 'quad_updated_twice', 'betas_swapped', 'clip_once_in_v', 'no_weight_decay'])
def test_adam_bound_rejects_one_wrong_quad_in_12m_elements(adam12m, fault):
    state, hp, clean, refs = adam12m
    q = slice(4 * FAULT_QUAD, 4 * FAULT_QUAD + 4)
    got = [a.copy() for a in clean]
    before = [a[q] for a in state]
    if fault == 'quad_not_updated':
        new = (before[0], before[2], before[3])
    elif fault == 'quad_updated_twice':
        once = _adam_f32(*before, hp)
        new = _adam_f32(once[0], before[1], once[1], once[2], hp)
    elif fault == 'betas_swapped':
        new = _adam_f32(*before, hp, swap=True)
    elif fault == 'clip_once_in_v':
        new = _adam_f32(*before, hp, clip_v_once=True)
    else:
        new = _adam_f32(*before, hp, no_wd=True)
    for a, x in zip(got, new):
        a[q] = x
    for a, ref, bar in zip(got, refs, (ADAM_GLOBAL_PM, ADAM_GLOBAL_PM, ADAM_GLOBAL_V)):
        assert U.rel_l2(torch.from_numpy(a), ref) < bar                 # the present global bars let it through
    worst = U.adam_bound(_t(*got), _t(*state), hp)
    w, at = max(worst.values())
    assert w > 2.0 and at // 4 == FAULT_QUAD, worst
    with pytest.raises(AssertionError, match='quad %d' % FAULT_QUAD):
        U.assert_adam_bound(_t(*got), _t(*state), hp, what=fault)


def test_adam_bound_wants_exact_zeros_where_every_term_is_zero():
    z = np.zeros(8, dtype=F32)
    p = np.ones(8, dtype=F32)
    hp = _hp(np.ones(8, dtype=F32), False, 0.0)
    assert max(w for w, _ in U.adam_bound(_t(p, z, z), _t(p, z, z, z), hp).values()) == 0.0
    m = z.copy(); m[5] = 1e-30
    assert U.adam_bound(_t(p, m, z), _t(p, z, z, z), hp)['m'] == (math.inf, 5)


SUMSQ_MAXBLK, SUMSQ_QUADS_PER_BLOCK = 2048, 1024      # m3p_sumsq_f32: blocks = clamp(ceil(n4 / 1024), 1, 2048) of 256 threads


def _sumsq_f32(x, threads, skip_quad=None, drop_tail=False):
    """sumsq_kernel restated: thread k adds the quads k, k + threads, ... in fp32, each quad as (a^2 + b^2) + (c^2 + d^2); a
    butterfly over the 64 lanes of a wave in fp32; the waves in fp64.  Faults: one quad skipped; the quads the 4 x unrolled
    loop leaves to the tail loop dropped."""
    sq = x.reshape(-1, 4) * x.reshape(-1, 4)
    quad = (sq[:, 0] + sq[:, 1]) + (sq[:, 2] + sq[:, 3])
    n4 = quad.size
    if skip_quad is not None:
        quad[skip_quad] = 0
    t = -(-n4 // threads)
    if drop_tail:
        quad[(n4 // (4 * threads)) * 4 * threads:] = 0
    quad = np.concatenate([quad, np.zeros(t * threads - n4, dtype=F32)]).reshape(t, threads)
    acc = np.zeros(threads, dtype=F32)
    for row in quad:
        acc = acc + row
    acc = acc.reshape(-1, 64)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ o]
    assert acc.dtype == F32
    return float(acc[:, 0].astype(np.float64).sum()), t


def _sumsq_threads(n4):
    return 256 * min(max(-(-n4 // SUMSQ_QUADS_PER_BLOCK), 1), SUMSQ_MAXBLK)


@pytest.mark.parametrize('n4,threads', [(3 * SUMSQ_MAXBLK * 256 * 4 + 77, None), (256 * 2000 + 3, 256), (1, None)])
def test_sumsq_bound_accepts_the_fp32_restatement(n4, threads):
    """At the launcher's grid (t = 13) and with one block walking 2001 quads per thread: the bound is linear in t."""
    x = (np.random.RandomState(n4 % 1000).standard_normal(4 * n4) * 3).astype(F32)
    got, t = _sumsq_f32(x, threads or _sumsq_threads(n4))
    U.assert_sumsq_bound(got, float((x.astype(np.float64) ** 2).sum()), t, what='fp32 restatement')


def test_sumsq_bound_rejects_a_skipped_quad_and_a_dropped_tail():
    n4 = SUMSQ_MAXBLK * 256 * 4                        # t = 4: every thread of the full grid runs the unrolled loop once
    x = np.random.RandomState(3).standard_normal(4 * n4).astype(F32)
    x[4 * 777_777 + 2] = 3.5                           # one large gradient element: 12 of a sum of 8.4 M
    ref = float((x.astype(np.float64) ** 2).sum())
    got, t = _sumsq_f32(x, _sumsq_threads(n4), skip_quad=777_777)
    assert t == 4 and abs(math.sqrt(got) - math.sqrt(ref)) < 1e-6 * math.sqrt(ref)      # the present bar (on the norm) lets it through
    assert U.sumsq_bound(got, ref, t) > 1.5
    with pytest.raises(AssertionError, match='sum of squares'):
        U.assert_sumsq_bound(got, ref, t, what='skipped quad')
    n4 = 3 * SUMSQ_MAXBLK * 256 * 4 + 77               # the unrolled loop three times, then 77 quads for the tail loop
    x = np.random.RandomState(4).standard_normal(4 * n4).astype(F32)
    got, t = _sumsq_f32(x, _sumsq_threads(n4), drop_tail=True)
    assert t == 13 and U.sumsq_bound(got, float((x.astype(np.float64) ** 2).sum()), t) > 5.0
    assert U.sumsq_bound(float('nan'), 1.0, 4) == math.inf


# --- rows of the embedding assembly ------------------------------------------------------------------------------------
EMB_B, EMB_S, EMB_R, EMB_D = 64, 40, 12, 768
EMBED_GLOBAL_H, EMBED_GLOBAL_GRAD = 6e-3, 1.5e-2        # the rel_l2 bars of test_embed_assemble_fwd_bwd
EMBED_BENCH_ROWS = 256 * 164                            # rows of h at the benchmarked size; de has 36 x 256


def _ln(x, g, b):
    mu = x.mean(-1, keepdim=True)
    rs = 1.0 / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + 1e-12)
    return (x - mu) * rs * g + b, (x - mu) * rs, rs


def _ln_bwd(dy, g, xh, rs):
    gd = dy * g
    return (gd - gd.mean(-1, keepdim=True) - xh * (gd * xh).mean(-1, keepdim=True)) * rs


@pytest.fixture(scope='module')
def embed_rows():
    """h = LN_emb(z) from a bf16 z, and de = LN_img backward of the image rows of dz = LN_emb backward of dh: exact in fp64,
    and restated with the roundings the kernels make (fp32 arithmetic, h and de stored in bf16, dz stored in bf16 between
    the two backward kernels)."""
    gen = torch.Generator().manual_seed(9)
    rnd = lambda *s: torch.randn(s, generator=gen, dtype=torch.float64)      # noqa: E731
    z, e, dh = _bf16(rnd(EMB_B, EMB_S, EMB_D) * 0.6), _bf16(rnd(EMB_B, EMB_R, EMB_D)), _bf16(rnd(EMB_B, EMB_S, EMB_D))
    g_emb, be_emb, g_img = (1 + 0.1 * rnd(EMB_D)).float().double(), (0.1 * rnd(EMB_D)).float().double(), (1 + 0.1 * rnd(EMB_D)).float().double()
    out = {}
    for name, f in (('exact', lambda t: t), ('kernel', lambda t: t.float().double())):
        h, xh, rs = _ln(z, g_emb, be_emb)
        dz = f(_ln_bwd(dh, g_emb, f(xh), f(rs)))
        _, xh_i, rs_i = _ln(e, g_img, 0.0)
        if name == 'kernel':
            h, dz = _bf16(f(h)), _bf16(dz)
        de = _ln_bwd(dz[:, :EMB_R], g_img, f(xh_i), f(rs_i))
        out[name] = dict(h=h, dz=dz, de=_bf16(f(de)) if name == 'kernel' else de)
    return out


def test_row_bounds_accept_the_embedding_rows_with_their_roundings(embed_rows):
    """One bf16 rounding (h) reaches 0.48 of ROW_RTOL_BF16 on these 2560 rows, two with a LayerNorm backward between them
    (de) 0.68 on 768 rows: the bar of de is sqrt(2) ROW_RTOL_BF16."""
    exact, kern = embed_rows['exact'], embed_rows['kernel']
    h = U.assert_block_bound(kern['h'], exact['h'], ('b', 's'), U.ROW_RTOL_BF16, U.ROW_FLOOR, 'h')
    de = U.assert_block_bound(kern['de'], exact['de'], ('b', 'r'), U.EMBED_DE_RTOL, U.ROW_FLOOR, 'de')
    assert 0.4 * U.ROW_RTOL_BF16 < h < 0.6 * U.ROW_RTOL_BF16 and 0.45 * U.EMBED_DE_RTOL < de, (h, de)     # about 2 x room


@pytest.mark.parametrize('fault', ['row_without_its_last_64_columns', 'row_2_percent', 'last_sequence_unwritten'])
def test_row_bounds_reject_wrong_embedding_rows(embed_rows, fault):
    exact, kern = embed_rows['exact'], embed_rows['kernel']
    for name, rtol, bar, n_bench in (('h', U.ROW_RTOL_BF16, EMBED_GLOBAL_H, EMBED_BENCH_ROWS), ('de', U.EMBED_DE_RTOL, EMBED_GLOBAL_GRAD, 36 * 256)):
        got = kern[name].clone()
        if fault == 'row_without_its_last_64_columns':
            got[EMB_B - 1, 3, -64:] = 0
        elif fault == 'row_2_percent':
            got[EMB_B - 1, 3] = _bf16(got[EMB_B - 1, 3] * 1.02)
        else:
            got[EMB_B - 1] = float('nan')                  # what a poisoned output reads where a batch slice stopped early
        if fault != 'last_sequence_unwritten':
            assert _global_at(got, kern[name], exact[name], n_bench * EMB_D) < bar
        worst, at, _ = U.block_bound(got, exact[name], ('b', 'row'), rtol, U.ROW_FLOOR)
        assert worst > 2 * rtol and at['b'] == EMB_B - 1, (name, worst, at)


def test_accum_bound_on_sums_gathered_in_any_order():
    """d_pos-like sums of B fp32 terms: an fp32 sum in a shuffled order passes; one lost term of 256 fails although the global
    bar of the gradient tests lets it through."""
    gen = torch.Generator().manual_seed(4)
    terms = torch.randn((256, 40, 64), generator=gen).double()           # fp32 values
    ref, absref = terms.sum(0), terms.abs().sum(0)
    acc = torch.zeros((40, 64))
    for b in torch.randperm(256, generator=gen).tolist():
        acc = acc + terms[b].float()
    worst, _ = U.accum_bound(acc, ref, absref, 256)
    assert worst < 0.5
    lost = acc.clone()
    lost[17] = (ref[17] - terms[255, 17]).float()
    assert U.rel_l2(lost, ref) < EMBED_GLOBAL_GRAD
    worst, at = U.accum_bound(lost, ref, absref, 256)
    assert worst > 100 and at['row'] == 17
    with pytest.raises(AssertionError, match='accumulation bound at row 17'):
        U.assert_accum_bound(lost, ref, absref, 256, what='lost term')
    n = torch.tensor([[1.0]] * 20 + [[256.0]] * 20, dtype=torch.float64)      # rows that gather different numbers of terms
    assert U.accum_bound(acc, ref, absref, n)[0] > worst * 0 and U.accum_bound(acc, ref, absref, n)[1]['row'] < 20


# --- elementwise bf16 kernels -----------------------------------------------------------------------------------------
GELU_BENCH = 41984 * 3072            # elements of the benchmarked GELU call
GELU_GLOBAL = 4e-3                   # the rel_l2 bar of test_gelu_fwd_and_batched_transpose


def _gelu_parts_f32(x):
    """gelu_parts of csrc/common.hpp in NumPy fp32 (IEEE division and libm exp where the kernel has v_rcp_f32 / v_exp_f32)."""
    z = np.abs(x) * F32(0.70710678118654752440)
    t = F32(1) / (F32(1) + F32(0.3275911) * z)
    with np.errstate(over="ignore"):
        e = np.exp(-z * z)
    poly = F32(1.061405429)
    for c in (-1.453152027, 1.421413741, -0.284496736, 0.254829592):
        poly = poly * t + F32(c)
    cdf_abs = F32(0.5) + F32(0.5) * (F32(1) - poly * t * e)
    cdf = np.where(x >= 0, cdf_abs, F32(1) - cdf_abs)
    assert cdf.dtype == F32
    return cdf, F32(0.39894228040143267794) * e


@pytest.fixture(scope='module')
def gelu():
    rs = np.random.RandomState(8)
    x = torch.from_numpy((rs.standard_normal(1 << 20) * 2).astype(F32)).to(torch.bfloat16)
    x[:10] = torch.tensor([0.0, -0.0, 2.0 ** -20, -2.0 ** -20, 8.0, -8.0, 40.0, -40.0, 3.3895313892515355e38, -3.3895313892515355e38])
    cdf, pdf = _gelu_parts_f32(x.float().numpy())
    xf = x.float().numpy()
    with np.errstate(over='ignore', invalid='ignore'):
        h, dh = torch.from_numpy(xf * cdf).to(torch.bfloat16), torch.from_numpy(cdf + xf * pdf).to(torch.bfloat16)
    x64 = x.double()
    return x64, h, dh, U._gelu64(x, 'cpu'), U._dgelu64(x, 'cpu')


def test_elementwise_bound_accepts_the_fp32_gelu(gelu):
    x, h, dh, ref, dref = gelu
    zero = torch.zeros_like(ref)
    U.assert_gemm_bound(h, ref, zero, 0, U.BF16_OUT, 2 * U.EPS_ERF * x.abs(), what='gelu')
    U.assert_gemm_bound(dh, dref, zero, 0, U.BF16_OUT, U.EPS_DGELU, what="gelu'")


@pytest.mark.parametrize('fault', ['two_bf16_ulps', 'eight_elements_unwritten', 'eight_elements_of_the_neighbour'])
def test_elementwise_bound_rejects_what_the_global_bar_lets_through(gelu, fault):
    x, h, dh, ref, dref = gelu
    got = h.double()
    i = 8 * 5000
    if fault == 'two_bf16_ulps':
        i = int(ref.abs().argmax())
        got[i] = float(got[i]) * (1 + 2 * 2.0 ** -7)
    elif fault == 'eight_elements_unwritten':
        got[i:i + 8] = 0                    # (what the allocator handed back; under poisoned_outputs() it reads NaN)
    else:
        got[i:i + 8] = got[i + 8:i + 16]
    assert _global_at(got, h.double(), ref, GELU_BENCH) < GELU_GLOBAL
    worst, at = U.gemm_bound(got, ref, torch.zeros_like(ref), 0, U.BF16_OUT, 2 * U.EPS_ERF * x.abs())
    assert worst > 1.5 and i <= at['row'] < i + 8, (worst, at)


def test_glu_terms_hold_the_fp32_restatement():
    """The fp32 restatement reaches 0.50 (y, da) and 0.31 (db) of the approximation terms alone (no output rounding), and
    stays inside the whole bound once its outputs are rounded to bf16."""
    rs = np.random.RandomState(12)
    bf = lambda a: torch.from_numpy(a.astype(F32)).to(torch.bfloat16)      # noqa: E731
    a, b, g = bf(rs.standard_normal(1 << 20) * 1.5), bf(rs.standard_normal(1 << 20) * 3), bf(rs.standard_normal(1 << 20))
    b[:6] = torch.tensor([0.0, 20.0, -20.0, 60.0, -60.0, 9.0])
    an, bn, gn = (t.float().numpy() for t in (a, b, g))
    s = F32(1) / (F32(1) + np.exp(-bn))
    y, da, db = an * s, gn * s, gn * an * s * (F32(1) - s)
    assert db.dtype == F32
    a64, b64, g64 = a.double(), b.double(), g.double()
    s64 = torch.sigmoid(b64)
    refs = (a64 * s64, g64 * s64, g64 * a64 * s64 * (1 - s64))
    eps = (U.glu_eps(a, b),) + U.glu_eps(a, b, g)
    zero = torch.zeros_like(a64)
    reached = 0.0
    for got, ref, e in zip((y, da, db), refs, eps):
        got = torch.from_numpy(got)
        reached = max(reached, U.gemm_bound(got, ref, zero, 0, 0.0, e)[0])
        U.assert_gemm_bound(got.to(torch.bfloat16), ref, zero, 0, U.BF16_OUT, e, what='glu')
    assert 0.45 < reached <= 1.0, reached                  # (2 x room)


# --- the row kernels behind the shifted-exponential MLM head (csrc/heads.hip: ce_shift_*) -----------------------------------
MODEL_LOSS_BAR, MODEL_GRAD_BAR = 5e-3, 5e-2     # the model-level bars of tests/test_model_parity.py: |loss|, rel_l2 of a gradient
SHIFT_MAXBLK = 2048                             # ce_shift_blocks: at most 2048 blocks of 256 threads, one 4-element chunk each


def _shift_rows_f32(stats, gs, drop_partial=None, drop_tail=False):
    """ce_shift_partial_kernel and ce_shift_final_kernel restated in NumPy fp32, one rounding per operation in the kernels'
    order: the blocks of a row in 32 splits; in a split four waves take every fourth block, four at a time into four
    accumulators while `b + 12 < b1`, the rest one by one into the first; (s0 + s1) + (s2 + s3), the four waves folded the
    same way, the 32 partial sums one after the other.  Faults: the partial sum (split, row) dropped; the blocks the unrolled
    loop leaves to the tail loop dropped."""
    n_blocks, n = stats.shape
    per = -(-n_blocks // U.CE_LSE_SPLIT)
    total = np.zeros(n, dtype=F32)
    for k in range(U.CE_LSE_SPLIT):
        b0, b1 = k * per, min(n_blocks, k * per + per)
        sh = []
        for q in range(4):
            s = [np.zeros(n, dtype=F32) for _ in range(4)]
            b = b0 + q
            while b + 12 < b1:
                for j in range(4):
                    s[j] = s[j] + stats[b + 4 * j]
                b += 16
            while b < b1:
                if not drop_tail:
                    s[0] = s[0] + stats[b]
                b += 4
            sh.append((s[0] + s[1]) + (s[2] + s[3]))
        part = (sh[0] + sh[1]) + (sh[2] + sh[3])
        if drop_partial is not None and drop_partial[0] == k:
            part[drop_partial[1]] = 0
        total = total + part
    gs = F32(gs)
    with np.errstate(over='ignore'):
        e0 = np.exp(F32(-U.CE_SHIFT))
        sigma = total + e0
        r = total * np.exp(F32(U.CE_SHIFT))
        loss2 = F32(U.CE_SHIFT) + np.log(sigma)
        loss = np.where(total < e0, np.log1p(r), loss2)
        q = np.where(total < e0, -gs * r / (F32(1) + r), gs * np.expm1(-loss2))
        s = gs / sigma
    assert total.dtype == loss.dtype == q.dtype == s.dtype == F32
    return loss, s, q


def _shift_stats(n_blocks, n, seed):
    """The synthetic block sums of tests/test_mlm_head_kernels.py: row n sums to e^-40 r_n, log r_n spread over [-30, 30]."""
    rs = np.random.RandomState(seed)
    raw = np.exp(rs.uniform(-2.0, 2.0, (n_blocks, n)))
    logr = rs.permutation(np.linspace(-30.0, 30.0, n))
    return (raw / raw.sum(0) * np.exp(logr - U.CE_SHIFT)).astype(F32), logr


@pytest.mark.parametrize('n_blocks', [1, 33, 416, 547, 3907])
def test_shift_rows_bound_accepts_the_fp32_restatement(n_blocks):
    stats, _ = _shift_stats(n_blocks, 64, n_blocks)
    loss, s, q = _shift_rows_f32(stats, 1.0 / 64)
    worst = U.assert_shift_rows_bound(*_t(loss, s, q, stats), 1.0 / 64, what='fp32 restatement')
    print('fp32 restatement of the row statistics at %d blocks: %s of the bounds' % (n_blocks, worst))
    assert max(worst.values()) <= 0.5                       # (2 x room: libm's functions against the device's)
    assert U.shift_rowsum_adds(n_blocks) == {1: 37, 33: 37, 416: 40, 547: 41, 3907: 67}[n_blocks]


@pytest.mark.parametrize('fault', ['partial_dropped', 'tail_dropped'])
def test_shift_rows_bound_rejects_lost_block_sums(fault):
    """One of a row's 32 partial sums lost - on a confident row (r = e^-20: the loss itself is below every absolute bar, only q,
    held relative to itself, shows it) and on a hopeless one - and the blocks behind the unrolled loop lost (547 blocks: 2 of
    every split's 18).  The mean loss over the 64 rows, the model-level check, moves by less than its bar."""
    n_blocks = 547
    stats, logr = _shift_stats(n_blocks, 64, 5)
    clean = _shift_rows_f32(stats, 1.0 / 64)
    ref = U.shift_rows_ref64(torch.from_numpy(stats), 1.0 / 64)
    if fault == 'tail_dropped':
        got = _shift_rows_f32(stats, 1.0 / 64, drop_tail=True)
        worst = U.shift_rows_bound(*_t(*got, stats), 1.0 / 64)
        assert worst['loss'][0] > 100 and worst['q'][0] > 100 and worst['s'][0] > 100, worst
        return
    for row in (int(np.argmin(np.abs(logr + 20))), int(np.argmax(logr))):
        got = _shift_rows_f32(stats, 1.0 / 64, drop_partial=(5, row))
        assert abs(float(got[0].astype(np.float64).mean()) - float(ref[1].mean())) < MODEL_LOSS_BAR
        worst = U.shift_rows_bound(*_t(*got, stats), 1.0 / 64)
        if logr[row] > 0:      # r = e^30: the loss and s move by 3 per cent of the sum; q = -gs (1 - e^-30) does not notice
            key = 'loss'
            assert worst['loss'][0] > 100 and worst['loss'][1] == row and worst['s'][0] > 100 and worst['s'][1] == row, (row, worst)
        else:                  # r = e^-20: loss ~ r is far below its absolute bound, s = gs / (sum + e^-40) barely moves: only q tells
            key = 'q'
            assert worst['q'][0] > 100 and worst['q'][1] == row, (row, worst)
            assert worst['loss'][0] <= 1.0 and abs(float(got[0][row]) - float(clean[0][row])) < 1e-9
        with pytest.raises(AssertionError, match='%s of row %d' % (key, row)):
            U.assert_shift_rows_bound(*_t(*got, stats), 1.0 / 64, what='lost partial')


def _bf16_t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(torch.bfloat16)


@pytest.fixture(scope='module')
def shift_rows_case():
    """(n, d) = (2112, 1024): 540 672 chunks of four, past the 524 288 one trip of the capped grid covers.  The fp32
    restatements of ce_shift_scale_rows_kernel, bf16(h (g s)), and of ce_shift_dh_kernel, bf16((dh32 s + E[y] q) g)."""
    n, d = 2112, 1024
    rs = np.random.RandomState(21)
    h = _bf16_t(rs.standard_normal((n, d))).float().numpy()
    dh32 = (rs.standard_normal((n, d)) * 3).astype(F32)
    ey = _bf16_t(rs.standard_normal((n, d)) * 0.7).float().numpy()
    s, q, g = (rs.standard_normal(n) * 2).astype(F32), rs.standard_normal(n).astype(F32), F32(0.5)
    scaled = h * (g * s)[:, None]
    dh = (dh32 * s[:, None] + ey * q[:, None]) * g
    assert scaled.dtype == dh.dtype == F32 and n * d // 4 > SHIFT_MAXBLK * 256
    return dict(h=h, dh32=dh32, ey=ey, s=s, q=q, scaled=scaled, dh=dh)


def _row_bounds(c, scaled, dh):
    h, dh32, ey, s, q = _t(c['h'], c['dh32'], c['ey'], c['s'], c['q'])
    return U.scale_rows_bound(scaled, h, s, 0.5), U.shift_dh_bound(dh, dh32, ey, s, q, 0.5)


def test_row_scaled_bounds_accept_the_fp32_restatement(shift_rows_case):
    c = shift_rows_case
    (ws, _), (wd, _) = _row_bounds(c, _bf16_t(c['scaled']), _bf16_t(c['dh']))
    print('fp32 restatement of scale_rows / dh: %.3f / %.3f of the bounds' % (ws, wd))
    # BF16_OUT is bf16's unit roundoff: over 2 M elements round-to-nearest comes within a per cent of it, just above a power of
    # two.  The fp32 evaluation before it (two roundings for scale_rows, at most four for dh) stays inside the F32_OUT term, so
    # the bound holds for every input, with no room to spare and none needed.
    assert 0.9 < ws <= 1.0 and 0.9 < wd <= 1.0


@pytest.mark.parametrize('fault', ['neighbours_s', 'second_trip_unwritten'])
def test_row_scaled_bounds_reject_a_wrong_row_and_an_unwritten_trip(shift_rows_case, fault):
    c = shift_rows_case
    scaled, dh = c['scaled'].copy(), c['dh'].copy()
    s = c['s']
    if fault == 'neighbours_s':
        rel = np.abs(s[1:] - s[:-1]) / np.abs(s[:-1])
        row = int(np.nonzero((rel > 0.02) & (rel < 0.1))[0][0])           # a neighbour 2 .. 10 per cent away
        scaled[row] = c['h'][row] * (F32(0.5) * s[row + 1])
        dh[row] = (c['dh32'][row] * s[row + 1] + c['ey'][row] * c['q'][row]) * F32(0.5)
        for got, clean in ((scaled, c['scaled']), (dh, c['dh'])):            # the model-level bar lets both through
            assert U.rel_l2(_bf16_t(got).double(), torch.from_numpy(clean).double()) < MODEL_GRAD_BAR
        first = (row, row)
    else:
        start = 4 * SHIFT_MAXBLK * 256                                     # what a poisoned output reads past the first trip
        scaled.reshape(-1)[start:] = np.nan
        dh.reshape(-1)[start:] = np.nan
        first = (start // 1024, start // 1024)
    (ws, at_s), (wd, at_d) = _row_bounds(c, _bf16_t(scaled), _bf16_t(dh))
    assert ws > 4 and wd > 4 and (at_s['row'], at_d['row']) == first, (ws, at_s, wd, at_d)


def _target_rows_f32(h, y, q, g, demb0, dbias0, order, once=None):
    """ce_shift_target_rows_kernel restated: row by row in the given order, demb[y] += (g q) h and dbias[y] += g q in fp32.
    Fault: of the rows that name word `once`, only the first adds."""
    demb, dbias = demb0.copy(), dbias0.copy()
    seen = False
    for r in order:
        if y[r] == once:
            if seen:
                continue
            seen = True
        c = F32(g) * q[r]
        v = c * h[r]
        demb[y[r]] = demb[y[r]] + v
        dbias[y[r]] = dbias[y[r]] + c
    assert demb.dtype == dbias.dtype == F32
    return demb, dbias


def test_target_rows_bound_accepts_any_order_and_rejects_a_lost_repeat():
    """257 rows of width 68 over ten words and over one: the fp32 sums in two shuffled orders pass; a word named k times that
    receives one of its k terms fails, on its own row and entry."""
    n, d, V = 257, 68, 268
    rs = np.random.RandomState(31)
    h = _bf16_t(rs.standard_normal((n, d))).float().numpy()
    q = rs.standard_normal(n).astype(F32)
    q[::5] = 0
    demb0, dbias0 = rs.standard_normal((V, d)).astype(F32), rs.standard_normal(V).astype(F32)
    words = np.array([0, V - 1, 3, 4, 5, 6, 7, V // 2, V - 3, V - 2])
    for y in (words[rs.randint(0, 10, n)], np.full(n, 5)):
        args = _t(demb0, dbias0, h) + (torch.from_numpy(y),) + _t(q)
        for seed in (1, 2):
            demb, dbias = _target_rows_f32(h, y, q, 0.5, demb0, dbias0, np.random.RandomState(seed).permutation(n))
            (we, _), (wb, _) = U.target_rows_bound(*_t(demb, dbias), *args, 0.5)
            assert we <= 0.5 and wb <= 0.5, (we, wb)
            unnamed = np.bincount(y, minlength=V) == 0
            assert np.array_equal(demb[unnamed].view(np.int32), demb0[unnamed].view(np.int32))
        word = int(y[1])
        k = int((y == word).sum())
        assert k > 10
        demb, dbias = _target_rows_f32(h, y, q, 0.5, demb0, dbias0, np.arange(n), once=word)
        (we, at_e), (wb, at_b) = U.target_rows_bound(*_t(demb, dbias), *args, 0.5)
        assert we > 100 and wb > 100 and at_e['row'] == word and at_b['row'] == word, (we, at_e, wb, at_b)


# --- the MLM head where it stores its logits in bf16 -------------------------------------------------------------------------
def _head_in_place_f64(H, E, b, y, g_up, round_logits=True, lose_row=None):
    """The head's path that stores the logits in bf16 and rewrites them into their gradient (ce_fwd_bwd, ce_fwd_bwd_colsum,
    ce_from_block_stats), restated in fp64 with nothing but its bf16 roundings: the stored logits, the gradient written over
    them, the hidden rows times the upstream gradient, the data gradient.  Fault: one row left out of the weight gradient."""
    n = H.shape[0]
    rows = torch.arange(n)
    x = H.double() @ E.double().t() + b.double()
    if round_logits:
        x = _bf16(x)
    lse = torch.logsumexp(x, 1)
    G = torch.exp(x - lse[:, None])
    G[rows, y] -= 1.0
    G = _bf16(G / n)
    hs = _bf16(H.double() * g_up)
    dH = _bf16(g_up * (G @ E.double()))
    db = g_up * G.sum(0)
    if lose_row is not None:
        G = G.clone()
        G[lose_row] = 0
    return float((lse - x[rows, y]).mean()), dH, G.t() @ hs, db


def test_head_bounds_need_the_stored_logits_rounding_below_4096_rows():
    """Why tests/test_mlm_shifted_gpu.py counts the rounding of the stored logits in dE below 4096 rows.  At n = 1024 (d = 256,
    V = 5000, the bands' head) the restatement with exact logits stays inside the bounds of the 4096-row head; with the logits
    rounded to bf16 - no fault - it reaches 1.80 of the bound of dE, which models one rounding of G and none in its exponent;
    with that rounding counted it is inside again, and a row left out of the weight gradient, which the model-level bar on the
    whole matrix lets through, is still rejected."""
    import types
    from tests.test_mlm_shifted_gpu import _distances, _reference
    n, d, V, g_up = 1024, 256, 5000, 0.5
    g = torch.Generator().manual_seed(11)
    E = (torch.randn((V, d), generator=g) * (1.2 / math.sqrt(d))).to(torch.bfloat16).float()
    b = torch.randn((V,), generator=g) * 0.5
    H = torch.randn((n, d), generator=g).to(torch.bfloat16)
    y = torch.randint(0, V, (n,), generator=g)
    ref = _reference(H, E, b, y, g_up)
    head = types.SimpleNamespace(n=n)
    exact = _distances(head, _head_in_place_f64(H, E, b, y, g_up, round_logits=False), ref)
    assert max(exact.values()) <= 0.6, exact
    got = _head_in_place_f64(H, E, b, y, g_up)
    plain, counted = _distances(head, got, ref), _distances(head, got, ref, stored_logits=True)
    print('restatement at n = 1024: exact logits %s; stored logits %s; with their rounding counted dE %.3g' % (exact, plain, counted['dE']))
    assert 1.5 < plain['dE'] < 2.1 and max(plain[k] for k in ('loss', 'dH', 'db')) <= 1.0, plain
    assert counted['dE'] <= 0.6 and all(counted[k] == plain[k] for k in ('loss', 'dH', 'db')), counted
    lost = _head_in_place_f64(H, E, b, y, g_up, lose_row=700)
    assert U.rel_l2(lost[2], ref['dE']) < MODEL_GRAD_BAR
    assert _distances(head, lost, ref, stored_logits=True)['dE'] > 20


# --- column gradients of LayerNorm ---------------------------------------------------------------------------------------
LN_GLOBAL_COLS = 1e-4                # the rel_l2 bar tests/test_layernorm.py holds dgamma and dbeta to
LN_GLOBAL_DBIAS = 1e-5               # and dbias_drop, against the column sums of the stored dx
LN_BWD_MAXBLK = 512                  # layernorm.hip m3p_layernorm_bwd_rows: min(ceil(rows / 4), 512) blocks of 4 rows, or
LN_BWD_HW_ROWS = 8                   # LN_BWD_BLOCKS = 512 blocks of 8 rows (ln_bwd_hw_kernel, d = 768 / 1024)
LN_FAULT_COL = 77


def _ln_cols_f32(x, dya, dyb, g, lose_term=None, first_trip_only=0):
    """The LayerNorm kernels' arithmetic in fp32 (NumPy): two-pass mean and variance, xhat from the fp32 mean and rstd, the
    per-row products, dx rounded to bf16 as it is stored, then the three column sums over the rows one after the other (an
    order no better than the kernels': every wave adds its rows, the block its four waves, atomics the blocks).
    lose_term = (row, column) whose dgamma term is left out; first_trip_only = rows the first trip of the grid covers (the
    rest is lost from all three sums).  -> dict of mean, rstd, dg, db, dbias (of the stored bf16 dx), dbias_unrounded, dx (bf16)."""
    f = np.float32
    x, dya, dyb, g = (t.numpy().astype(f) for t in (x, dya, dyb, g))
    rows, d = x.shape
    inv_d = f(1.0) / f(d)
    mu = x.sum(-1, dtype=f) * inv_d
    xc = x - mu[:, None]
    rs = f(1.0) / np.sqrt((xc * xc).sum(-1, dtype=f) * inv_d + f(1e-12))
    xh = xc * rs[:, None]
    dy = dya + dyb
    gd = dy * g
    c1, c2 = gd.sum(-1, dtype=f) * inv_d, (gd * xh).sum(-1, dtype=f) * inv_d
    o = (gd - c1[:, None] - xh * c2[:, None]) * rs[:, None]
    ob = torch.from_numpy(o).to(torch.bfloat16)
    tg = dy * xh
    if lose_term is not None:
        tg[lose_term] = 0
    n = first_trip_only or rows
    dg, db, dbias, dbias_u = (np.zeros(d, f) for _ in range(4))
    obf = ob.float().numpy()
    for r in range(n):
        dg += tg[r]; db += dy[r]; dbias += obf[r]; dbias_u += o[r]
    t = torch.from_numpy
    return dict(mean=t(mu), rstd=t(rs), dg=t(dg), db=t(db), dbias=t(dbias), dbias_unrounded=t(dbias_u), dx=ob)


@pytest.fixture(scope='module', params=[(2051, 132), (4101, 768)], ids=lambda s: '%dx%d' % s)
def ln_cols(request):
    """x, and gradients with a part common to the rows, as a trained layer's are: dy_a = bf16(xhat + noise), dy_b = bf16(1 + noise),
    so that dgamma and dbeta are about the number of rows in every column.  (With gradients of zero mean a column is a random walk
    of about sqrt(rows), and one lost term of it already stands out of the global bar.)"""
    rows, d = request.param
    gen = torch.Generator().manual_seed(31)
    rnd = lambda *s: torch.randn(s, generator=gen, dtype=torch.float64)      # noqa: E731
    x = _bf16(rnd(rows, d) * 2.0)
    mu = x.mean(-1)
    rs = 1.0 / torch.sqrt((x - mu[:, None]).pow(2).mean(-1) + 1e-12)
    xhat = (x - mu[:, None]) * rs[:, None]
    dya, dyb = _bf16(xhat + rnd(rows, d)), _bf16(1.0 + rnd(rows, d))
    g = (1.0 + 0.5 * rnd(d)).float().double()
    dy = dya + dyb
    return dict(rows=rows, d=d, x=x, dya=dya, dyb=dyb, g=g, dy=dy, mu=mu, rs=rs, xhat=xhat,
                dg=(dy * xhat).sum(0), db=dy.sum(0), clean=_ln_cols_f32(x, dya, dyb, g))


def _ln_worst(c, k):
    (wg, ag), (wb, ab) = U.ln_colsum_bounds(k['dg'], k['db'], c['dy'], c['x'], c['mu'], c['rs'])
    wd, ad = U.ln_dbias_bound(k['dbias'], k['dx'])
    return {'dg': (wg, ag['row']), 'db': (wb, ab['row']), 'dbias': (wd, ad['row'])}       # (1-D outputs are columns: 'row' = the column)


def test_ln_column_bounds_accept_the_fp32_restatement(ln_cols):
    """The restatement's mean and rstd pass the bounds ln_dgamma_extra is derived from, and its three column sums reach
    0.044 / 0.009 / 0.005 (2051 x 132) and 0.038 / 0.013 / 0.011 (4101 x 768) of dgamma's, dbeta's and dbias' bounds.  The bounds
    ln_stat_bounds hands out are the very denominators of those two assertions: a value off by exactly that much sits at 1."""
    c, k = ln_cols, ln_cols['clean']
    U.assert_gemm_bound(k['mean'], c['mu'], c['x'].abs().mean(-1), c['d'], U.F32_OUT, what='mean')
    U.assert_gemm_bound(k['rstd'], c['rs'], c['rs'], c['d'], U.F32_OUT, what='rstd')
    e_mu, e_rs = U.ln_stat_bounds(c['x'], c['mu'], c['rs'])
    assert abs(U.gemm_bound(c['mu'] + e_mu, c['mu'], c['x'].abs().mean(-1), c['d'], U.F32_OUT)[0] - 1.0) < 1e-6
    assert abs(U.gemm_bound(c['rs'] + e_rs, c['rs'], c['rs'], c['d'], U.F32_OUT)[0] - 1.0) < 1e-6
    worst = {n: w for n, (w, _) in _ln_worst(c, k).items()}
    print('LayerNorm column sums, fp32 restatement at %d x %d: %s' % (c['rows'], c['d'], worst))
    assert all(w < 0.5 for w in worst.values()), worst
    assert U.rel_l2(k['dg'], c['dg']) < LN_GLOBAL_COLS and U.rel_l2(k['db'], c['db']) < LN_GLOBAL_COLS


@pytest.mark.parametrize('fault', ['dgamma_lost_term', 'dbeta_neighbour', 'dbias_unrounded', 'second_trip_lost'])
def test_ln_column_bounds_reject_lost_terms_and_rows(ln_cols, fault):
    """The per-column bounds reject all four faults, and name the column of the two that have one.  What the global bars of
    tests/test_layernorm.py make of them is asserted as it is:
    - one lost term of one dgamma column passes rel_l2 < 1e-4;
    - a dbeta column that holds its neighbour's sum does not: the two sums differ by sqrt(2 rows) noise terms, 2e-3 of the
      vector and more on these shapes;
    - nor do sums without the 3 (5) rows past the first trip of 512 blocks: 3 / 2051 (5 / 4101) of every column even where all
      terms have one sign, 1.2e-3 at the least;
    - nor does dbias summed from the fp32 dx (its bar is 1e-5 against the stored values; the bf16 roundings are 1e-3 of them)."""
    c, k = ln_cols, dict(ln_cols['clean'])
    rows, d = c['rows'], c['d']
    if fault == 'dgamma_lost_term':
        r = int((c['dy'] * c['xhat'])[:, LN_FAULT_COL].abs().median(0).indices)      # a term of median size in its column
        k['dg'] = _ln_cols_f32(c['x'], c['dya'], c['dyb'], c['g'], lose_term=(r, LN_FAULT_COL))['dg']
        hit, col = ('dg',), LN_FAULT_COL
        assert U.rel_l2(k['dg'], c['dg']) < LN_GLOBAL_COLS
    elif fault == 'dbeta_neighbour':
        k['db'] = k['db'].clone()
        k['db'][LN_FAULT_COL] = k['db'][LN_FAULT_COL + 1]
        hit, col = ('db',), LN_FAULT_COL
        assert U.rel_l2(k['db'], c['db']) > LN_GLOBAL_COLS
    elif fault == 'dbias_unrounded':
        k['dbias'] = k['dbias_unrounded']
        hit, col = ('dbias',), None
        assert LN_GLOBAL_DBIAS < U.rel_l2(k['dbias'], k['dx'].double().sum(0)) < 2.0 ** -9
    else:
        per_block = LN_BWD_HW_ROWS if d in (768, 1024) else 4
        first = LN_BWD_MAXBLK * per_block
        assert first < rows <= first + 8
        k = _ln_cols_f32(c['x'], c['dya'], c['dyb'], c['g'], first_trip_only=first)
        k['dx'] = ln_cols['clean']['dx']
        hit, col = ('dg', 'db', 'dbias'), None
        assert U.rel_l2(k['dg'], c['dg']) > LN_GLOBAL_COLS
        assert U.rel_l2(k['db'], c['db']) > LN_GLOBAL_COLS
    worst = _ln_worst(c, k)
    print('LayerNorm column sums, %s at %d x %d: %s' % (fault, rows, d, {n: round(w, 3) for n, (w, _) in worst.items()}))
    for n in ('dg', 'db', 'dbias'):
        if n in hit:
            assert worst[n][0] > 2.0 and col in (None, worst[n][1]), (fault, n, worst)
        else:
            assert worst[n][0] < 0.5, (fault, n, worst)


# --- attention backward of a batch entry with a single key -------------------------------------------------------------
ATTN_SINGLE_KEY_BAR = 1e-2          # test_attention_fwd_bwd, the single position: |dq|, |dk| < 1e-2 x the gradient's norm


def _single_key_residue(B, S, H, dh, round_p, p=0.1, b=1, seed=4242):
    """Entry b (keylen = 1) of test_attention_short_key_lengths on its own data, as the kernels' documented arithmetic has it:
    P = 1, z = keep / (1 - p), O = bf16(z V_0) with z rounded to bf16 first (round_p: it is an operand of the P V product), D =
    dO . O, dS = z dO . V_0 - D.  -> (|dq|, |dk|, |dv|) of the entry, in fp64."""
    from m3p_amd import rng
    d = H * dh
    _, qkv = U.randn_bf16((B * S, 3 * d), 1, 0.7, device='cpu')
    _, dctx = U.randn_bf16((B * S, d), 7, device='cpu')
    keep = torch.from_numpy(rng.keep_mask(B * H * S * S, seed, p, (B, H, S, S)))[b, :, :, 0].double()
    x = qkv[b * S:(b + 1) * S].double().view(S, 3, H, dh)
    q, k0, v0 = x[:, 0], x[0, 1], x[0, 2]
    do = dctx[b * S:(b + 1) * S].double().view(S, H, dh)
    z = keep.t() / (1 - p)
    o = _bf16((_bf16(z) if round_p else z)[..., None] * v0)
    ds = z * (do * v0).sum(-1) - (do * o).sum(-1)
    dq, dk, dv = ds[..., None] * k0 / math.sqrt(dh), (ds[..., None] * q).sum(0), (z[..., None] * do).sum(0)
    return float(dq.norm()), float(dk.norm()), float(dv.norm())


def test_single_key_bar_is_reached_by_the_restatement_of_the_rounded_context():
    """With one valid key dq = dk = 0 exactly; the kernels leave the residue of D = rowsum(dO * O) taken from the bf16 context.
    The restatement reproduces what the kernels gave on an MI355X at (11, 356, 2, 64), |dq| = 0.259, |dk| = 2.28, |dv| = 225:
    dk is 1.015 of the old bar there (0.70 with z unrounded: bf16(1 / 0.9) = 1.109375 is 1.6e-3 low in every kept query, as
    large as the rounding of the product), and 0.54 .. 0.76 of it at the other shapes of that test; dq stays under 0.15 of it.  So
    tests/test_attention.py holds dk of such an entry to this restatement (from the kernel's stored context) by the row
    bound, and keeps the 1e-2 bar for dq."""
    got = {shape: _single_key_residue(*shape, round_p=True) for shape in ((11, 164, 2, 64), (11, 74, 2, 32), (11, 180, 2, 64),
                                                                           (11, 200, 2, 32), (11, 356, 2, 64))}
    for shape, (ndq, ndk, ndv) in got.items():
        print('single key %s: |dq| = %.3g, |dk| = %.3g, |dv| = %.3g: %.3g and %.3g of the bar' % (
            shape, ndq, ndk, ndv, ndq / (ATTN_SINGLE_KEY_BAR * ndv), ndk / (ATTN_SINGLE_KEY_BAR * ndv)))
        assert ndq < 0.2 * ATTN_SINGLE_KEY_BAR * ndv
        assert (ndk > ATTN_SINGLE_KEY_BAR * ndv) == (shape[1] == 356)
    ndq, ndk, ndv = got[(11, 356, 2, 64)]
    assert abs(ndq - 0.259) < 2e-3 and abs(ndk - 2.28) < 1e-2 and abs(ndv - 225.1) < 0.1
    assert 1.0 < ndk / (ATTN_SINGLE_KEY_BAR * ndv) < 1.03
    plain = _single_key_residue(11, 356, 2, 64, round_p=False)
    assert 0.65 < plain[1] / (ATTN_SINGLE_KEY_BAR * plain[2]) < 0.75
