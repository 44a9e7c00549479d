import contextlib
import math

import numpy as np
import pytest
import torch

BF16 = torch.bfloat16


def rel_l2(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ---------------------------------------------------------------------------------------------------------------------
# Elementwise and per-block bounds.  A global relative L2 norm over tens of millions of elements leaves room for a kernel
# that is wrong in one row, one fragment or one head (tests/test_parity_bounds.py injects such faults and shows them
# passing the global bars); these bound every element, or every row, from a floating-point error model instead.
# ---------------------------------------------------------------------------------------------------------------------

# The global bars the GPU parity tests apply with rel_l2 (kept beside the new bounds).
GLOBAL_GEMM = 4e-3              # bf16 GEMM outputs
GLOBAL_ATTN_CTX = 6e-3          # attention context
GLOBAL_ATTN_GRAD = 1.5e-2       # attention dq / dk / dv

# Accumulation error of a depth-K fp32 dot product, in units of sqrt(K) 2^-24 sum_k |a_k w_k|: the worst case grows like K,
# rounding errors of random sign like sqrt(K) with a spread of a few units.  Chosen once from the model, not per test.
KAPPA = 8.0
U32 = 2.0 ** -24                # unit roundoff of fp32
BF16_OUT = 2.0 ** -8            # out_rounding of a bf16 output: its unit roundoff (8 significant bits), the most
                                # round-to-nearest moves a value relative to itself
F32_OUT = 4 * 2.0 ** -24        # out_rounding of an fp32 output: a few fp32 roundings of the epilogue

# Per-row bars of attention, from the kernel's precision.  The operands of its MFMA products are bf16: P (forward and dV),
# dS = P (dP - D) (dQ and dK), and each output is stored in bf16.  One such rounding is at most 2^-8 relative per element
# (2^-9 on average), so it moves a row by at most 2^-8 of the norm of the terms it enters.
# - ctx = P V and dv = P^T dO: the rounding of P and of the output, 2 x 2^-8 = 4 x 2^-9 (the CPU restatement reaches
#   4.2e-3, the kernels 5.1e-3).  A row below ROW_FLOOR times the RMS row norm of its (b, h) head is measured against it.
# - dq = dS K and dk = dS^T Q: the rows of dS sum to exactly 0, so a row of dq is a difference of keys and can be far
#   smaller than the terms whose dS rounding (2^-9 each) it carries; the rounded D = rowsum(dO * O) of the bf16 O moves every
#   dS of a row alike.  No per-row relative bar follows from the precision: measured against the RMS row of the head
#   (ATTN_DS_FLOOR = 1), the fp64 restatement with bf16 dS reaches 2e-2 on 1312 rows (tests/test_parity_bounds.py) and the
#   kernels 5.4e-2 on the 504 K rows of the benchmarked launch (B = 256), the tail growing with the number of rows.  The
#   bar, 2^-3, is for rows a kernel loses, zeroes or misplaces (relative error ~1), not a few per cent of scale: those
#   show in ctx and dv, which share the kernel's P.
ATTN_CTX_RTOL = 4 * 2.0 ** -9
ATTN_DS_RTOL = 2.0 ** -3
ROW_FLOOR = 0.25
ATTN_DS_FLOOR = 1.0
ROW_RTOL_BF16 = 2.0 ** -8       # rows of a bf16 output computed in fp32 from exact inputs (LayerNorm, softmax gradients)
# de of the embedding assembly: two bf16 roundings (the stored dz, then de) with a LayerNorm backward between them, which
# keeps the relative size of the first; independent over a row, they add in quadrature.  The CPU restatement reaches 0.68 of
# ROW_RTOL_BF16 on 768 rows (tests/test_parity_bounds.py), one rounding alone 0.48; the kernels 0.72 on 9216 rows.
EMBED_DE_RTOL = math.sqrt(2.0) * ROW_RTOL_BF16

_TINY = 1e-300
_CHUNK = 1 << 24                # elements compared at once: a few hundred MB of fp64 temporaries at most


def gemm_bound(got, ref64, absref64, depth, out_rounding, eps_epi=0.0, row0=0, linear=False):
    """Largest normalised error  |got - ref| / (out_rounding |ref| + KAPPA sqrt(depth) 2^-24 absref + eps_epi + tiny)  of a
    GEMM output and where it occurs.  ref64 = the exact result in fp64; absref64 = the same expression with |A| |W|^T in
    place of the product and the absolute values of the epilogue's addends (every fp32 operation of the epilogue rounds
    relative to its operands); eps_epi = the documented approximation error of the epilogue function, a number or a
    tensor shaped like the output.  A NaN anywhere (an unwritten poisoned element) counts as an infinite error.  1-D
    outputs are columns.  row0 = the row of got[0] in the whole output (callers that compare in row chunks).
    linear: the worst-case accumulation term 2 depth 2^-24 absref in place of KAPPA sqrt(depth) 2^-24 absref, for matrix
    instructions whose additions are not each rounded to nearest (the 8-bit MFMA of gfx950 sums 128 products in one
    instruction; its error exceeds the sqrt(depth) model by up to 1.25 x at K = 128 - no sqrt(K) cancellation - and stays
    within 2 u per addition, the bound of directed rounding).
    Returns (worst, {'row', 'col', 'tile256', 'frag16'})."""
    got = torch.as_tensor(got).detach()
    if got.dim() == 1:
        got, ref64, absref64 = got[:, None], ref64[:, None], absref64[:, None]
        if torch.is_tensor(eps_epi) and eps_epi.dim() == 1:
            eps_epi = eps_epi[:, None]
    assert got.shape == ref64.shape == absref64.shape, (got.shape, ref64.shape, absref64.shape)
    acc = (2.0 * depth if linear else KAPPA * math.sqrt(depth)) * 2.0 ** -24
    rows, cols = got.shape
    step = max(1, _CHUNK // max(cols, 1))
    worst, at = -1.0, (0, 0)
    for r0 in range(0, rows, step):
        sl = slice(r0, r0 + step)
        ref = ref64[sl].double()
        g = got[sl].to(ref.device, torch.float64)
        eps = eps_epi[sl].to(ref.device, torch.float64) if torch.is_tensor(eps_epi) and eps_epi.dim() == 2 else eps_epi
        den = out_rounding * ref.abs() + acc * absref64[sl].to(ref.device, torch.float64) + eps + _TINY
        r = torch.nan_to_num((g - ref).abs() / den, nan=math.inf)
        v, i = r.reshape(-1).max(0)
        if float(v) > worst:
            worst, at = float(v), (r0 + int(i) // cols, int(i) % cols)
    i, j = at[0] + row0, at[1]
    return worst, {'row': i, 'col': j, 'tile256': (i // 256, j // 256), 'frag16': (i // 16, j // 16)}


def assert_gemm_bound(got, ref64, absref64, depth, out_rounding, eps_epi=0.0, what='', row0=0, linear=False):
    worst, at = gemm_bound(got, ref64, absref64, depth, out_rounding, eps_epi, row0, linear)
    assert worst <= 1.0, '%s: the error reaches %.3g x the elementwise bound at row %d, column %d (256 x 256 tile %s, ' \
                         '16 x 16 fragment %s)' % (what, worst, at['row'], at['col'], at['tile256'], at['frag16'])
    return worst


def block_bound(got, ref, blocks, rtol, floor):
    """Relative error of every block of ``got``.  got and ref are shaped [*groups, n_blocks, block]: the last dimension is
    one block (a row, or one (b, h, query) row of attention), the one before it counts the blocks of a group, and
    ``blocks`` names every dimension but the last for the report.  The denominator of a block is max(|ref_block|, floor *
    RMS block norm of its group), so rows with a tiny reference are not blown up.  NaN counts as infinite.
    Returns (worst relative error, {name: index} of the worst block, worst / rtol)."""
    ref = torch.as_tensor(ref).detach().double()
    got = torch.as_tensor(got).detach().to(ref.device, torch.float64)
    assert got.shape == ref.shape and len(blocks) == ref.dim() - 1, (got.shape, ref.shape, blocks)
    err = torch.nan_to_num((got - ref).norm(dim=-1), nan=math.inf)
    nrm = ref.norm(dim=-1)
    rms = nrm.pow(2).mean(dim=-1, keepdim=True).sqrt()
    rel = err / (torch.maximum(nrm, floor * rms) + _TINY)
    v, i = rel.reshape(-1).max(0)
    idx = np.unravel_index(int(i), tuple(rel.shape))
    return float(v), {n: int(k) for n, k in zip(blocks, idx)}, float(v) / rtol


def assert_block_bound(got, ref, blocks, rtol, floor=ROW_FLOOR, what=''):
    worst, at, _ = block_bound(got, ref, blocks, rtol, floor)
    assert worst <= rtol, '%s: block %s has relative error %.3g > %.3g' % (what, at, worst, rtol)
    return worst


# The GELU of csrc/common.hpp (gelu_parts), shared by the GEMM epilogues and the streaming GELU kernels.  The dGELU epilogue
# looks gelu' up in a table of fp32 values that is exact to fp32 except below |u| = 2^-15, where the first entry serves:
# 2.4e-5 (csrc/gemm.hip: gelu_grad_table_fill).  The GELU epilogue evaluates erf with |error| <= 1.5e-7 (csrc/common.hpp:83).
EPS_DGELU = 2.4e-5
EPS_ERF = 1.5e-7


def _gelu64(x, device='cuda'):
    x = x.to(device).double()
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def _dgelu64(x, device='cuda'):
    x = x.to(device).double()
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


# The gate of nn.GLU (csrc/refiner.hip: sigmoid_f = v_rcp_f32(1 + __expf(-b))).  v_exp_f32 and v_rcp_f32 are accurate to 1 ulp
# = 2 u each; __expf rounds its argument -b log2(e) once, which moves the exponential by |b| u relative; the sum 1 + e rounds
# once.  The relative error of the sigmoid is within (2 + |b|) u e / (1 + e) + u + 2 u <= (5 + |b|) u.  Forward y = a s: one
# more product.  Backward db = g a s (1 - s): the error d of s enters as g a s d (1 - 2 s), and four more roundings of
# products and the difference: within |g a| s (9 + |b|) u.  The fp32 restatement of tests/test_parity_bounds.py (libm exp,
# IEEE division) reaches 0.50 of the forward and da terms and 0.31 of the db term.
def glu_eps(a, b, g=None):
    """Approximation terms (eps_epi of gemm_bound) of GLU forward, or with the output gradient g of its backward (da, db)."""
    a, b = a.double(), b.double()
    s = torch.sigmoid(b)
    if g is None:
        return a.abs() * s * (6.0 + b.abs()) * U32
    g = g.double()
    return g.abs() * s * (6.0 + b.abs()) * U32, (g * a).abs() * s * (9.0 + b.abs()) * U32


# ---------------------------------------------------------------------------------------------------------------------
# Streaming kernels: the fused Adam update, the sum of squares, fp32 sums gathered with atomics.
# ---------------------------------------------------------------------------------------------------------------------
# Roundings of the fused update (csrc/optim.hip: adam_kernel), counted: the clip coefficient costs about 3 (square root,
# division, product with grad_scale) and enters m once and v twice; then the products, the sum, the correctly rounded sqrtf
# and division, the two subtractions.  Contraction to FMA only removes roundings.  The fp32 restatement of
# tests/test_parity_bounds.py reaches 2.4, 3.7 and 5.1 u against these, the kernels 2.7, 4.3 and 4.7 u at 12.6 M elements.
ADAM_M_U, ADAM_V_U, ADAM_P_U = 8.0, 12.0, 16.0


def _f32(x):
    return float(np.float32(x))


def adam_ref64(p, g, m, v, hp):
    """The fused Adam update in fp64 from fp32 state and the fp32 values of the scalars, with the bounds of its three
    outputs.  hp: lr, beta1, beta2, eps, weight_decay, step_size, max_norm, grad_scale, gnorm_sq (a number read from the
    device scalar the kernel is handed, or None).  With gc = g coef, A_m = |beta1 m| + |(1 - beta1) gc|, den = sqrt(v_new)
    + eps:  |m_new - ref| <= 8 u A_m,  |v_new - ref| <= 12 u v_ref,  |p_new - ref| <= 16 u (|p| + step_size A_m / den).
    Returns (p_ref, m_ref, v_ref), (p_bound, m_bound, v_bound), all fp64 on the device of p."""
    b1, b2, eps, lr = _f32(hp['beta1']), _f32(hp['beta2']), _f32(hp['eps']), _f32(hp['lr'])
    wdl = _f32(hp['weight_decay']) * lr
    step_size, max_norm = _f32(hp['step_size']), _f32(hp['max_norm'])
    gs = _f32(hp['grad_scale']) or 1.0                       # (the launcher reads 0 as 1)
    coef = gs
    if hp.get('gnorm_sq') is not None and max_norm > 0:
        c = max_norm / (math.sqrt(float(hp['gnorm_sq'])) * gs + _f32(1e-6))
        coef *= min(c, 1.0)
    p, g, m, v = (t.double() for t in (p, g, m, v))
    gc = g * coef
    a_m = (b1 * m).abs() + ((1.0 - b1) * gc).abs()
    m_ref = b1 * m + (1.0 - b1) * gc
    v_ref = b2 * v + (1.0 - b2) * gc * gc
    den = v_ref.sqrt() + eps
    p_ref = (p - wdl * p) - step_size * (m_ref / den)
    return (p_ref, m_ref, v_ref), (ADAM_P_U * U32 * (p.abs() + step_size * a_m / den), ADAM_M_U * U32 * a_m,
                                   ADAM_V_U * U32 * v_ref)


def adam_bound(got, before, hp, start=0):
    """Largest |got - ref| / bound of the parameters, first and second moments after one fused Adam step, over every element,
    and where.  got = (p, m, v) after the step, before = (p, g, m, v) before it (fp32, same length).  An element whose
    bound is 0 (all of its terms are 0) must be exact; NaN counts as infinite.  Compared in chunks; start = the index of
    element 0 in the whole arena, for the report.  Returns {'p' | 'm' | 'v': (worst, index)}."""
    n = before[0].numel()
    worst = {k: (-1.0, start) for k in 'pmv'}
    for i0 in range(0, n, _CHUNK):
        sl = slice(i0, i0 + _CHUNK)
        refs, bounds = adam_ref64(*(t.reshape(-1)[sl] for t in before), hp)
        for k, x, ref, bnd in zip('pmv', got, refs, bounds):
            err = (x.reshape(-1)[sl].to(ref.device, torch.float64) - ref).abs()
            r = torch.nan_to_num(torch.where(err == 0, torch.zeros_like(err), err / bnd), nan=math.inf, posinf=math.inf)   # (0 / 0 = 0; x / 0 = inf)
            w, i = r.max(0)
            if float(w) > worst[k][0]:
                worst[k] = (float(w), start + i0 + int(i))
    return worst


def assert_adam_bound(got, before, hp, what='', start=0):
    worst = adam_bound(got, before, hp, start)
    for k, name in zip('pmv', ('parameter', 'first moment', 'second moment')):
        assert worst[k][0] <= 1.0, '%s: the %s at element %d (quad %d) is off by %.3g x its bound' % (
            what, name, worst[k][1], worst[k][1] // 4, worst[k][0])
    return {k: w for k, (w, _) in worst.items()}


def sumsq_bound(got, ref64, t):
    """|got - ref| / ((t + 8) u ref) of a sum of squares accumulated in fp32: t = the number of 4-element quads one thread
    adds up (its running sum rounds once per quad; the 8 covers the squares and sums inside a quad and the reduction across
    the wave).  All terms are non-negative, so the worst case is linear in t and relative to the result."""
    got, ref64 = float(got), float(ref64)
    if math.isnan(got):
        return math.inf
    return abs(got - ref64) / ((t + 8) * U32 * ref64 + _TINY)


def assert_sumsq_bound(got, ref64, t, what=''):
    worst = sumsq_bound(got, ref64, t)
    assert worst <= 1.0, '%s: sum of squares %r against %r is off by %.3g x the bound (t = %d)' % (what, float(got), float(ref64), worst, t)
    return worst


def accum_bound(got, ref64, abssum64, n_terms, extra=0.0):
    """Elements of an fp32 sum of n_terms addends gathered in any order (atomics):  |got - ref| <= KAPPA sqrt(n_terms) u
    sum|terms| + extra, the accumulation model of gemm_bound.  abssum64 = the same sum over the absolute values of every
    operand of every term; n_terms a number or a tensor that broadcasts against the output (rows that gather different
    numbers of terms); extra = what is not accumulation (a bf16 rounding upstream), same shape or a number.
    Returns (worst, {'row', 'col', ...}) like gemm_bound."""
    n = torch.as_tensor(n_terms, dtype=torch.float64, device=ref64.device).clamp(min=1.0)
    bound = KAPPA * n.sqrt() * U32 * abssum64 + extra
    if bound.dim() < ref64.dim() or bound.shape != ref64.shape:
        bound = bound.expand_as(ref64)
    return gemm_bound(got, ref64, torch.zeros_like(ref64), 0, 0.0, bound.contiguous())


def assert_accum_bound(got, ref64, abssum64, n_terms, extra=0.0, what=''):
    worst, at = accum_bound(got, ref64, abssum64, n_terms, extra)
    assert worst <= 1.0, '%s: the error reaches %.3g x the accumulation bound at row %d, column %d' % (what, worst, at['row'], at['col'])
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# Column gradients of LayerNorm (csrc/layernorm.hip: acc_g, acc_b, acc_d, gathered over waves, blocks and trips of the grid).
# ---------------------------------------------------------------------------------------------------------------------
def ln_stat_bounds(x64, mu64, rs64):
    """What the LayerNorm tests allow the saved fp32 mean and rstd of each row to be off by: the denominators of
    assert_gemm_bound(mean, mu64, mean|x|, d, F32_OUT) and assert_gemm_bound(rstd, rs64, rs64, d, F32_OUT).  -> (e_mu, e_rs), [rows]."""
    d = x64.shape[-1]
    acc = KAPPA * math.sqrt(d) * U32
    return F32_OUT * mu64.abs() + acc * x64.abs().mean(-1), (F32_OUT + acc) * rs64


def ln_dgamma_extra(dy64, x64, mu64, rs64):
    """The part of dgamma's error that is not accumulation: the kernel's xhat = (x - mean) * rstd is formed in fp32 from the
    saved fp32 mean and rstd, which carry the error of their own depth-d sums.  To first order
        |xhat - xhat64| <= e_mu rs64 + |x - mu64| e_rs + F32_OUT |xhat64|
    with (e_mu, e_rs) = ln_stat_bounds, the very bounds the mean / rstd assertions put on those two numbers, and F32_OUT for
    the roundings of the difference, the two products and the sum dy_a + dy_b (four fp32 operations).  -> sum_r |dy| times that,
    [d]: the `extra` of accum_bound.  Worst case over the rows (no sqrt): the errors of mean and rstd are not independent of the
    data.  The fp32 restatement of tests/test_parity_bounds.py reaches 0.044 of the whole bound at 2051 x 132 and 0.038 at
    4101 x 768 (the rounding errors do cancel); one lost term of median size in a column reaches 7.5 and 2.1."""
    e_mu, e_rs = ln_stat_bounds(x64, mu64, rs64)
    xc = x64 - mu64[:, None]
    dxhat = (e_mu * rs64)[:, None] + xc.abs() * e_rs[:, None] + F32_OUT * (xc * rs64[:, None]).abs()
    return (dy64.abs() * dxhat).sum(0)


def ln_colsum_bounds(dg, db, dy64, x64, mu64, rs64):
    """dgamma = sum_r dy xhat and dbeta = sum_r dy of LayerNorm backward, every column against fp64 with accum_bound over
    n_terms = rows.  dy64 = the fp64 sum dy_a + dy_b with masked rows zeroed (the kernel multiplies dy by the row mask).
    -> ((worst, at) of dgamma, (worst, at) of dbeta)."""
    rows = x64.shape[0]
    xhat = (x64 - mu64[:, None]) * rs64[:, None]
    wg = accum_bound(dg, (dy64 * xhat).sum(0), (dy64.abs() * xhat.abs()).sum(0), rows, ln_dgamma_extra(dy64, x64, mu64, rs64))
    wb = accum_bound(db, dy64.sum(0), dy64.abs().sum(0), rows)
    return wg, wb


def ln_dbias_bound(dbias, stored):
    """dbias_drop against the fp64 column sums of the bf16 values the kernel stored (dx_drop, or what it would have held):
    exact terms, so accumulation error only."""
    s = stored.double()
    return accum_bound(dbias, s.sum(0), s.abs().sum(0), s.shape[0])


# ---------------------------------------------------------------------------------------------------------------------
# The row kernels behind the shifted-exponential MLM head (csrc/heads.hip: ce_shift_*).
# ---------------------------------------------------------------------------------------------------------------------
CE_SHIFT = 40.0                 # heads.hip CE_SHIFT: the rows' shift above the target's own logit
CE_LSE_SPLIT = 32               # heads.hip CE_LSE_SPLIT: the splits of a row's blocks, one partial sum each


def shift_rowsum_adds(n_blocks):
    """The most fp32 additions any one block sum passes through on its way into a row's sum (ce_shift_partial_kernel, then
    ce_shift_final_kernel).  All addends are positive, so the sum's relative error is at most that many unit roundoffs -
    linear in the count, as in sumsq_bound.  Counted in the kernels' order:
      t   a split holds per = ceil(n_blocks / 32) blocks and its four waves take every fourth, so a thread adds at most
          t = ceil(per / 4) of them one after the other (the unrolled loop spreads them over four accumulators and only the
          tail is sequential: t is the upper bound of both);
      2   the thread's four accumulators, (s0 + s1) + (s2 + s3);
      2   the four waves of the block, (w0 + w1) + (w2 + w3);
      32  the partial sums of the 32 splits, added one after the other."""
    per = -(-int(n_blocks) // CE_LSE_SPLIT)
    t = -(-per // 4)
    return t + 2 + 2 + CE_LSE_SPLIT


def shift_rows_ref64(stats, gs):
    """fp64 (row sum, loss, s, q) of ce_shift_from_block_sums from the fp32 block sums [n_blocks, n] and the fp32 value of the
    gradient scale: r = sum e^40 is the other columns' mass relative to the target's; loss = log1p(r), s = gs / (sum + e^-40),
    q = gs expm1(-loss) = gs (p_target - 1)."""
    gs = _f32(gs)
    total = stats.double().sum(0)
    loss = torch.log1p(total * math.exp(CE_SHIFT))
    return total, loss, gs / (total + math.exp(-CE_SHIFT)), gs * torch.expm1(-loss)


def shift_rows_bound(row_loss, row_s, row_q, stats, gs):
    """Every row's loss, s and q against shift_rows_ref64, in units of its bound.  With rho = shift_rowsum_adds(n_blocks) u,
    the relative error of the row sum: the loss moves by at most rho (d log1p(r) = dr / (1 + r) <= dr / r), plus the fp32
    evaluation of 40 + log(sum + e^-40), relative to its operands: F32_OUT (40 + loss), absolute.  s and q are held relative
    to themselves: rho plus F32_OUT 40 (q = gs expm1(-loss) follows the loss' absolute error, at most F32_OUT 40 where the
    second branch begins, at loss = log 2, where d q / q = d loss / (e^loss - 1) = d loss).  NaN counts as infinite.
    Returns {'loss' | 's' | 'q': (worst, row)}."""
    _, loss, s, q = shift_rows_ref64(stats, gs)
    rho = shift_rowsum_adds(stats.shape[0]) * U32
    out = {}
    for k, got, ref, bound in (('loss', row_loss, loss, rho + F32_OUT * (CE_SHIFT + loss)),
                               ('s', row_s, s, s.abs() * (rho + F32_OUT * CE_SHIFT)),
                               ('q', row_q, q, q.abs() * (rho + F32_OUT * CE_SHIFT))):
        r = torch.nan_to_num((got.to(ref.device, torch.float64) - ref).abs() / (bound + _TINY), nan=math.inf)
        w, i = r.max(0)
        out[k] = (float(w), int(i))
    return out


def assert_shift_rows_bound(row_loss, row_s, row_q, stats, gs, what=''):
    worst = shift_rows_bound(row_loss, row_s, row_q, stats, gs)
    for k, (w, i) in worst.items():
        assert w <= 1.0, '%s: %s of row %d is off by %.3g x its bound (%d blocks)' % (what, k, i, w, stats.shape[0])
    return {k: w for k, (w, _) in worst.items()}


def scale_rows_bound(got, h, row_s, g):
    """ce_shift_scale_rows: bf16(g s_n h[n, :]) against fp64 - one bf16 rounding of the result plus the fp32 products, F32_OUT
    relative to |g s h|."""
    ref = float(g) * row_s.double()[:, None] * h.double()
    return gemm_bound(got, ref, torch.zeros_like(ref), 0, BF16_OUT, F32_OUT * ref.abs())


def shift_dh_bound(got, dh32, emb_rows, row_s, row_q, g):
    """ce_shift_dh: bf16(g (s_n dh32[n, :] + q_n E[y_n, :])) against fp64 (emb_rows = E[y], [n, d]) - one bf16 rounding of the
    result plus the fp32 evaluation, relative to the two terms that may cancel: F32_OUT |g| (|s dh32| + |q E[y]|)."""
    a, b = row_s.double()[:, None] * dh32.double(), row_q.double()[:, None] * emb_rows.double()
    ref = float(g) * (a + b)
    return gemm_bound(got, ref, torch.zeros_like(ref), 0, BF16_OUT, F32_OUT * abs(float(g)) * (a.abs() + b.abs()))


def target_rows_bound(demb, dbias, demb0, dbias0, h, y, row_q, g):
    """ce_shift_target_rows: demb[y_n, :] += g q_n h[n, :] and dbias[y_n] += g q_n onto what the two held before (demb0,
    dbias0), fp32 atomics in any order.  accum_bound with as many terms per word as rows name it; the products g q h are
    rounded in fp32 before they are added: extra = F32_OUT sum |g q h|.  Returns ((worst, at) of demb, (worst, at) of dbias)."""
    V = demb0.shape[0]
    c = float(g) * row_q.double()
    terms = c[:, None] * h.double()
    cnt = torch.bincount(y, minlength=V).double()
    ref = demb0.double().index_add(0, y, terms)
    at = torch.zeros_like(ref).index_add(0, y, terms.abs())
    we = accum_bound(demb, ref, demb0.double().abs() + at, cnt[:, None], F32_OUT * at)
    refb = dbias0.double().index_add(0, y, c)
    ab = torch.zeros_like(refb).index_add(0, y, c.abs())
    wb = accum_bound(dbias, refb, dbias0.double().abs() + ab, cnt, F32_OUT * ab)
    return we, wb


def assert_bits_equal(got, ref, what=''):
    """Bit-for-bit equality of two tensors of one dtype and shape (signed zeros and NaN payloads included), naming the first
    element that differs."""
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
    a, b = got.contiguous().view(view).reshape(-1), ref.to(got.device).contiguous().view(view).reshape(-1)
    for i0 in range(0, a.numel(), 1 << 27):
        bad = a[i0:i0 + (1 << 27)] != b[i0:i0 + (1 << 27)]
        if bool(bad.any()):
            i = i0 + int(bad.nonzero()[0, 0])
            assert False, '%s: %d elements differ; the first is element %d (row %s): %r against %r' % (
                what, int((a != b).sum()), i, i // got.shape[-1] if got.dim() > 1 else '-', got.reshape(-1)[i].item(),
                ref.reshape(-1)[i].item())


def assert_exact_zero(t, where):
    """Every element of t is exactly 0: positions whose exact value is 0 (masked rows, keys past the sequence)."""
    t = torch.as_tensor(t).detach()
    bad = ((t != 0) | torch.isnan(t)) if t.is_floating_point() else (t != 0)
    n = int(bad.sum())
    if n:
        first = tuple(int(k) for k in np.unravel_index(int(bad.reshape(-1).nonzero()[0, 0]), tuple(t.shape)))
        assert False, '%s: %d elements that must be exactly 0 are not (the first at %s holds %r)' % (
            where, n, first, float(t[first]))


def heads(x, B, T, H, dh):
    """[B*T, H*dh] -> [B, H, T, dh]: one block per (sequence, head, row)."""
    return x.reshape(B, T, H, dh).transpose(1, 2)


GUARD = 3                       # guard rows before and after every output of guarded()


def guarded(rows, cols, dtype):
    """A poisoned (0xFF bytes) buffer of GUARD + rows + GUARD rows -> (whole buffer, the view handed to the kernel)."""
    buf = torch.empty((rows + 2 * GUARD, cols), dtype=dtype, device='cuda')
    buf.untyped_storage().fill_(0xFF)
    return buf, buf[GUARD:GUARD + rows]


def assert_guards(buf, what):
    poison = torch.empty_like(buf)
    poison.untyped_storage().fill_(0xFF)
    assert_bits_equal(buf[:GUARD], poison[:GUARD], what + ': guard rows before the output')
    assert_bits_equal(buf[-GUARD:], poison[-GUARD:], what + ': guard rows behind the output')


# ---------------------------------------------------------------------------------------------------------------------
# Poisoned outputs.  Inside poisoned_outputs() the floating-point buffers that the launchers of m3p_amd/ops.py allocate
# with torch.empty / torch.empty_like come back filled with 0xFF bytes - NaN in bf16 and fp32 - so an element a kernel
# never writes reads NaN instead of what the caching allocator handed back (often the previous call's output).
# ---------------------------------------------------------------------------------------------------------------------
_POISON_DTYPES = (torch.bfloat16, torch.float16, torch.float32, torch.float64)


def _poison(t):
    # Floating-point buffers only.  Integer and byte buffers are never touched: the cached workspaces (ops._WGRAD_WS,
    # ops._CE_WS) and the tile queue hold counters the kernels rely on, keep words and byte codes are read as bits, and an
    # index or counter of 0xFF bytes can send a kernel out of bounds.
    if t.dtype in _POISON_DTYPES and t.is_cuda and t.numel():
        t.untyped_storage().fill_(0xFF)
    return t


class _PoisonTorch:
    """Stands in for the ``torch`` module inside m3p_amd/ops.py; everything but empty / empty_like is torch's own."""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        return getattr(self._real, name)

    def empty(self, *args, **kw):
        return _poison(self._real.empty(*args, **kw))

    def empty_like(self, *args, **kw):
        return _poison(self._real.empty_like(*args, **kw))


@contextlib.contextmanager
def poisoned_outputs(device='cuda'):
    """ops.py launchers hand back NaN-filled outputs until a kernel writes them.  Use it around launchers whose floating-
    point allocations are all returned to the caller (gemm_nt, gemm_nt_fp8, attn_fwd / attn_bwd, layernorm_fwd / _bwd,
    ce_fwd_bwd).  The weight-gradient workspace of this device and stream is created before the proxy goes in (under the
    key the launchers look it up with), so that it never comes from the proxy; it is a byte buffer of counters and partial
    tiles, which _poison leaves alone in any case, and so are the cross-entropy workspace and the tile queue."""
    from m3p_amd import ops
    dev = torch.device(device)
    ops._wgrad_workspace(torch.device(dev.type, torch.cuda.current_device() if dev.index is None else dev.index))
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, 'torch', _PoisonTorch(torch))
        yield


@pytest.fixture
def poison_outputs():
    """poisoned_outputs() around a whole test: ``@pytest.mark.usefixtures('poison_outputs')`` with this name imported."""
    with poisoned_outputs():
        yield


@contextlib.contextmanager
def gemm_schedule(grid=0, queue_slots=0):
    """The two process-wide schedule switches of the persistent GEMMs (include/m3p_hip.h) around a block of launches:
    m3p_set_persistent_grid(grid) and, with queue_slots > 0, a tile-queue ring of that many slots.  Yields the ring's counter
    pool (int32 [queue_slots * 8], one slot of eight per queued launch) or None.  Both setters want no GEMM in flight, so the
    device is synchronised before they are set and before they are put back (grid 0, queue off) - whatever the block did.
    A queue that is armed on entry (a suite started with M3P_TILE_QUEUE=1) is an error: the block would not test what it says."""
    from m3p_amd import ops, lib as L
    lib = L.load()
    dev = torch.cuda.current_device()
    assert dev not in ops._TILE_QUEUE, 'a tile queue is armed already (M3P_TILE_QUEUE?): the schedule tests need the default schedule'
    torch.cuda.synchronize()
    try:
        L.check(lib.m3p_set_persistent_grid(int(grid)), 'm3p_set_persistent_grid')
        if queue_slots > 0:
            ops.set_tile_queue(True, slots=int(queue_slots))
        yield ops._TILE_QUEUE[dev] if queue_slots > 0 else None
    finally:
        torch.cuda.synchronize()
        L.check(lib.m3p_set_persistent_grid(0), 'm3p_set_persistent_grid')
        ops.set_tile_queue(False)


def max_abs(a, b):
    return float((torch.as_tensor(a).detach().double().cpu() - torch.as_tensor(b).detach().double().cpu()).abs().max())


def randn_bf16(shape, seed, scale=1.0, device='cuda'):
    """bf16-representable random tensor: returns (device bf16 tensor, CPU fp32 copy of the same values)."""
    rs = np.random.RandomState(seed)
    t = torch.from_numpy(rs.standard_normal(shape).astype(np.float32) * scale).to(BF16)
    return t.to(device), t.float()


def randn_f32(shape, seed, scale=1.0, device='cuda'):
    rs = np.random.RandomState(seed)
    t = torch.from_numpy(rs.standard_normal(shape).astype(np.float32) * scale)
    return t.to(device), t.clone()


def encoder_keep_masks(model, step, B, T, R, p, p_attn):
    """The dropout keep masks the encoder kernels draw for forward pass number ``step`` of ``model``, rebuilt on
    the host with the NumPy twin of the device RNG (m3p_amd/rng.py) in the layout oracle.ref_cpu.jointfwd's
    ``keeps`` takes.  Element indices: image rows (r*B + b)*d + c, everything else (b*S + s)*d + c, attention
    probabilities ((b*H + h)*S + q)*S + k."""
    from m3p_amd import functional as Fn, rng
    S, d, H = R + T, model.dim, model.n_heads
    seed = lambda kind, i=0: rng.stream_seed(model.base_seed, step, Fn._site(kind, i))   # noqa: E731
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))                               # noqa: E731
    keeps = {'emb': t(rng.keep_mask(B * S * d, seed('emb'), p, (B, S, d)))}
    if R:
        keeps['img'] = t(rng.keep_mask(R * B * d, seed('img'), p, (R, B, d)).transpose(1, 0, 2))
    for i in range(model.n_layers):
        keeps[('attn_p', i)] = t(rng.keep_mask(B * H * S * S, seed('attn_p', i), p_attn, (B, H, S, S)))
        keeps[('attn_out', i)] = t(rng.keep_mask(B * S * d, seed('attn_out', i), p, (B, S, d)))
        keeps[('ffn', i)] = t(rng.keep_mask(B * S * d, seed('ffn', i), p, (B, S, d)))
    return keeps
