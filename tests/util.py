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


def assert_exact_zero(t, where):
    """Every element of t is exactly 0: positions whose exact value is 0 (masked rows, keys past the sequence)."""
    t = torch.as_tensor(t).detach()
    bad = ((t != 0) | torch.isnan(t)) if t.is_floating_point() else (t != 0)
    n = int(bad.sum())
    if n:
        first = tuple(int(k) for k in np.unravel_index(int(bad.reshape(-1).nonzero()[0, 0]), tuple(t.shape)))
        assert False, '%s: %d elements that must be exactly 0 are not (the first at %s holds %r)' % (
            where, n, first, float(t[first]))


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
