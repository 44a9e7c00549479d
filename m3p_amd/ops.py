"""Raw (non-autograd) launchers: one Python function per C-ABI entry point.

Each allocates its outputs with torch (device memory + caching allocator are plumbing),
passes raw device pointers and the current HIP stream across the C ABI and raises on any
error code.  The autograd layer (m3p_amd/functional.py) composes these."""
import ctypes as C
import os

import torch

from . import lib as L
from . import rng

BF16 = torch.bfloat16
_DEBUG_CHECKS = os.environ.get('M3P_DEBUG_CHECKS') == '1'      # host-synchronising consistency checks (tests, debugging)

# bench.py sets this to a dict to time individual GEMM launches with HIP events recorded on
# the launch stream: {(kind, M, N, K): [(start_event, end_event), ...]}
PROFILE = None
_EPI_NAMES = ['gemm_nt/none', 'gemm_nt/bias', 'gemm_nt/bias_gelu', 'gemm_nt/bias_drop_res', 'gemm_nt/res',
              'gemm_nt/dgelu', 'gemm_nt/mul', 'gemm_nt/mulq', 'gemm_nt/bias_geluq', 'gemm_nt/bias_lse']


PROFILE_ONLY = None     # if set: the one (kind, M, N, K) instance that is timed (bench.py: the dominant kernel)


def _prof_begin(key=None):
    if PROFILE is None or (PROFILE_ONLY is not None and key != PROFILE_ONLY):
        return None
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def _prof_end(e0, key):
    if e0 is not None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        PROFILE.setdefault(key, []).append((e0, e1))


def _chk_bf16(*ts):
    for t in ts:
        if t is not None:
            assert t.dtype == BF16 and t.is_cuda, (t.dtype, t.device)


def gemm_nt(a, w, epilogue=L.EPI_NONE, bias=None, aux=None, out=None, out2=None, colsum=None,
            scale_cols=0, scale=1.0, alpha=1.0, seed=0, p_drop=0.0, n=None, out8=None, scale8=None, amax8=None, out8_bf8=False,
            rng_rows=None, row_ref=None):
    """C[M,N] = epi(a[M,K] @ w[N,K]^T).  a, w bf16 (row pitch = stride(0)); returns C (bf16).
    ``n`` restricts the number of output columns (rows of w) used.
    rng_rows (EPI_BIAS_DROP_RES on gathered rows): int32 [M], the number of each row in the full tensor the dropout stream
    is indexed by - the launch then drops exactly the elements the launch over all rows drops in those rows.
    out8 (EPI_BIAS_GELUQ / EPI_MULQ): uint8 [M, N] that receives the 8-bit copy of C - sat(C * scale8) in e4m3, or e5m2 with
    out8_bf8 - for the fp8 product that consumes C; amax8 (fp32 [1], zeroed by the caller) is raised to max |C|.
    row_ref (EPI_BIAS_LSE): the rows' {shift, target} pairs of ``ce_shift_target`` - the shifted-exponential form of the
    epilogue: C = bf16(exp(a w^T + bias - shift)), 0 at the target and pad columns, out2 = float32 [N / 64, M] block sums."""
    M, K = a.shape
    N = w.shape[0] if n is None else n
    if epilogue == L.EPI_MULQ:     # aux = the byte codes of gelu_fwd_gq for this [M, N], in the GEMM's fragment order
        _chk_bf16(a, w, out)
        assert aux is not None and aux.dtype == torch.uint8 and aux.is_contiguous() and aux.numel() == M * N
    elif epilogue == L.EPI_BIAS_LSE:        # out2 = float32 [N / 64, M, 2] block statistics; scale_cols = V (valid columns)
        _chk_bf16(a, w, out)
        assert out2 is not None and out2.dtype == torch.float32 and out2.is_contiguous()
        assert out2.numel() == (N // 64) * M * (2 if row_ref is None else 1)
        assert bias is not None and 0 < scale_cols <= N
        assert row_ref is None or (row_ref.dtype == torch.int32 and row_ref.is_cuda and row_ref.is_contiguous() and row_ref.numel() == 2 * M)
    elif epilogue == L.EPI_BIAS_GELUQ:      # out2 = where those codes go (uint8 [M * N]); C = gelu(a w^T + bias)
        _chk_bf16(a, w, out)
        assert out2 is not None and out2.dtype == torch.uint8 and out2.is_contiguous() and out2.numel() == M * N and bias is not None
    else:
        _chk_bf16(a, w, aux, out, out2)
    assert w.shape[1] == K and a.stride(1) == 1 and w.stride(1) == 1
    if out is None:
        out = torch.empty((M, N), dtype=BF16, device=a.device)
    ep = L.Epilogue()
    ep.bias = L.ptr(bias)
    ep.aux = L.ptr(aux)
    ep.out2 = L.ptr(out2)
    ep.colsum = L.ptr(colsum)
    ep.ld_aux = aux.stride(0) if (aux is not None and epilogue != L.EPI_MULQ) else 0
    ep.ld_out2 = out2.stride(0) if (out2 is not None and epilogue not in (L.EPI_BIAS_GELUQ, L.EPI_BIAS_LSE)) else 0
    ep.scale_cols = scale_cols
    if epilogue == L.EPI_BIAS_LSE:
        ep.ld_out2, ep.scale_cols = scale_cols, 0
    ep.scale = scale
    ep.alpha = alpha
    ep.seed = seed
    ep.thresh24 = L.thresh24(p_drop)
    ep.inv_keep = 1.0 / (1.0 - p_drop) if p_drop > 0 else 1.0
    if bias is not None:
        assert bias.dtype == torch.float32
    if rng_rows is not None:
        assert epilogue == L.EPI_BIAS_DROP_RES and rng_rows.dtype == torch.int32 and rng_rows.is_cuda \
            and rng_rows.is_contiguous() and rng_rows.numel() == M
        ep.rng_rows = rng_rows.data_ptr()
    if row_ref is not None:
        assert epilogue == L.EPI_BIAS_LSE
        ep.row_ref = row_ref.data_ptr()
    if out8 is not None:
        assert epilogue in (L.EPI_BIAS_GELUQ, L.EPI_MULQ) and out8.dtype == torch.uint8 and out8.shape == (M, N) and out8.stride(1) == 1
        ep.out8, ep.ld_out8, ep.out8_bf8 = out8.data_ptr(), out8.stride(0), 1 if out8_bf8 else 0
        ep.scale8, ep.amax8 = L.ptr(scale8), L.ptr(amax8)
    e0 = _prof_begin((_EPI_NAMES[epilogue], M, N, K))
    rc = L.load().m3p_gemm_nt_bf16(a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), out.data_ptr(),
                                   out.stride(0), M, N, K, epilogue, C.byref(ep), L.stream())
    L.check(rc, 'm3p_gemm_nt_bf16')
    _prof_end(e0, (_EPI_NAMES[epilogue], M, N, K))
    return out


def quant_fp8(x, scale=None, amax=None, bf8=False, out=None):
    """x bf16 [rows, cols] -> 8-bit [rows, cols] (uint8 storage): fp8 e4m3, or bf8 e5m2 when ``bf8``; multiplied by the
    device scalar ``scale`` first, saturating; ``amax`` (device fp32 scalar, zeroed by the caller) is raised to max |x|."""
    _chk_bf16(x)
    rows, cols = x.shape
    assert x.stride(1) == 1
    if out is None:
        out = torch.empty((rows, cols), dtype=torch.uint8, device=x.device)
    rc = L.load().m3p_quant_fp8(x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), rows, cols, L.ptr(scale), L.ptr(amax),
                                1 if bf8 else 0, L.stream())
    L.check(rc, 'm3p_quant_fp8')
    return out


def quant_fp8_batch(desc, n_desc, blocks_per_matrix=512):
    """Many contiguous bf16 matrices -> e4m3 in one launch; desc int64 [n_desc, 5] on the device (csrc/optim.hip)."""
    L.check(L.load().m3p_quant_fp8_batch(desc.data_ptr(), n_desc, blocks_per_matrix, L.stream()), 'm3p_quant_fp8_batch')


def gemm_nt_fp8(a8, w8, epilogue=L.EPI_NONE, a_is_bf8=False, descale_a=None, descale_b=None, bias=None, aux=None, out=None,
                colsum=None, scale_cols=0, scale=1.0, seed=0, p_drop=0.0):
    """C[M,N] (bf16) = epi(descale_a * descale_b * a8[M,K] @ w8[N,K]^T): 8-bit operands (uint8 storage) from quant_fp8,
    descale_* device fp32 scalars (1 / the quantisation scales)."""
    assert a8.dtype == torch.uint8 and w8.dtype == torch.uint8 and a8.is_cuda and w8.is_cuda
    M, K = a8.shape
    N = w8.shape[0]
    assert w8.shape[1] == K and a8.stride(1) == 1 and w8.stride(1) == 1
    _chk_bf16(aux, out)
    if out is None:
        out = torch.empty((M, N), dtype=BF16, device=a8.device)
    ep = L.Epilogue()
    ep.bias = L.ptr(bias)
    ep.aux = L.ptr(aux)
    ep.colsum = L.ptr(colsum)
    ep.ld_aux = aux.stride(0) if aux is not None else 0
    ep.scale_cols = scale_cols
    ep.scale = scale
    ep.alpha = 1.0
    ep.seed = seed
    ep.thresh24 = L.thresh24(p_drop)
    ep.inv_keep = 1.0 / (1.0 - p_drop) if p_drop > 0 else 1.0
    ep.descale_a = L.ptr(descale_a)
    ep.descale_b = L.ptr(descale_b)
    e0 = _prof_begin(('gemm_fp8/' + _EPI_NAMES[epilogue].split('/')[1], M, N, K))
    rc = L.load().m3p_gemm_nt_fp8(a8.data_ptr(), a8.stride(0), 1 if a_is_bf8 else 0, w8.data_ptr(), w8.stride(0), out.data_ptr(),
                                  out.stride(0), M, N, K, epilogue, C.byref(ep), L.stream())
    L.check(rc, 'm3p_gemm_nt_fp8')
    _prof_end(e0, ('gemm_fp8/' + _EPI_NAMES[epilogue].split('/')[1], M, N, K))
    return out


def gemm_nt_streamk(a, w, out_f32, alpha=1.0):
    """out_f32[M,N] (fp32) += alpha * a[M,K] @ w[N,K]^T  (stream-K, fp32 atomics)."""
    _chk_bf16(a, w)
    M, K = a.shape
    N = w.shape[0]
    assert w.shape[1] == K and out_f32.dtype == torch.float32 and out_f32.shape == (M, N)
    e0 = _prof_begin(('gemm_nt/streamk', M, N, K))
    rc = L.load().m3p_gemm_nt_streamk_f32(a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), out_f32.data_ptr(),
                                          out_f32.stride(0), M, N, K, alpha, L.stream())
    L.check(rc, 'm3p_gemm_nt_streamk_f32')
    _prof_end(e0, ('gemm_nt/streamk', M, N, K))
    return out_f32


def gemm_nn_streamk(a, w_kn, out_f32, alpha=1.0):
    """out_f32[M,N] (fp32) += alpha * a[M,K] @ w_kn[:K]  with w_kn [k_valid <= K, N] row-major (stream-K, fp32
    atomics); columns k_valid..K of ``a`` must be zeros."""
    _chk_bf16(a, w_kn)
    M, K = a.shape
    k_valid, N = w_kn.shape
    assert k_valid <= K and out_f32.dtype == torch.float32 and out_f32.shape == (M, N) and w_kn.stride(1) == 1
    e0 = _prof_begin(('gemm_nt/streamk', M, N, K))
    rc = L.load().m3p_gemm_nn_streamk_f32(a.data_ptr(), a.stride(0), w_kn.data_ptr(), w_kn.stride(0), k_valid,
                                          out_f32.data_ptr(), out_f32.stride(0), M, N, K, alpha, L.stream())
    L.check(rc, 'm3p_gemm_nn_streamk_f32')
    _prof_end(e0, ('gemm_nt/streamk', M, N, K))
    return out_f32


def gemm_nn(a, w_kn, out_f32, alpha=1.0, k_rows_readable=None):
    """out_f32[M,N] (fp32) += alpha * a[M,K] @ w_kn[:K].  Whole-tile shapes whose second operand is readable (finite) for all
    K rows - k_rows_readable >= K: the rows behind w_kn's own k_valid are memory the caller vouches for, e.g. the arena
    behind the vocabulary matrix - run on the four-wave kernel (m3p_gemm_nn_w4_f32, no atomics); everything else on the
    stream-K form."""
    _chk_bf16(a, w_kn)
    M, K = a.shape
    k_valid, N = w_kn.shape
    if (k_rows_readable or k_valid) >= K and M % 256 == 0 and N % 256 == 0 and K % 64 == 0 and K >= 4096:
        assert out_f32.dtype == torch.float32 and out_f32.shape == (M, N) and w_kn.stride(1) == 1
        e0 = _prof_begin(('gemm_nn/w4', M, N, K))
        ws = _wgrad_workspace(a.device)
        rc = L.load().m3p_gemm_nn_w4_f32(a.data_ptr(), a.stride(0), w_kn.data_ptr(), w_kn.stride(0), out_f32.data_ptr(),
                                         out_f32.stride(0), M, N, K, alpha, ws.data_ptr(), ws.numel(), L.stream())
        if rc == 0:
            _prof_end(e0, ('gemm_nn/w4', M, N, K))
            return out_f32
        if rc != -2:
            L.check(rc, 'm3p_gemm_nn_w4_f32')
    return gemm_nn_streamk(a, w_kn, out_f32, alpha)


_WGRAD_WS = {}     # (device index, stream) -> workspace tensor of the four-wave weight-gradient kernel


def _wgrad_workspace(device):
    """One scratch buffer per (device, stream): launches on one stream are ordered, so they can share it."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _WGRAD_WS.get(key)
    if ws is None:
        ws = _WGRAD_WS[key] = torch.empty(int(L.load().m3p_gemm_wgrad_workspace_bytes()), dtype=torch.uint8, device=device)
    return ws


def gemm_wgrad(dy, x, dw, alpha=1.0, n=None, k=None, dw_is_zero=False, report_store=False, must_store=False, bias=None):
    """_gemm_wgrad; bias = (w fp32 [M], bsum fp32 [>= N]): a whole-tile launch also leaves bsum[:N] = w @ dy (gemm_wgrad_bias: the
    same kernel through the entry points of this call) and the result becomes (result, whether bsum was written)."""
    if bias is None:
        return _gemm_wgrad(dy, x, dw, alpha, n, k, dw_is_zero, report_store, must_store)
    w, bsum = bias
    assert w.dtype == bsum.dtype == torch.float32 and w.is_contiguous() and bsum.is_contiguous()
    assert w.numel() == dy.shape[0] and bsum.numel() >= (dy.shape[1] if n is None else n)
    lib = L.load()
    armed = lib.m3p_gemm_wgrad_bias_arm(w.data_ptr(), bsum.data_ptr()) == 0        # (anything else: declined)
    try:
        res = _gemm_wgrad(dy, x, dw, alpha, n, k, dw_is_zero, report_store, must_store)
    finally:
        took = armed and lib.m3p_gemm_wgrad_bias_arm(None, None) == 1
    return res, took


def _gemm_wgrad(dy, x, dw, alpha=1.0, n=None, k=None, dw_is_zero=False, report_store=False, must_store=False):
    """dw[N,K] (fp32) += alpha * dy[M,N]^T @ x[M,K].  dw_is_zero: the caller knows dw[:N, :K] to hold zeros - shapes dealt out
    as whole tiles (the vocabulary matrix) are then stored instead of accumulated with atomics; same result.  must_store: dw is
    only LOGICALLY zero (the arena's lazily zeroed range): a launcher that declines the store raises here instead of
    accumulating onto what the buffer physically holds."""
    _chk_bf16(dy, x)
    assert dw.dtype == torch.float32 and dw.stride(-1) == 1
    M = dy.shape[0]
    N = dy.shape[1] if n is None else n
    K = x.shape[1] if k is None else k
    assert x.shape[0] == M and dw.shape[0] >= N and dw.shape[1] >= K
    e0 = _prof_begin(('gemm_wgrad', M, N, K))
    ws = _wgrad_workspace(dy.device)
    if dw_is_zero:
        rc = L.load().m3p_gemm_wgrad_store_bf16(dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), dw.data_ptr(),
                                                dw.stride(0), M, N, K, alpha, ws.data_ptr(), ws.numel(), L.stream())
        if rc == 0:
            _prof_end(e0, ('gemm_wgrad', M, N, K))
            return True if report_store else dw
        if rc != -2:        # (M3P_ENOTIMPL: not a whole-tile shape - accumulate below)
            L.check(rc, 'm3p_gemm_wgrad_store_bf16')
        if must_store:
            raise L.M3PError('m3p_gemm_wgrad_store_bf16 declined (M3P_ENOTIMPL) a store the caller depends on: dw is not physically zero')
    rc = L.load().m3p_gemm_wgrad_bf16(dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), dw.data_ptr(),
                                      dw.stride(0), M, N, K, alpha, ws.data_ptr(), ws.numel(), L.stream())
    L.check(rc, 'm3p_gemm_wgrad_bf16')
    _prof_end(e0, ('gemm_wgrad', M, N, K))
    return False if report_store else dw


def gemm_wgrad_bias(dy, x, dw, w, bsum, alpha=1.0, n=None, k=None, store=False):
    """The whole-tile weight gradient that also leaves bsum[:N] = w @ dy (w fp32 [M], bsum fp32 [>= N]): dw[N,K] = (store) or +=
    alpha * dy^T @ x, bit-identical to gemm_wgrad.  Returns False - nothing launched, nothing written - where the launcher does
    not run the whole-tile schedule (M3P_ENOTIMPL); the caller then takes gemm_wgrad and a column-sum pass."""
    _chk_bf16(dy, x)
    assert dw.dtype == torch.float32 and dw.stride(-1) == 1
    M = dy.shape[0]
    N = dy.shape[1] if n is None else n
    K = x.shape[1] if k is None else k
    assert x.shape[0] == M and dw.shape[0] >= N and dw.shape[1] >= K
    assert w.dtype == bsum.dtype == torch.float32 and w.is_contiguous() and bsum.is_contiguous() and w.numel() == M and bsum.numel() >= N
    e0 = _prof_begin(('gemm_wgrad_bias', M, N, K))
    rc = L.load().m3p_gemm_wgrad_bias_bf16(dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), dw.data_ptr(), dw.stride(0),
                                           M, N, K, alpha, w.data_ptr(), bsum.data_ptr(), int(bool(store)), L.stream())
    if rc == -2:
        return False
    L.check(rc, 'm3p_gemm_wgrad_bias_bf16')
    _prof_end(e0, ('gemm_wgrad_bias', M, N, K))
    return True


def gemm_wgrad_pair(dy_a, x_a, dw_a, dy_b, x_b, dw_b, alpha=1.0):
    """dw_a += alpha * dy_a^T @ x_a and dw_b += alpha * dy_b^T @ x_b (same M) in one launch where the shapes allow."""
    _chk_bf16(dy_a, x_a, dy_b, x_b)
    assert dw_a.dtype == torch.float32 and dw_b.dtype == torch.float32 and dw_a.stride(-1) == 1 and dw_b.stride(-1) == 1
    M = dy_a.shape[0]
    assert x_a.shape[0] == M and dy_b.shape[0] == M and x_b.shape[0] == M
    Na, Ka, Nb, Kb = dy_a.shape[1], x_a.shape[1], dy_b.shape[1], x_b.shape[1]
    assert dw_a.shape[0] >= Na and dw_a.shape[1] >= Ka and dw_b.shape[0] >= Nb and dw_b.shape[1] >= Kb
    e0 = _prof_begin(('gemm_wgrad_pair', M, Na + Nb, Ka))
    ws = _wgrad_workspace(dy_a.device)
    rc = L.load().m3p_gemm_wgrad_pair_bf16(dy_a.data_ptr(), dy_a.stride(0), x_a.data_ptr(), x_a.stride(0), dw_a.data_ptr(), dw_a.stride(0),
                                           Na, Ka, dy_b.data_ptr(), dy_b.stride(0), x_b.data_ptr(), x_b.stride(0), dw_b.data_ptr(),
                                           dw_b.stride(0), Nb, Kb, M, alpha, ws.data_ptr(), ws.numel(), L.stream())
    L.check(rc, 'm3p_gemm_wgrad_pair_bf16')
    _prof_end(e0, ('gemm_wgrad_pair', M, Na + Nb, Ka))


def wgrad_group_takes(dy, x, dw):
    """Whether dw += dy^T @ x can be an item of a grouped whole-tile launch (the conditions of m3p_gemm_wgrad_group_bf16 that
    one product decides alone; the launcher checks them again, and the summed tile count)."""
    M, N = dy.shape
    K = x.shape[1]
    return (M % 64 == 0 and M >= 4096 and N % 256 == 0 and K % 256 == 0 and dy.stride(1) == 1 and x.stride(1) == 1
            and dw.stride(-1) == 1 and dy.stride(0) % 8 == 0 and x.stride(0) % 8 == 0 and dw.stride(0) % 4 == 0
            and dw.stride(0) >= K and dy.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0 and dw.data_ptr() % 16 == 0)


def wgrad_group_place(tiles, workgroups):
    """The grouped launch's placement for items of tiles = [(tiles_i, tiles_j), ...] on `workgroups` workgroups (host only):
    a list with (item, tile row, tile column) or None per workgroup; workgroup w runs on XCD w % 8."""
    n = len(tiles)
    ti = (C.c_int * n)(*[t[0] for t in tiles])
    tj = (C.c_int * n)(*[t[1] for t in tiles])
    place = (C.c_uint32 * max(workgroups, 1))()
    L.check(L.load().m3p_gemm_wgrad_group_place(ti, tj, n, workgroups, place), 'm3p_gemm_wgrad_group_place')
    return [None if p == 0xffffffff else (p >> 16, (p >> 8) & 255, p & 255) for p in place]


def gemm_wgrad_group(items, alpha=1.0):
    """dw += alpha * dy^T @ x for every (dy, x, dw) of `items` (at most lib.WGRAD_GROUP_MAX, one shared M) in ONE launch with
    one workgroup per 256 x 256 output tile over all of M: no partial tiles, no reduction.  Returns False - nothing launched,
    nothing written - when the launcher declines (M3P_ENOTIMPL: a shape that is not whole tiles, more tiles than CUs): the
    caller sends the products through gemm_wgrad / gemm_wgrad_pair."""
    n = len(items)
    assert 1 <= n <= L.WGRAD_GROUP_MAX
    M = items[0][0].shape[0]
    arr = (L.WgradItem * n)()
    for k, (dy, x, dw) in enumerate(items):
        _chk_bf16(dy, x)
        assert dw.dtype == torch.float32 and dw.stride(-1) == 1 and dy.stride(1) == 1 and x.stride(1) == 1
        assert dy.shape[0] == M and x.shape[0] == M and dw.shape[0] >= dy.shape[1] and dw.shape[1] >= x.shape[1]
        arr[k] = L.WgradItem(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), dy.stride(0), x.stride(0), dw.stride(0),
                             dy.shape[1], x.shape[1])
    key = ('gemm_wgrad_group', M, sum(dy.shape[1] * x.shape[1] for dy, x, _ in items) // 256, 256)     # (2 M N K = the group's flops)
    e0 = _prof_begin(key)
    rc = L.load().m3p_gemm_wgrad_group_bf16(arr, n, M, alpha, L.stream())
    if rc == -2:
        return False
    L.check(rc, 'm3p_gemm_wgrad_group_bf16')
    _prof_end(e0, key)
    return True


def layernorm_fwd(x, gamma, beta, rowmask=None, eps=1e-12):
    _chk_bf16(x)
    rows, d = x.shape
    assert x.is_contiguous()
    y = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    rc = L.load().m3p_layernorm_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), L.ptr(rowmask), y.data_ptr(),
                                    mean.data_ptr(), rstd.data_ptr(), rows, d, eps, L.stream())
    L.check(rc, 'm3p_layernorm_fwd')
    return y, mean, rstd


def layernorm_bwd(dy_a, dy_b, x, gamma, mean, rstd, rowmask, dgamma, dbeta, dbias_drop=None,
                  want_drop=False, seed=0, p_drop=0.0, rng_rows=None):
    """Returns (dx, dx_drop).  dx_drop is dx pushed through the residual-branch dropout
    (None unless want_drop).  dgamma/dbeta/dbias_drop are accumulated in place (fp32).
    rng_rows: int32 [rows], the rows' numbers in the full tensor the dropout stream is indexed by (see gemm_nt)."""
    _chk_bf16(dy_a, dy_b, x)
    rows, d = x.shape
    if rng_rows is not None:
        assert rng_rows.dtype == torch.int32 and rng_rows.is_cuda and rng_rows.is_contiguous() and rng_rows.numel() == rows
    dx = torch.empty_like(x)
    dx_drop = torch.empty_like(x) if want_drop else None
    rc = L.load().m3p_layernorm_bwd_rows(dy_a.data_ptr(), L.ptr(dy_b), x.data_ptr(), gamma.data_ptr(), mean.data_ptr(),
                                         rstd.data_ptr(), L.ptr(rowmask), dx.data_ptr(), L.ptr(dx_drop),
                                         dgamma.data_ptr(), dbeta.data_ptr(), L.ptr(dbias_drop), rows, d, seed,
                                         L.thresh24(p_drop), 1.0 / (1.0 - p_drop) if p_drop > 0 else 1.0,
                                         L.ptr(rng_rows), L.stream())
    L.check(rc, 'm3p_layernorm_bwd_rows')
    return dx, dx_drop


def attn_fwd(qkv, keylen, B, S, H, dh, seed=0, p_drop=0.0, want_mask=False):
    """qkv bf16 [B*S, 3*H*dh] -> (ctx bf16 [B*S, H*dh], lse fp32 [B,H,S]) and, with want_mask, the dropout
    keep-bit words for attn_bwd (None when p_drop == 0)."""
    _chk_bf16(qkv)
    assert qkv.is_contiguous() and qkv.shape == (B * S, 3 * H * dh) and keylen.dtype == torch.int32
    ctx = torch.empty((B * S, H * dh), dtype=BF16, device=qkv.device)
    lse = torch.empty((B, H, S), dtype=torch.float32, device=qkv.device)
    mask = None
    if want_mask and p_drop > 0:
        nt = (S + 15) // 16
        mask = torch.empty((B * H, nt, nt, 4), dtype=torch.int64, device=qkv.device)
    rc = L.load().m3p_attn_fwd(qkv.data_ptr(), keylen.data_ptr(), ctx.data_ptr(), lse.data_ptr(), L.ptr(mask), B, S, H, dh,
                               seed, L.thresh24(p_drop), 1.0 / (1.0 - p_drop) if p_drop > 0 else 1.0, L.stream())
    L.check(rc, 'm3p_attn_fwd')
    return (ctx, lse, mask) if want_mask else (ctx, lse)


def attn_bwd(qkv, keylen, ctx, dctx, lse, B, S, H, dh, dbias_qkv=None, seed=0, p_drop=0.0, keepmask=None):
    """dqkv of attn_fwd.  With dropout on, keepmask = the words attn_fwd(..., want_mask=True) returned (required)."""
    _chk_bf16(qkv, ctx, dctx)
    assert dctx.is_contiguous() and ctx.is_contiguous()
    assert p_drop == 0 or keepmask is not None, 'attention backward with dropout needs the keep words of the forward pass'
    dqkv = torch.empty_like(qkv)
    rc = L.load().m3p_attn_bwd(qkv.data_ptr(), keylen.data_ptr(), ctx.data_ptr(), dctx.data_ptr(), lse.data_ptr(),
                               L.ptr(keepmask), dqkv.data_ptr(), L.ptr(dbias_qkv), B, S, H, dh, 1.0 / (dh ** 0.5), seed,
                               L.thresh24(p_drop), 1.0 / (1.0 - p_drop) if p_drop > 0 else 1.0, L.stream())
    L.check(rc, 'm3p_attn_bwd')
    return dqkv


def attn_query_fwd(q, kv, klen, B, Tq, H, dh, Lk, causal=False, pos0=0, owner=None):
    """Decoder-inference attention: q bf16 [B*Tq, >= H*dh] (scaled), kv bf16 [B, >= Lk, >= 2*H*dh] (keys | values per
    cached position), klen int32 [B] or None -> ctx bf16 [B*Tq, H*dh]  (csrc/decode.hip).
    owner: int32 tensor, [B, >= Lk] (a kv row per (sequence, key): key j of sequence b is read from kv[owner[b, j], j]) or
    [B] (a kv row per sequence); kv then holds any number of rows and every entry of owner must name one of them."""
    _chk_bf16(q, kv)
    assert q.stride(1) == 1 and kv.dim() == 3 and kv.stride(2) == 1 and kv.shape[1] >= Lk
    ctx = torch.empty((B * Tq, H * dh), dtype=BF16, device=q.device)
    if owner is None:
        assert kv.shape[0] == B
        rc = L.load().m3p_attn_query_fwd(q.data_ptr(), q.stride(0), kv.data_ptr(), kv.stride(0), kv.stride(1), L.ptr(klen),
                                         ctx.data_ptr(), B, Tq, H, dh, Lk, 1 if causal else 0, pos0, L.stream())
        L.check(rc, 'm3p_attn_query_fwd')
        return ctx
    assert owner.dtype == torch.int32 and owner.is_cuda and owner.shape[0] == B and owner.dim() in (1, 2)
    assert owner.dim() == 1 or (owner.shape[1] >= Lk and owner.stride(1) == 1)
    if _DEBUG_CHECKS:
        used = owner if owner.dim() == 1 else owner[:, :Lk]
        assert int(used.min()) >= 0 and int(used.max()) < kv.shape[0], 'owner names a row outside the key / value tensor'
    rc = L.load().m3p_attn_query_owner_fwd(q.data_ptr(), q.stride(0), kv.data_ptr(), kv.stride(0), kv.stride(1), L.ptr(klen),
                                           ctx.data_ptr(), B, Tq, H, dh, Lk, 1 if causal else 0, pos0, owner.data_ptr(),
                                           owner.stride(0), 1 if owner.dim() == 2 else 0, L.stream())
    L.check(rc, 'm3p_attn_query_owner_fwd')
    return ctx


_ENOTIMPL = -2          # M3P_ENOTIMPL of include/m3p_hip.h


def vocab_select_max_k():
    """VS_MAX_K of csrc/select.hip: the most entries per sentence m3p_vocab_select returns."""
    return int(L.load().m3p_vocab_select_max_k())


def _plan_takes(plan, *shape):
    """A launcher's plan as a yes or no: False where it would answer M3P_ENOTIMPL; a malformed shape raises."""
    rc = getattr(L.load(), plan)(*shape)
    if rc == _ENOTIMPL:
        return False
    L.check(rc, plan)
    return True


def vocab_select_takes(n, V, ld, beam, k):
    """Does the launcher of vocab_select take the shape?  (False: it would answer M3P_ENOTIMPL; a malformed one raises.)"""
    return _plan_takes('m3p_vocab_select_plan', n, V, ld, beam, k)


def vocab_select(logits, V, beam_scores, beam, k):
    """Word selection of a decoding step (csrc/select.hip): logits bf16 [n, ld >= V] (n = bs * beam rows, columns past V
    hold anything), beam_scores fp32 [n] or None (zeros) -> (scores fp32 [bs, k], flat_idx int64 [bs, k], lse fp32 [n]):
    lse = the rows' log-sum-exp over V columns, the score of (row r, word w) = (float(logits[r, w]) - lse[r]) + beam_scores[r]
    in fp32, and per sentence the first k of its beam * V entries by score descending, beam ascending, logit descending, word
    ascending, flat_idx = beam * V + word.  None when the launcher does not take the shape (M3P_ENOTIMPL: k > 16, beam > 64)."""
    _chk_bf16(logits)
    assert logits.dim() == 2 and logits.stride(1) == 1
    n = logits.shape[0]
    assert n % beam == 0 and logits.shape[1] >= V
    if beam_scores is not None:
        assert beam_scores.dtype == torch.float32 and beam_scores.is_cuda and beam_scores.is_contiguous() and beam_scores.numel() == n
    lib = L.load()
    rc = lib.m3p_vocab_select_plan(n, V, logits.stride(0), beam, k)
    if rc == _ENOTIMPL:
        return None
    L.check(rc, 'm3p_vocab_select_plan')
    bs = n // beam
    dev = logits.device
    ws_bytes = lib.m3p_vocab_select_workspace_bytes(n, V, k)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    scores = torch.empty((bs, k), dtype=torch.float32, device=dev)
    flat_idx = torch.empty((bs, k), dtype=torch.int64, device=dev)
    lse = torch.empty((n,), dtype=torch.float32, device=dev)
    rc = lib.m3p_vocab_select(logits.data_ptr(), logits.stride(0), n, V, L.ptr(beam_scores), beam, k, ws.data_ptr(), ws_bytes,
                              scores.data_ptr(), flat_idx.data_ptr(), lse.data_ptr(), L.stream())
    L.check(rc, 'm3p_vocab_select')
    return scores, flat_idx, lse


def vocab_select_wide_max_k():
    """VSB_MAX_K of csrc/select.hip: the most entries per sentence m3p_vocab_select_wide returns."""
    return int(L.load().m3p_vocab_select_wide_max_k())


def vocab_select_wide_takes(n, V, ld, beam, k):
    """Does the launcher of vocab_select_wide take the shape?  (False: it would answer M3P_ENOTIMPL; a malformed one raises.)"""
    return _plan_takes('m3p_vocab_select_wide_plan', n, V, ld, beam, k)


def vocab_select_wide(logits, V, beam_scores, beam, k):
    """vocab_select for wider beams (csrc/select.hip: m3p_vocab_select_wide): the same arguments, the same contract and the
    same results - (scores fp32 [bs, k], flat_idx int64 [bs, k], lse fp32 [n]) - for 1 <= k <= vocab_select_wide_max_k() (64)
    and beam <= 32, by a count selection of every row's first k words and one sort of the sentence's beam * k entries instead
    of k rounds of a maximum; lse has the bits of vocab_select, and so have scores and flat_idx for k <= 16.  None when the
    launcher does not take the shape (M3P_ENOTIMPL: k > 64, beam > 32); k > V raises."""
    _chk_bf16(logits)
    assert logits.dim() == 2 and logits.stride(1) == 1
    n = logits.shape[0]
    assert n % beam == 0 and logits.shape[1] >= V
    if beam_scores is not None:
        assert beam_scores.dtype == torch.float32 and beam_scores.is_cuda and beam_scores.is_contiguous() and beam_scores.numel() == n
    lib = L.load()
    rc = lib.m3p_vocab_select_wide_plan(n, V, logits.stride(0), beam, k)
    if rc == _ENOTIMPL:
        return None
    L.check(rc, 'm3p_vocab_select_wide_plan')
    bs = n // beam
    dev = logits.device
    ws_bytes = lib.m3p_vocab_select_wide_workspace_bytes(n, V, beam, k)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    scores = torch.empty((bs, k), dtype=torch.float32, device=dev)
    flat_idx = torch.empty((bs, k), dtype=torch.int64, device=dev)
    lse = torch.empty((n,), dtype=torch.float32, device=dev)
    rc = lib.m3p_vocab_select_wide(logits.data_ptr(), logits.stride(0), n, V, L.ptr(beam_scores), beam, k, ws.data_ptr(), ws_bytes,
                                   scores.data_ptr(), flat_idx.data_ptr(), lse.data_ptr(), L.stream())
    L.check(rc, 'm3p_vocab_select_wide')
    return scores, flat_idx, lse


def _vocab_draw(stem, call, logits, V, temperature, seed, top_k, top_p=None):
    """The seeded draws' common course - plan (stem + '_plan'), workspace (stem + '_workspace_bytes'), outputs, call, check:
    -> (words int64 [n], logprob fp32 [n], key fp32 [n]) and, with top_p (a launcher that cuts), cut fp32 [n]; None when the
    plan answers M3P_ENOTIMPL."""
    _chk_bf16(logits)
    assert logits.dim() == 2 and logits.stride(1) == 1 and logits.shape[1] >= V
    n = logits.shape[0]
    lib = L.load()
    rc = getattr(lib, stem + '_plan')(n, V, logits.stride(0), top_k)
    if rc == _ENOTIMPL:
        return None
    L.check(rc, stem + '_plan')
    dev = logits.device
    ws_bytes = getattr(lib, stem + '_workspace_bytes')(n, V, top_k)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    outs = [torch.empty((n,), dtype=torch.int64, device=dev)]
    outs += [torch.empty((n,), dtype=torch.float32, device=dev) for _ in range(2 if top_p is None else 3)]
    cut_args = () if top_p is None else (top_p,)
    rc = getattr(lib, call)(logits.data_ptr(), logits.stride(0), n, V, rng.inv_temperature(temperature), top_k, *cut_args,
                            int(seed) & 0xFFFFFFFF, ws.data_ptr(), ws_bytes, *[o.data_ptr() for o in outs], L.stream())
    L.check(rc, call)
    return tuple(outs)


def vocab_sample_takes(n, V, ld, top_k):
    """Does the launcher of vocab_sample take the shape?  (False: it would answer M3P_ENOTIMPL; a malformed one raises.)"""
    return _plan_takes('m3p_vocab_sample_plan', n, V, ld, top_k)


def vocab_sample(logits, V, temperature, seed, top_k=0):
    """Seeded sampling of a decoding step (csrc/select.hip; the contract is in include/m3p_hip.h, the NumPy twin in
    m3p_amd/rng.py): logits bf16 [n, ld >= V] (columns past V hold anything) -> (words int64 [n], logprob fp32 [n], key fp32 [n]):
    per row the argmax over the allowed set of  float(logit) * inv_t - log(-log(u)),  u from m3p_hash32(row * V + word, seed),
    inv_t = rng.inv_temperature(temperature); top_k = 0 allows every word, 1 .. 16 the row's top_k under (logit descending, word
    ascending); logprob = x_w * inv_t - log-sum-exp over the allowed set; key = the winning key.  None when the launcher does
    not take the shape (M3P_ENOTIMPL: top_k > 16, n * V >= 2^32)."""
    return _vocab_draw('m3p_vocab_sample', 'm3p_vocab_sample', logits, V, temperature, seed, top_k)


def vocab_nucleus_takes(n, V, ld, top_k):
    """Does the launcher of vocab_nucleus_sample take the shape?  (False: it would answer M3P_ENOTIMPL; a malformed one raises.)"""
    return _plan_takes('m3p_vocab_nucleus_plan', n, V, ld, top_k)


def vocab_nucleus_sample(logits, V, temperature, seed, top_p, top_k=0):
    """Seeded nucleus (top-p) sampling of a decoding step (csrc/select.hip; the contract is in include/m3p_hip.h, the NumPy
    twin in m3p_amd/rng.py: nucleus_cut, sample_words(top_p=...)): vocab_sample with its allowed set cut to the words whose
    logit is >= the row's cut x* = the largest logit value whose cumulated mass under softmax(float(logit) * inv_t) over the
    candidates (every word, or the row's top_k) reaches top_p - whole classes of equal logits.
    -> (words int64 [n], logprob fp32 [n], key fp32 [n], cut fp32 [n]); logprob is taken over the cut set, cut is x*.
    top_p None or >= 1.0 is "off": vocab_sample's own result, bit for bit, and cut = -inf; top_p <= 0 raises ValueError.
    None when the launcher does not take the shape (M3P_ENOTIMPL: top_k > 16, n * V >= 2^32)."""
    top_p = rng.nucleus_top_p(top_p)
    if top_p is None:
        top_p = 1.0                                # (the launcher's "off": it runs m3p_vocab_sample and fills cut with -inf)
    return _vocab_draw('m3p_vocab_nucleus', 'm3p_vocab_nucleus_sample', logits, V, temperature, seed, top_k, top_p)


def vocab_sample_wide_max_k():
    """VSW_MAX_K of csrc/select.hip: the most candidates per row m3p_vocab_sample_wide takes."""
    return int(L.load().m3p_vocab_sample_wide_max_k())


def vocab_sample_wide_takes(n, V, ld, top_k):
    """Does the launcher of vocab_sample_wide take the shape?  (False: it would answer M3P_ENOTIMPL; a malformed one raises.)"""
    return _plan_takes('m3p_vocab_sample_wide_plan', n, V, ld, top_k)


def vocab_sample_wide(logits, V, temperature, seed, top_k, top_p=None):
    """Seeded top-k sampling of a decoding step over 1 <= top_k <= vocab_sample_wide_max_k() (1024) candidates, with the
    nucleus cut when top_p is given (csrc/select.hip; the contract is in include/m3p_hip.h, the NumPy twin in m3p_amd/rng.py:
    sample_allowed, nucleus_cut, sample_words): the semantics of vocab_nucleus_sample - the row's first top_k words under
    (logit descending, word ascending), cut to the words whose logit is >= x*, the largest logit value whose cumulated mass
    over those candidates reaches top_p, and the Gumbel-max draw over what is left - by a count selection instead of top_k
    rounds of a maximum.  -> (words int64 [n], logprob fp32 [n], key fp32 [n], cut fp32 [n]).  top_p None or >= 1.0 is "off":
    no cut, cut = -inf; top_p <= 0 raises ValueError.  None when the launcher does not take the shape (M3P_ENOTIMPL: top_k >
    1024, n * V >= 2^32); top_k < 1 or > V raises."""
    top_p = rng.nucleus_top_p(top_p)
    if top_p is None:
        top_p = 1.0                                # (the launcher's "off")
    return _vocab_draw('m3p_vocab_sample_wide', 'm3p_vocab_sample_wide', logits, V, temperature, seed, top_k, top_p)


def logits_constrain_takes(n, V, ld, hist_len, ngram=0, n_banned=0):
    """Does the launcher of logits_constrain take the shape?  (False: it would answer M3P_ENOTIMPL - hist_len > 1024, ngram > 16,
    n_banned > 4096; a malformed one raises.)  The answer depends on shapes alone: a search loop asks once, with max_len - 1 as
    the history bound."""
    return _plan_takes('m3p_logits_constrain_plan', n, V, ld, hist_len, ngram, n_banned)


def logits_constrain(logits, V, generated, cur_len, theta=1.0, inv_theta=1.0, ngram=0, eos=-1, banned=None):
    """Decoding constraints of the step that decodes position cur_len (csrc/constrain.hip; the contract is in include/m3p_hip.h,
    the torch twin is decoder.constrain_scores_): edits logits bf16 [n, ld >= V] IN PLACE and returns them.  generated int64
    [>= cur_len, n] on the device, row-major: row r of the logits has the history generated[1:cur_len, r] (position 0, the
    <EOS> that serves as <BOS>, is not part of it; no copy and no transpose is made).  In this order: the repetition penalty
    (theta, inv_theta) = decoder.penalty_pair(...) on every distinct history word ((1.0, 1.0): off), -inf for the word that would
    complete a repeated n-gram (ngram = 0: off), -inf for the word `eos` (-1: off; the loop passes <EOS> while cur_len <=
    min_len), -inf for every id of `banned` (int64 device tensor or None).  None when the launcher does not take the shape
    (M3P_ENOTIMPL: cur_len - 1 > 1024, ngram > 16, more than 4096 banned ids); the logits are then untouched."""
    _chk_bf16(logits)
    assert logits.dim() == 2 and logits.stride(1) == 1 and logits.shape[1] >= V
    n = logits.shape[0]
    assert generated.dtype == torch.int64 and generated.is_cuda and generated.dim() == 2 and generated.stride(1) == 1
    assert 1 <= cur_len <= generated.shape[0] and generated.shape[1] == n and generated.stride(0) >= n
    n_banned = 0
    if banned is not None:
        assert banned.dtype == torch.int64 and banned.is_cuda and banned.dim() == 1 and banned.is_contiguous()
        n_banned = banned.numel()
    hist_len = cur_len - 1
    lib = L.load()
    rc = lib.m3p_logits_constrain_plan(n, V, logits.stride(0), hist_len, ngram, n_banned)
    if rc == _ENOTIMPL:
        return None
    L.check(rc, 'm3p_logits_constrain_plan')
    hist = generated.data_ptr() + generated.stride(0) * generated.element_size() if hist_len > 0 else None
    rc = lib.m3p_logits_constrain(logits.data_ptr(), logits.stride(0), n, V, hist, generated.stride(0), hist_len, float(theta),
                                  float(inv_theta), int(ngram), int(eos), L.ptr(banned) if n_banned else None, n_banned, L.stream())
    L.check(rc, 'm3p_logits_constrain')
    return logits


_BEAM_STATE = (('hyp_tok', torch.int64), ('hyp_len', torch.int32), ('hyp_score', torch.float64), ('hyp_sum', torch.float32),
               ('hyp_arrival', torch.int32), ('hyp_count', torch.int32), ('arrivals', torch.int32), ('done', torch.uint8),
               ('status', torch.int32))


def beam_state(bs, beam, max_len, pad, device):
    """The empty hypothesis state of beam_advance on `device`: decoder.beam_state_host as tensors (the same names, shapes and
    dtypes; hyp_tok filled with pad, everything else zero)."""
    shapes = dict(hyp_tok=(bs, beam, max_len), hyp_count=(bs,), arrivals=(bs,), done=(bs,), status=(bs,))
    state = {name: torch.zeros(shapes.get(name, (bs, beam)), dtype=dt, device=device) for name, dt in _BEAM_STATE}
    state['hyp_tok'].fill_(pad)
    return state


def beam_advance_takes(bs, beam, k, max_len):
    """Does the launcher of beam_advance take the shape?  (False: it would answer M3P_ENOTIMPL - beam > 32, k > 64, max_len >
    1025; a malformed one raises.)  The answer depends on shapes alone: generate_beam asks once."""
    return _plan_takes('m3p_beam_advance_plan', bs, beam, k, max_len)


def beam_advance(next_scores, flat_idx, gen_in, gen_out, owner_in, owner_out, state, cur_len, max_len, eos, pad, V, beam,
                 early_stopping, norm, norm_max):
    """The hypothesis bookkeeping of the beam-search step that decodes position cur_len, on the device (csrc/beam.hip; the
    contract is in include/m3p_hip.h, the host twin is decoder.beam_advance_host - equal bit for bit).  next_scores fp32 [bs, k],
    flat_idx int64 [bs, k]: the step's candidates as vocab_select returns them.  gen_in / gen_out int64 [max_len, n], owner_in /
    owner_out int32 [n, >= max_len] (n = bs * beam): read one, write the other - never the same tensor.  state: beam_state(...),
    updated IN PLACE.  norm fp64 [max_len + 1] on the device and norm_max: decoder.beam_norms.
    -> (beam_scores fp32 [n], beam_words int64 [n], beam_idx int64 [n]); gen_out holds the re-ordered tokens with the new words
    at position cur_len, owner_out the owner table decoder.advance_owner would return.  None when the launcher does not take the
    shape (M3P_ENOTIMPL); nothing is written then."""
    bs, k = next_scores.shape
    n = bs * beam
    dev = next_scores.device
    assert next_scores.dtype == torch.float32 and next_scores.is_cuda and next_scores.is_contiguous()
    assert flat_idx.dtype == torch.int64 and flat_idx.shape == (bs, k) and flat_idx.is_contiguous() and flat_idx.device == dev
    for g in (gen_in, gen_out):
        assert g.dtype == torch.int64 and g.device == dev and g.dim() == 2 and g.shape[0] >= max_len and g.shape[1] == n
        assert g.stride(1) == 1 and g.stride(0) == gen_in.stride(0)
    for o in (owner_in, owner_out):
        assert o.dtype == torch.int32 and o.device == dev and o.dim() == 2 and o.shape[0] == n and o.shape[1] >= max_len
        assert o.stride(1) == 1 and o.stride(0) == owner_in.stride(0)
    assert gen_in.data_ptr() != gen_out.data_ptr() and owner_in.data_ptr() != owner_out.data_ptr()
    assert norm.dtype == torch.float64 and norm.device == dev and norm.is_contiguous() and norm.numel() >= max_len + 1
    shapes = dict(hyp_tok=(bs, beam, max_len), hyp_count=(bs,), arrivals=(bs,), done=(bs,), status=(bs,))
    for name, dt in _BEAM_STATE:
        t = state[name]
        assert t.dtype == dt and t.device == dev and t.is_contiguous() and tuple(t.shape) == shapes.get(name, (bs, beam)), name
    lib = L.load()
    rc = lib.m3p_beam_advance_plan(bs, beam, k, max_len)
    if rc == _ENOTIMPL:
        return None
    L.check(rc, 'm3p_beam_advance_plan')
    beam_scores = torch.empty((n,), dtype=torch.float32, device=dev)
    beam_words = torch.empty((n,), dtype=torch.int64, device=dev)
    beam_idx = torch.empty((n,), dtype=torch.int64, device=dev)
    rc = lib.m3p_beam_advance(next_scores.data_ptr(), flat_idx.data_ptr(), bs, beam, k, int(V), int(cur_len), int(max_len), int(eos),
                              int(pad), 1 if early_stopping else 0, norm.data_ptr(), float(norm_max), gen_in.data_ptr(),
                              gen_out.data_ptr(), gen_in.stride(0), owner_in.data_ptr(), owner_out.data_ptr(), owner_in.stride(0),
                              beam_scores.data_ptr(), beam_words.data_ptr(), beam_idx.data_ptr(),
                              *[state[name].data_ptr() for name, _ in _BEAM_STATE], L.stream())
    L.check(rc, 'm3p_beam_advance')
    return beam_scores, beam_words, beam_idx


def attn_rows_fwd(q, kv, klen, B, Tq, H, dh, Lk, causal=False, seed=0, p_drop=0.0):
    """Training form of attn_query_fwd: dropout on the probabilities, returns (ctx bf16 [B*Tq, H*dh], lse fp32 [B, H, Tq])."""
    _chk_bf16(q, kv)
    assert q.stride(1) == 1 and kv.dim() == 3 and kv.stride(2) == 1 and kv.shape[0] == B and kv.shape[1] >= Lk
    ctx = torch.empty((B * Tq, H * dh), dtype=BF16, device=q.device)
    lse = torch.empty((B, H, Tq), dtype=torch.float32, device=q.device)
    rc = L.load().m3p_attn_rows_fwd(q.data_ptr(), q.stride(0), kv.data_ptr(), kv.stride(0), kv.stride(1), L.ptr(klen),
                                    ctx.data_ptr(), lse.data_ptr(), B, Tq, H, dh, Lk, 1 if causal else 0, 0, seed,
                                    L.thresh24(p_drop), 1.0 / (1.0 - p_drop) if p_drop > 0 else 1.0, L.stream())
    L.check(rc, 'm3p_attn_rows_fwd')
    return ctx, lse


def attn_rows_bwd(q, kv, klen, dctx, lse, B, Tq, H, dh, Lk, qscale, causal=False, seed=0, p_drop=0.0, dq_out=None):
    """-> (dq bf16 [B*Tq, H*dh] (or written into dq_out, row pitch dq_out.stride(0)), dkv fp32 [B, Lk, 2*H*dh])."""
    _chk_bf16(q, kv, dctx)
    assert dctx.is_contiguous()
    d = H * dh
    dq = dq_out if dq_out is not None else torch.empty((B * Tq, d), dtype=BF16, device=q.device)
    dkv = torch.zeros((B, Lk, 2 * d), dtype=torch.float32, device=q.device)
    rc = L.load().m3p_attn_rows_bwd(q.data_ptr(), q.stride(0), kv.data_ptr(), kv.stride(0), kv.stride(1), L.ptr(klen),
                                    dctx.data_ptr(), lse.data_ptr(), dq.data_ptr(), dq.stride(0), dkv.data_ptr(), B, Tq, H, dh, Lk,
                                    1 if causal else 0, 0, qscale, seed, L.thresh24(p_drop),
                                    1.0 / (1.0 - p_drop) if p_drop > 0 else 1.0, L.stream())
    L.check(rc, 'm3p_attn_rows_bwd')
    return dq, dkv


def _attn_tiled_fwd_out(out, B, T, H, dh, device):
    """(ctx bf16 [B*T, H*dh], lse fp32 [B, H, T]) of a tiled forward: ``out`` checked, or fresh."""
    if out is None:
        return (torch.empty((B * T, H * dh), dtype=BF16, device=device), torch.empty((B, H, T), dtype=torch.float32, device=device))
    ctx, lse = out
    assert ctx.dtype == BF16 and ctx.is_contiguous() and ctx.shape == (B * T, H * dh)
    assert lse.dtype == torch.float32 and lse.is_contiguous() and lse.shape == (B, H, T)
    return ctx, lse


def attn_causal_fwd(qkv, B, T, H, dh, seed=0, p_drop=0.0, out=None):
    """Causal self-attention of a decoder-only training pass on the tiled MFMA kernels (csrc/attn_tiled.hip): qkv bf16
    [B*T, >= 3*H*dh] (q scaled | k | v) -> (ctx bf16 [B*T, H*dh], lse fp32 [B, H, T]), the results of
    attn_rows_fwd(causal=True, klen=None, Lk=T) under the same seed.  Returns None when the kernels do not take the shape
    (M3P_ENOTIMPL: dh not in {32, 64}, T > 512, ...) - the caller then runs the rows kernels.  out = (ctx, lse) to write into."""
    _chk_bf16(qkv)
    assert qkv.dim() == 2 and qkv.stride(1) == 1 and qkv.shape[0] == B * T and qkv.shape[1] >= 3 * H * dh
    ctx, lse = _attn_tiled_fwd_out(out, B, T, H, dh, qkv.device)
    th, ik = _drop_args(p_drop)
    rc = L.load().m3p_attn_causal_fwd(qkv.data_ptr(), qkv.stride(0), ctx.data_ptr(), lse.data_ptr(), B, T, H, dh, seed, th, ik,
                                      L.stream())
    if rc == -2:            # (M3P_ENOTIMPL)
        return None
    L.check(rc, 'm3p_attn_causal_fwd')
    return ctx, lse


def attn_causal_bwd(qkv, dctx, lse, B, T, H, dh, qscale, seed=0, p_drop=0.0, out=None):
    """-> dqkv bf16 [B*T, 3*H*dh] (dq of the unscaled projection | dk | dv; every element written, no atomics), or written
    into ``out`` (row pitch out.stride(0)); None when the kernels do not take the shape."""
    _chk_bf16(qkv, dctx)
    assert qkv.dim() == 2 and qkv.stride(1) == 1 and qkv.shape[0] == B * T and dctx.is_contiguous()
    assert dctx.shape == (B * T, H * dh) and lse.dtype == torch.float32 and lse.is_contiguous() and lse.shape == (B, H, T)
    if out is not None:
        dqkv = out
        assert dqkv.dtype == BF16 and dqkv.stride(1) == 1 and dqkv.shape == (B * T, 3 * H * dh)
    else:
        dqkv = torch.empty((B * T, 3 * H * dh), dtype=BF16, device=qkv.device)
    th, ik = _drop_args(p_drop)
    rc = L.load().m3p_attn_causal_bwd(qkv.data_ptr(), qkv.stride(0), dctx.data_ptr(), lse.data_ptr(), dqkv.data_ptr(),
                                      dqkv.stride(0), B, T, H, dh, qscale, seed, th, ik, L.stream())
    if rc == -2:            # (M3P_ENOTIMPL)
        return None
    L.check(rc, 'm3p_attn_causal_bwd')
    return dqkv


def attn_cross_fwd(q, kv, klen, B, Tq, H, dh, Lk, seed=0, p_drop=0.0, out=None):
    """Attention over a source encoding in a teacher-forced decoder pass on the tiled MFMA kernels (csrc/attn_tiled.hip):
    operands as attn_rows_fwd(causal=False) -> (ctx bf16 [B*Tq, H*dh], lse fp32 [B, H, Tq]), its results under the same
    seed; key / value rows at or past klen[b] may hold anything.  Returns None when the kernels do not take the shape
    (M3P_ENOTIMPL: dh not in {32, 64}, Tq > 512, Lk > 1024, ...) - the caller then runs the rows kernels.
    out = (ctx, lse) to write into."""
    _chk_bf16(q, kv)
    assert q.dim() == 2 and q.stride(1) == 1 and q.shape[0] == B * Tq
    assert kv.dim() == 3 and kv.stride(2) == 1 and kv.shape[0] == B and kv.shape[1] >= Lk
    ctx, lse = _attn_tiled_fwd_out(out, B, Tq, H, dh, q.device)
    th, ik = _drop_args(p_drop)
    rc = L.load().m3p_attn_cross_fwd(q.data_ptr(), q.stride(0), kv.data_ptr(), kv.stride(0), kv.stride(1), L.ptr(klen),
                                     ctx.data_ptr(), lse.data_ptr(), B, Tq, H, dh, Lk, seed, th, ik, L.stream())
    if rc == -2:            # (M3P_ENOTIMPL)
        return None
    L.check(rc, 'm3p_attn_cross_fwd')
    return ctx, lse


def attn_prefix_fwd(q, kv, B, Tq, H, dh, pos0, out=None):
    """The prefill of a prompted decoding call on the tiled MFMA kernels (csrc/attn_tiled.hip): q bf16 [B*Tq, >= H*dh]
    (scaled), kv bf16 [B, >= pos0 + Tq, >= 2*H*dh] (the cache, the Tq new rows already stored at pos0 ..) ->
    (ctx bf16 [B*Tq, H*dh], lse fp32 [B, H, Tq]), the results of attn_query_fwd(causal=True, klen=None, Lk=pos0 + Tq,
    pos0=pos0); cache rows at or past pos0 + Tq may hold anything.  Returns None when the kernel does not take the shape
    (M3P_ENOTIMPL: dh not in {32, 64}, Tq > 512, pos0 + Tq > 1024, ...) - the caller then runs the rows kernel.
    out = (ctx, lse) to write into."""
    _chk_bf16(q, kv)
    assert q.dim() == 2 and q.stride(1) == 1 and q.shape[0] == B * Tq and pos0 >= 0
    assert kv.dim() == 3 and kv.stride(2) == 1 and kv.shape[0] == B and kv.shape[1] >= pos0 + Tq
    ctx, lse = _attn_tiled_fwd_out(out, B, Tq, H, dh, q.device)
    rc = L.load().m3p_attn_prefix_fwd(q.data_ptr(), q.stride(0), kv.data_ptr(), kv.stride(0), kv.stride(1), ctx.data_ptr(),
                                      lse.data_ptr(), B, Tq, H, dh, pos0, L.stream())
    if rc == -2:            # (M3P_ENOTIMPL)
        return None
    L.check(rc, 'm3p_attn_prefix_fwd')
    return ctx, lse


def attn_cross_bwd(q, kv, klen, dctx, lse, B, Tq, H, dh, Lk, qscale, seed=0, p_drop=0.0, out=None):
    """-> (dq bf16 [B*Tq, H*dh] of the unscaled projection, dkv BF16 [B, Lk, 2*H*dh]: every row written once, exact zeros
    for keys >= klen[b], no atomics - nothing to zero or cast), or written into out = (dq, dkv) (row pitches
    dq.stride(0), dkv.stride(1)); None when the kernels do not take the shape."""
    _chk_bf16(q, kv, dctx)
    d = H * dh
    assert q.dim() == 2 and q.stride(1) == 1 and q.shape[0] == B * Tq and dctx.is_contiguous() and dctx.shape == (B * Tq, d)
    assert kv.dim() == 3 and kv.stride(2) == 1 and kv.shape[0] == B and kv.shape[1] >= Lk
    assert lse.dtype == torch.float32 and lse.is_contiguous() and lse.shape == (B, H, Tq)
    if out is not None:
        dq, dkv = out
        assert dq.dtype == BF16 and dq.stride(1) == 1 and dq.shape == (B * Tq, d)
        assert dkv.dtype == BF16 and dkv.shape == (B, Lk, 2 * d) and dkv.stride(2) == 1 and dkv.stride(0) == Lk * dkv.stride(1)
    else:
        dq = torch.empty((B * Tq, d), dtype=BF16, device=q.device)
        dkv = torch.empty((B, Lk, 2 * d), dtype=BF16, device=q.device)
    th, ik = _drop_args(p_drop)
    rc = L.load().m3p_attn_cross_bwd(q.data_ptr(), q.stride(0), kv.data_ptr(), kv.stride(0), kv.stride(1), L.ptr(klen),
                                     dctx.data_ptr(), lse.data_ptr(), dq.data_ptr(), dq.stride(0), dkv.data_ptr(),
                                     dkv.stride(1), B, Tq, H, dh, Lk, qscale, seed, th, ik, L.stream())
    if rc == -2:            # (M3P_ENOTIMPL)
        return None
    L.check(rc, 'm3p_attn_cross_bwd')
    return dq, dkv


def cast_bf16(x):
    """fp32 -> bf16 through the HIP cast kernel (bf16 input is returned unchanged)."""
    if x.dtype == BF16:
        return x
    assert x.dtype == torch.float32 and x.is_contiguous() and x.numel() % 4 == 0
    out = torch.empty(x.shape, dtype=BF16, device=x.device)
    L.check(L.load().m3p_cast_f32_bf16(x.data_ptr(), out.data_ptr(), x.numel(), L.stream()), 'm3p_cast_f32_bf16')
    return out


_TILE_QUEUE = {}      # device index -> the counter ring handed to m3p_set_tile_queue (kept alive here)


def set_tile_queue(enable=True, slots=4096):
    """Dynamic tile queues for the persistent NT GEMM (include/m3p_hip.h: m3p_set_tile_queue): workgroups pop output tiles
    from per-XCD queues, so CUs slowed down by a co-resident collective kernel take fewer tiles.  Process-wide; all GEMMs on
    one stream."""
    dev = torch.cuda.current_device()
    if not enable:
        L.check(L.load().m3p_set_tile_queue(None, 0), 'm3p_set_tile_queue')
        _TILE_QUEUE.pop(dev, None)
        return
    pool = torch.zeros(slots * 8, dtype=torch.int32, device='cuda')
    torch.cuda.current_stream().synchronize()
    L.check(L.load().m3p_set_tile_queue(pool.data_ptr(), slots), 'm3p_set_tile_queue')
    _TILE_QUEUE[dev] = pool


def cast_f32_bf16_into(src, dst):
    """dst (bf16) <- src (fp32), same element count, on the current stream."""
    assert src.dtype == torch.float32 and dst.dtype == BF16 and src.is_contiguous() and dst.is_contiguous()
    assert src.numel() == dst.numel() and src.numel() % 4 == 0
    L.check(L.load().m3p_cast_f32_bf16(src.data_ptr(), dst.data_ptr(), src.numel(), L.stream()), 'm3p_cast_f32_bf16')


def cast_rows_bf16(x):
    """fp32 (n0, n1, cols) with ANY leading strides (unit stride along cols) -> contiguous bf16 [n0 * n1, cols]: the cast
    reads through a transposed view (the collate's (n, R, 2048) features seen as (R, n, 2048)) instead of copying it first."""
    assert x.dim() == 3 and x.dtype == torch.float32 and x.stride(2) == 1
    n0, n1, cols = x.shape
    out = torch.empty((n0 * n1, cols), dtype=BF16, device=x.device)
    L.check(L.load().m3p_cast_rows_f32_bf16(x.data_ptr(), x.stride(0), x.stride(1), n0, n1, cols, out.data_ptr(), L.stream()),
            'm3p_cast_rows_f32_bf16')
    return out


def seq_masks(lengths, lengths_b, B, S):
    """-> (totlen int32 [B], rowmask uint8 [B * S]): totlen = lengths (+ lengths_b), rowmask[b, s] = s < totlen[b]."""
    dev = lengths.device
    assert lengths.dtype == torch.int64 and lengths.is_contiguous() and lengths.numel() == B
    if lengths_b is not None:
        assert lengths_b.dtype == torch.int64 and lengths_b.is_contiguous() and lengths_b.numel() == B and lengths_b.device == dev
    totlen = torch.empty((B,), dtype=torch.int32, device=dev)
    rowmask = torch.empty((B * S,), dtype=torch.uint8, device=dev)
    L.check(L.load().m3p_seq_masks(lengths.data_ptr(), L.ptr(lengths_b), B, S, totlen.data_ptr(), rowmask.data_ptr(), L.stream()),
            'm3p_seq_masks')
    return totlen, rowmask


def mask_to_rows(mask, inner, s0, s1, soff, d, n_rows):
    """Row numbers (int32 [n_rows]) of the True entries of ``mask`` (bool / uint8, flat order t * inner + b) inside the
    [*, d] row buffer under a strided (T, inner, d) view: (soff + t * s0 + b * s1) // d."""
    m = mask.reshape(-1)
    if m.dtype == torch.bool:
        m = m.view(torch.uint8)
    assert m.dtype == torch.uint8 and m.is_contiguous()
    rows = torch.empty((n_rows,), dtype=torch.int32, device=m.device)
    if _DEBUG_CHECKS:      # (M3P_DEBUG_CHECKS=1: a host sync per call - fewer True entries than n_rows would point the tail at row 0)
        assert int(m.sum().item()) == n_rows, 'mask holds %d True entries, the caller counted %d' % (int(m.sum().item()), n_rows)
    L.check(L.load().m3p_mask_to_rows(m.data_ptr(), m.numel(), inner, s0, s1, soff, d, rows.data_ptr(), n_rows, L.stream()),
            'm3p_mask_to_rows')
    return rows


def scale_bf16_dev(x, g):
    """bf16(g[0] * x) for a bf16 or fp32 ``x`` and a device scalar ``g`` (fp32 [1])."""
    assert x.is_contiguous() and x.dtype in (BF16, torch.float32) and g.dtype == torch.float32 and g.numel() == 1
    out = torch.empty(x.shape, dtype=BF16, device=x.device)
    L.check(L.load().m3p_scale_bf16_dev(x.data_ptr(), int(x.dtype == torch.float32), g.data_ptr(), out.data_ptr(), x.numel(),
                                        L.stream()), 'm3p_scale_bf16_dev')
    return out


def axpy_dev(dst, src, g):
    """dst += g[0] * src (fp32, contiguous), g a device scalar."""
    assert dst.dtype == src.dtype == g.dtype == torch.float32 and dst.is_contiguous() and src.is_contiguous()
    assert dst.numel() == src.numel()
    L.check(L.load().m3p_axpy_dev_f32(dst.data_ptr(), src.data_ptr(), g.data_ptr(), dst.numel(), L.stream()), 'm3p_axpy_dev_f32')


def itm_loss_fwd_bwd(scores, pos, sample_n, w_ce, w_bce):
    """-> (loss fp32 [1], dscores fp32 like scores): xtrainer.py:2357-2372 (CE over groups of sample_n + BCE vs one-hot)."""
    sc = scores.reshape(-1)
    assert sc.dtype == torch.float32 and sc.is_contiguous() and pos.dtype == torch.int64 and pos.is_contiguous()
    G = pos.numel()
    assert sc.numel() == G * sample_n, (sc.numel(), G, sample_n)
    loss = torch.empty((1,), dtype=torch.float32, device=sc.device)
    dsc = torch.empty_like(sc)
    L.check(L.load().m3p_itm_loss_fwd_bwd(sc.data_ptr(), pos.data_ptr(), G, sample_n, float(w_ce), float(w_bce), loss.data_ptr(),
                                          dsc.data_ptr(), L.stream()), 'm3p_itm_loss_fwd_bwd')
    return loss, dsc


def _drop_args(p):
    return L.thresh24(p), (1.0 / (1.0 - p) if p > 0 else 1.0)


def embed_assemble_fwd(tok, emb16, pos, img_proj, loc, w_loc, b_loc, g_img, be_img, g_emb, be_emb, totlen,
                       B, T, R, d, seed_img=0, seed_emb=0, p_drop=0.0, img_rows=None, img_saved=None):
    """img_rows (bf16 [B*R, d], rows b*R + r) replaces the computed image rows (AoA refiner output); img_saved is
    then the (e, mean_i, rstd_i) triple embed_image_rows_fwd returned for backward."""
    dev = emb16.device
    S = R + T
    h = torch.empty((B * S, d), dtype=BF16, device=dev)
    z = torch.empty((B * S, d), dtype=BF16, device=dev)
    mean_e = torch.empty(B * S, dtype=torch.float32, device=dev)
    rstd_e = torch.empty(B * S, dtype=torch.float32, device=dev)
    if img_rows is not None:
        assert img_rows.dtype == BF16 and img_rows.is_contiguous() and img_rows.shape == (B * R, d)
        e, mean_i, rstd_i = img_saved
    else:
        e = torch.empty((max(R * B, 1), d), dtype=BF16, device=dev)
        mean_i = torch.empty(max(R * B, 1), dtype=torch.float32, device=dev)
        rstd_i = torch.empty(max(R * B, 1), dtype=torch.float32, device=dev)
    th, ik = _drop_args(p_drop)
    rc = L.load().m3p_embed_assemble_fwd(
        tok.data_ptr(), emb16.data_ptr(), pos.data_ptr(), L.ptr(img_proj), L.ptr(loc), w_loc.data_ptr(),
        b_loc.data_ptr(), g_img.data_ptr(), be_img.data_ptr(), g_emb.data_ptr(), be_emb.data_ptr(), totlen.data_ptr(),
        h.data_ptr(), z.data_ptr(), mean_e.data_ptr(), rstd_e.data_ptr(), e.data_ptr(), mean_i.data_ptr(),
        rstd_i.data_ptr(), B, T, R, d, seed_img, seed_emb, th, ik, L.ptr(img_rows), L.stream())
    L.check(rc, 'm3p_embed_assemble_fwd')
    return h, (z, mean_e, rstd_e, e, mean_i, rstd_i)


def embed_image_rows_fwd(img_proj, loc, w_loc, b_loc, g_img, be_img, B, R, d, seed_img=0, p_drop=0.0):
    """Image rows after LayerNorm + dropout as their own tensor (bf16 [B*R, d], rows b*R + r) and the saved
    (e, mean_i, rstd_i) for backward."""
    dev = img_proj.device
    e = torch.empty((R * B, d), dtype=BF16, device=dev)
    mean_i = torch.empty(R * B, dtype=torch.float32, device=dev)
    rstd_i = torch.empty(R * B, dtype=torch.float32, device=dev)
    rows = torch.empty((B * R, d), dtype=BF16, device=dev)
    th, ik = _drop_args(p_drop)
    rc = L.load().m3p_embed_image_rows_fwd(img_proj.data_ptr(), loc.data_ptr(), w_loc.data_ptr(), b_loc.data_ptr(),
                                           g_img.data_ptr(), be_img.data_ptr(), e.data_ptr(), mean_i.data_ptr(),
                                           rstd_i.data_ptr(), rows.data_ptr(), B, R, d, seed_img, th, ik, L.stream())
    L.check(rc, 'm3p_embed_image_rows_fwd')
    return rows, (e, mean_i, rstd_i)


def embed_image_rows_bwd(d_rows, img_saved, g_img, loc, totlen, grads, B, R, d, seed_img=0, p_drop=0.0):
    """Backward of embed_image_rows_fwd alone (the image-only stream): d_rows bf16 [B*R, d] = gradient wrt the rows it
    returned -> its dropout, LayerNorm and location-projection backward (the image half of m3p_embed_assemble_bwd with no
    token rows).  grads: d_g_img, d_be_img, d_b_img, d_b_loc, d_w_loc.  Returns de (bf16 [R*B, d], rows r*B + b): the
    gradient wrt the image projection's output."""
    e, mean_i, rstd_i = img_saved
    assert d_rows.dtype == BF16 and d_rows.is_contiguous() and d_rows.shape == (B * R, d)
    de = torch.empty_like(e)
    th, ik = _drop_args(p_drop)
    dummy = d_rows.data_ptr()       # the token-row arguments are not read by the image half
    args = (dummy, dummy, mean_i.data_ptr(), rstd_i.data_ptr(), g_img.data_ptr(), e.data_ptr(), mean_i.data_ptr(),
            rstd_i.data_ptr(), g_img.data_ptr(), dummy, totlen.data_ptr(), loc.data_ptr(), d_rows.data_ptr(), de.data_ptr(),
            grads['d_g_img'].data_ptr(), grads['d_be_img'].data_ptr(), grads['d_g_img'].data_ptr(), grads['d_g_img'].data_ptr(),
            None, grads['d_g_img'].data_ptr(), grads['d_be_img'].data_ptr(), grads['d_b_img'].data_ptr(),
            grads['d_b_loc'].data_ptr(), grads['d_w_loc'].data_ptr(), B, 0, R, d, -1, seed_img, 0, th, ik)
    L.check(L.load().m3p_embed_assemble_bwd(*args, 2, L.stream()), 'm3p_embed_assemble_bwd')
    return de


def embed_assemble_bwd(dh, saved, g_emb, g_img, tok, totlen, loc, grads, B, T, R, d, pad_index,
                       seed_img=0, seed_emb=0, p_drop=0.0, img_rows_bwd=None, tok_rows=None):
    """grads: dict of fp32 gradient views (d_g_emb, d_be_emb, d_pos, d_emb, d_g_img, d_be_img, d_b_img,
    d_b_loc, d_w_loc).  Returns de (bf16 [R*B, d]).
    img_rows_bwd (refine_image): callable taking the gradient of the refined image rows (bf16 [B*R, d]) and
    returning the gradient of the refiner's input; run between the two halves of the backward.
    tok_rows (data parallelism): bf16 [T*B, d] buffer that receives the token rows' gradients instead of the
    scatter-add into d_emb."""
    z, mean_e, rstd_e, e, mean_i, rstd_i = saved
    dz = torch.empty_like(z)
    de = torch.empty_like(e)
    th, ik = _drop_args(p_drop)
    if tok_rows is not None:
        assert tok_rows.dtype == BF16 and tok_rows.is_contiguous() and tok_rows.shape == (T * B, d)
    args = (dh.data_ptr(), z.data_ptr(), mean_e.data_ptr(), rstd_e.data_ptr(), g_emb.data_ptr(), e.data_ptr(),
            mean_i.data_ptr(), rstd_i.data_ptr(), g_img.data_ptr(), tok.data_ptr(), totlen.data_ptr(), L.ptr(loc),
            dz.data_ptr(), de.data_ptr(), grads['d_g_emb'].data_ptr(), grads['d_be_emb'].data_ptr(),
            grads['d_pos'].data_ptr(), grads['d_emb'].data_ptr(), L.ptr(tok_rows), grads['d_g_img'].data_ptr(),
            grads['d_be_img'].data_ptr(), grads['d_b_img'].data_ptr(), grads['d_b_loc'].data_ptr(),
            grads['d_w_loc'].data_ptr(), B, T, R, d, pad_index, seed_img, seed_emb, th, ik)
    if img_rows_bwd is not None:
        L.check(L.load().m3p_embed_assemble_bwd(*args, 1, L.stream()), 'm3p_embed_assemble_bwd')
        dz_img = dz.view(B, R + T, d)[:, :R, :]
        dz_img.copy_(img_rows_bwd(dz_img.contiguous().view(B * R, d)).view(B, R, d))
        L.check(L.load().m3p_embed_assemble_bwd(*args, 2, L.stream()), 'm3p_embed_assemble_bwd')
        return de
    L.check(L.load().m3p_embed_assemble_bwd(*args, 0, L.stream()), 'm3p_embed_assemble_bwd')
    return de


def scatter_add_token_rows(rows, ids, dst, pad_index):
    """dst[ids[i], :] (fp32 [V, d]) += rows[i, :] (bf16 [n, d], any row pitch); pad rows skipped."""
    _chk_bf16(rows)
    assert ids.dtype == torch.int64 and dst.dtype == torch.float32 and rows.stride(1) == 1 and ids.is_contiguous()
    n, d = rows.shape
    assert ids.numel() == n and dst.shape[1] == d and dst.stride(0) == d
    L.check(L.load().m3p_scatter_add_token_rows(rows.data_ptr(), rows.stride(0), ids.data_ptr(), dst.data_ptr(), n, d, int(pad_index),
                                                L.stream()), 'm3p_scatter_add_token_rows')


def gather_rows(src_base, idx, n, d):
    out = torch.empty((n, d), dtype=BF16, device=idx.device)
    L.check(L.load().m3p_gather_rows(src_base.data_ptr(), idx.data_ptr(), out.data_ptr(), n, d, L.stream()), 'm3p_gather_rows')
    return out


BF16_NAN_BITS = 0x7FC0


def place_rows(src, inv, rows, fill_bits=0):
    """[rows, d] bf16 = src[inv[r]] where inv[r] >= 0 (src [n, d]), else the bit pattern fill_bits (0, or BF16_NAN_BITS):
    a fill and a row scatter written in one pass.  inv int32 [rows] = the inverse of the row list src was gathered by."""
    _chk_bf16(src)
    n, d = src.shape
    assert src.is_contiguous() and inv.dtype == torch.int32 and inv.is_cuda and inv.is_contiguous() and inv.numel() == rows
    out = torch.empty((rows, d), dtype=BF16, device=src.device)
    L.check(L.load().m3p_place_rows(src.data_ptr(), inv.data_ptr(), out.data_ptr(), rows, d, n, int(fill_bits), L.stream()),
            'm3p_place_rows')
    return out


def scatter_add_rows(src, idx, dst_base, n, d):
    L.check(L.load().m3p_scatter_add_rows(src.data_ptr(), idx.data_ptr(), dst_base.data_ptr(), n, d, L.stream()),
            'm3p_scatter_add_rows')


def ce_fwd_bwd(logits, V, target, loss_scale, grad_scale):
    """In place: logits <- dlogits.  Returns (loss_sum [1] fp32, row_loss [n] fp32)."""
    n, ld = logits.shape[0], logits.stride(0)
    row_loss = torch.empty(n, dtype=torch.float32, device=logits.device)
    assert target.dtype == torch.int64
    rc = L.load().m3p_ce_fwd_bwd(logits.data_ptr(), ld, n, V, target.data_ptr(), row_loss.data_ptr(),
                                 None, loss_scale, grad_scale, L.stream())
    L.check(rc, 'm3p_ce_fwd_bwd')
    loss_sum = (row_loss.sum() * loss_scale).reshape(1)   # tiny reduction; avoids n same-address atomics
    return loss_sum, row_loss


_CE_WS = {}


def ce_fwd_bwd_colsum(logits, V, target, loss_scale, grad_scale):
    """ce_fwd_bwd + the column sums of the gradient from the same pass.  In place: logits <- dlogits.
    Returns (loss_sum [1], row_loss [n], colsum fp32 [ld] of the rounded gradient)."""
    n, ld = logits.shape[0], logits.stride(0)
    dev = logits.device
    row_loss = torch.empty(n, dtype=torch.float32, device=dev)
    row_lse = torch.empty(n, dtype=torch.float32, device=dev)
    cs = torch.empty(ld, dtype=torch.float32, device=dev)
    need = L.load().m3p_ce_colsum_workspace_bytes(ld, n)
    ws = _CE_WS.get(dev)
    if ws is None or ws.numel() < need:
        ws = _CE_WS[dev] = torch.empty(need, dtype=torch.uint8, device=dev)
    assert target.dtype == torch.int64
    rc = L.load().m3p_ce_fwd_bwd_colsum(logits.data_ptr(), ld, n, V, target.data_ptr(), row_loss.data_ptr(), row_lse.data_ptr(),
                                        grad_scale, cs.data_ptr(), ws.data_ptr(), ws.numel(), L.stream())
    L.check(rc, 'm3p_ce_fwd_bwd_colsum')
    return (row_loss.sum() * loss_scale).reshape(1), row_loss, cs


def ce_from_block_stats(logits, V, target, stats, loss_scale, grad_scale):
    """ce_fwd_bwd_colsum with the first pass replaced by the 64-column block statistics the vocabulary projection wrote
    (gemm_nt(..., EPI_BIAS_LSE, out2=stats)): the rows' log-sum-exp is a reduction over N / 64 pairs, not over the logits."""
    n, ld = logits.shape[0], logits.stride(0)
    dev = logits.device
    row_loss = torch.empty(n, dtype=torch.float32, device=dev)
    row_lse = torch.empty(n, dtype=torch.float32, device=dev)
    cs = torch.empty(ld, dtype=torch.float32, device=dev)
    scratch = torch.empty((32, n, 2), dtype=torch.float32, device=dev)
    assert target.dtype == torch.int64 and stats.dtype == torch.float32 and stats.shape[1] == n
    L.check(L.load().m3p_ce_lse_from_blocks(stats.data_ptr(), stats.shape[0], n, logits.data_ptr(), ld, target.data_ptr(),
                                            row_loss.data_ptr(), row_lse.data_ptr(), scratch.data_ptr(), L.stream()),
            'm3p_ce_lse_from_blocks')
    need = L.load().m3p_ce_colsum_workspace_bytes(ld, n)
    ws = _CE_WS.get(dev)
    if ws is None or ws.numel() < need:
        ws = _CE_WS[dev] = torch.empty(need, dtype=torch.uint8, device=dev)
    L.check(L.load().m3p_ce_bwd_colsum(logits.data_ptr(), ld, n, V, target.data_ptr(), row_lse.data_ptr(), grad_scale, cs.data_ptr(),
                                       ws.data_ptr(), ws.numel(), L.stream()), 'm3p_ce_bwd_colsum')
    return (row_loss.sum() * loss_scale).reshape(1), row_loss, cs


def ce_shift_target(h, emb, bias, target):
    """The target's own logit of every row, t = h . emb[target] + bias[target] (fp32 accumulation over the bf16 operands), and the
    rows' {t + 40, target} pairs the shifted-exponential projection reads (``gemm_nt(..., EPI_BIAS_LSE, row_ref=...)``).
    Returns (row_t fp32 [n], row_ref int32 [n, 2]: the shift's fp32 bits and the target)."""
    _chk_bf16(h, emb)
    n, d = h.shape
    assert h.is_contiguous() and emb.stride(0) == d and emb.stride(1) == 1 and bias.dtype == torch.float32 and bias.is_contiguous()
    assert target.dtype == torch.int64 and target.is_contiguous() and target.numel() == n
    row_t = torch.empty(n, dtype=torch.float32, device=h.device)
    row_ref = torch.empty((n, 2), dtype=torch.int32, device=h.device)
    L.check(L.load().m3p_ce_shift_target(h.data_ptr(), emb.data_ptr(), bias.data_ptr(), target.data_ptr(), row_t.data_ptr(),
                                         row_ref.data_ptr(), n, d, L.stream()), 'm3p_ce_shift_target')
    return row_t, row_ref


def ce_shift_colsum(e, row_s):
    """colsum fp32 [ld] = sum_n row_s[n] e[n, :] in a pass of its own over e (bf16 [n, ld])."""
    n, ld = e.shape[0], e.stride(0)
    dev = e.device
    cs = torch.empty(ld, dtype=torch.float32, device=dev)
    need = L.load().m3p_ce_colsum_workspace_bytes(ld, n)
    ws = _CE_WS.get(dev)
    if ws is None or ws.numel() < need:
        ws = _CE_WS[dev] = torch.empty(need, dtype=torch.uint8, device=dev)
    L.check(L.load().m3p_ce_shift_colsum(e.data_ptr(), ld, n, row_s.data_ptr(), cs.data_ptr(), ws.data_ptr(), ws.numel(), L.stream()),
            'm3p_ce_shift_colsum')
    return cs


def ce_shift_from_block_sums(e, stats, loss_scale, grad_scale, colsum=True):
    """The cross-entropy from what the shifted-exponential projection left (e bf16 [n, ld], stats fp32 [N / 64, n] block sums):
    returns (loss_sum [1], row_loss [n], row_s [n] = grad_scale / Sigma, row_q [n] = grad_scale * (p_target - 1),
    colsum fp32 [ld] = sum_n row_s[n] e[n, :] - the output-bias gradient but for the targets' terms).  e is only read.
    colsum=False: no pass over e, None in its place (the caller gets the sums from gemm_wgrad_bias, or ce_shift_colsum later)."""
    n, ld = e.shape[0], e.stride(0)
    dev = e.device
    assert stats.dtype == torch.float32 and stats.is_contiguous() and stats.shape[1] == n
    row_loss = torch.empty(n, dtype=torch.float32, device=dev)
    row_s = torch.empty(n, dtype=torch.float32, device=dev)
    row_q = torch.empty(n, dtype=torch.float32, device=dev)
    scratch = torch.empty((32, n), dtype=torch.float32, device=dev)
    L.check(L.load().m3p_ce_shift_rows(stats.data_ptr(), stats.shape[0], n, grad_scale, row_loss.data_ptr(), row_s.data_ptr(),
                                       row_q.data_ptr(), scratch.data_ptr(), L.stream()), 'm3p_ce_shift_rows')
    cs = ce_shift_colsum(e, row_s) if colsum else None
    return (row_loss.sum() * loss_scale).reshape(1), row_loss, row_s, row_q, cs


def ce_shift_scale_rows(h, row_s, g):
    """bf16(g[0] * row_s[n] * h[n, :]): the weight-gradient product's second operand with the softmax normaliser on it."""
    _chk_bf16(h)
    assert h.is_contiguous() and row_s.dtype == g.dtype == torch.float32 and row_s.numel() == h.shape[0] and g.numel() == 1
    out = torch.empty_like(h)
    L.check(L.load().m3p_ce_shift_scale_rows(h.data_ptr(), row_s.data_ptr(), g.data_ptr(), out.data_ptr(), h.shape[0], h.shape[1],
                                             L.stream()), 'm3p_ce_shift_scale_rows')
    return out


def ce_shift_target_rows(h, target, row_q, g, demb, dbias):
    """demb[target[n], :] += g[0] * row_q[n] * h[n, :] and dbias[target[n]] += g[0] * row_q[n] (fp32 atomics; ids repeat)."""
    _chk_bf16(h)
    n, d = h.shape
    assert h.is_contiguous() and target.dtype == torch.int64 and target.numel() == n and row_q.dtype == g.dtype == torch.float32
    assert demb.dtype == dbias.dtype == torch.float32 and demb.shape[1] == d and demb.stride(0) == d and dbias.is_contiguous()
    L.check(L.load().m3p_ce_shift_target_rows(h.data_ptr(), target.data_ptr(), row_q.data_ptr(), g.data_ptr(), demb.data_ptr(),
                                              dbias.data_ptr(), n, d, L.stream()), 'm3p_ce_shift_target_rows')


def ce_shift_dh(dh32, emb, target, row_s, row_q, g):
    """bf16(g[0] * (row_s[n] * dh32[n, :] + row_q[n] * emb[target[n], :])) for dh32 = e x E (fp32 [n, d])."""
    _chk_bf16(emb)
    n, d = dh32.shape
    assert dh32.dtype == torch.float32 and dh32.is_contiguous() and emb.stride(0) == d and emb.stride(1) == 1
    assert target.dtype == torch.int64 and target.numel() == n and row_s.dtype == row_q.dtype == g.dtype == torch.float32
    out = torch.empty((n, d), dtype=BF16, device=dh32.device)
    L.check(L.load().m3p_ce_shift_dh(dh32.data_ptr(), emb.data_ptr(), target.data_ptr(), row_s.data_ptr(), row_q.data_ptr(),
                                     g.data_ptr(), out.data_ptr(), n, d, L.stream()), 'm3p_ce_shift_dh')
    return out


# ---- label smoothing of the tied vocabulary head (csrc/smooth.hip)
_LS_WS = {}


def _ls_workspace(dev, rows, d):
    need = L.load().m3p_vocab_mean_workspace_bytes(rows, d)
    ws = _LS_WS.get(dev)
    if ws is None or ws.numel() < need:
        ws = _LS_WS[dev] = torch.empty(need, dtype=torch.uint8, device=dev)
    return ws


def vocab_mean(emb, bias, V):
    """fp32 [d + 1]: the mean row of emb[:V] (bf16 [>= V, d], rows behind V not read) followed by the mean of bias[:V] (fp32).
    Ordered two-stage sums: bit-reproducible."""
    _chk_bf16(emb)
    d = emb.shape[1]
    assert emb.stride(0) == d and emb.stride(1) == 1 and emb.shape[0] >= V and bias.dtype == torch.float32 and bias.is_contiguous()
    assert bias.numel() >= V
    out = torch.empty(d + 1, dtype=torch.float32, device=emb.device)
    ws = _ls_workspace(emb.device, V, d)
    L.check(L.load().m3p_vocab_mean(emb.data_ptr(), bias.data_ptr(), V, d, out.data_ptr(), ws.data_ptr(), ws.numel(), L.stream()),
            'm3p_vocab_mean')
    return out


def ls_colsum_rows(h, scale):
    """fp32 [d] = scale * sum_r h[r, :] (h bf16 [n, d]), the ordered sums of vocab_mean."""
    _chk_bf16(h)
    n, d = h.shape
    assert h.is_contiguous()
    out = torch.empty(d, dtype=torch.float32, device=h.device)
    ws = _ls_workspace(h.device, n, d)
    L.check(L.load().m3p_ls_colsum_rows(h.data_ptr(), n, d, float(scale), out.data_ptr(), ws.data_ptr(), ws.numel(), L.stream()),
            'm3p_ls_colsum_rows')
    return out


def ls_row_aux(h, mean, row_t):
    """fp32 [n]: row_t[r] - h[r, :] . mean[:d] - mean[d], the rows' label-smoothing term (row_t: ce_shift_target)."""
    _chk_bf16(h)
    n, d = h.shape
    assert h.is_contiguous() and mean.dtype == row_t.dtype == torch.float32 and mean.numel() == d + 1 and row_t.numel() == n
    aux = torch.empty(n, dtype=torch.float32, device=h.device)
    L.check(L.load().m3p_ls_row_aux(h.data_ptr(), mean.data_ptr(), row_t.data_ptr(), aux.data_ptr(), n, d, L.stream()), 'm3p_ls_row_aux')
    return aux


def ls_sum_rows(v, scale):
    """fp32 [1] = scale * sum(v) (v fp32 [n]) added up in a fixed order by one block: the rows' aux terms into the loss."""
    assert v.dtype == torch.float32 and v.is_contiguous() and v.dim() == 1
    out = torch.empty(1, dtype=torch.float32, device=v.device)
    L.check(L.load().m3p_ls_sum_rows(v.data_ptr(), v.numel(), float(scale), out.data_ptr(), L.stream()), 'm3p_ls_sum_rows')
    return out


def ce_shift_dh_smooth(dh32, emb, target, row_s, row_q, g, mean, c):
    """bf16(g[0] * (row_s[n] * dh32[n, :] + (row_q[n] + c) * emb[target[n], :] - c * mean[:d])): ce_shift_dh with the label-
    smoothing operand, one rounding per element.  row_s = row_q = None: 1 and 0 (the plain routes' dh32 = dlogits x E)."""
    _chk_bf16(emb)
    n, d = dh32.shape
    assert dh32.dtype == torch.float32 and dh32.is_contiguous() and emb.stride(0) == d and emb.stride(1) == 1
    assert target.dtype == torch.int64 and target.numel() == n and g.dtype == mean.dtype == torch.float32 and mean.numel() == d + 1
    assert (row_s is None) == (row_q is None)
    if row_s is not None:
        assert row_s.dtype == row_q.dtype == torch.float32 and row_s.numel() == row_q.numel() == n
    out = torch.empty((n, d), dtype=BF16, device=dh32.device)
    L.check(L.load().m3p_ce_shift_dh_smooth(dh32.data_ptr(), emb.data_ptr(), target.data_ptr(), L.ptr(row_s), L.ptr(row_q), g.data_ptr(),
                                            mean.data_ptr(), float(c), out.data_ptr(), n, d, L.stream()), 'm3p_ce_shift_dh_smooth')
    return out


def ls_uniform_add(demb, dbias, u, g, db, V):
    """demb[v, :] += g[0] * u and dbias[v] += g[0] * db for v < V (fp32 [>= V, d] and [>= V]); rows from V on are not touched."""
    d = demb.shape[1]
    assert demb.dtype == dbias.dtype == u.dtype == g.dtype == torch.float32 and demb.stride(0) == d and demb.stride(1) == 1
    assert demb.shape[0] >= V and dbias.numel() >= V and dbias.is_contiguous() and u.numel() == d and g.numel() == 1
    L.check(L.load().m3p_ls_uniform_add(demb.data_ptr(), dbias.data_ptr(), u.data_ptr(), g.data_ptr(), float(db), V, d, L.stream()),
            'm3p_ls_uniform_add')


def ce_eval(logits, V, target):
    """Validation scoring, one read-only pass over bf16 logits [n, ld >= V] (columns [V, ld) ignored): returns
    (row_loss fp32 [n] = logsumexp - target logit, row_argmax int32 [n] = lowest column of the row's maximum)."""
    _chk_bf16(logits)
    assert logits.dim() == 2 and logits.stride(1) == 1 and target.dtype == torch.int64 and target.is_contiguous()
    n, ld = logits.shape[0], logits.stride(0)
    assert target.numel() == n and ld >= V
    row_loss = torch.empty(n, dtype=torch.float32, device=logits.device)
    row_argmax = torch.empty(n, dtype=torch.int32, device=logits.device)
    L.check(L.load().m3p_ce_eval(logits.data_ptr(), ld, n, V, target.data_ptr(), row_loss.data_ptr(), row_argmax.data_ptr(),
                                 L.stream()), 'm3p_ce_eval')
    return row_loss, row_argmax


def colsum(x, ncols, out, scale=None):
    rc = L.load().m3p_colsum_bf16(x.data_ptr(), x.stride(0), x.shape[0], ncols, out.data_ptr(), L.ptr(scale), L.stream())
    L.check(rc, 'm3p_colsum_bf16')


def sumsq(g, out):
    L.check(L.load().m3p_sumsq_f32(g.data_ptr(), g.numel(), out.data_ptr(), L.stream()), 'm3p_sumsq_f32')


def sumsq_ranges(buf, ranges, out):
    """out += sum of squares over the pieces buf[a:b] for (a, b) in ranges - one launch (m3p_sumsq_ranges_f32)."""
    ranges = [(int(a), int(b)) for a, b in ranges if b > a]
    if not ranges:
        return
    if len(ranges) == 1:
        return sumsq(buf[ranges[0][0]:ranges[0][1]], out)
    n = len(ranges)
    starts = (C.c_longlong * n)(*[a for a, _ in ranges])
    counts = (C.c_longlong * n)(*[b - a for a, b in ranges])
    L.check(L.load().m3p_sumsq_ranges_f32(buf.data_ptr(), starts, counts, n, out.data_ptr(), L.stream()), 'm3p_sumsq_ranges_f32')


def adam_step(p, g, m, v, w16, lr, beta1, beta2, eps, weight_decay, step_size, gnorm_sq=None, max_norm=0.0,
              grad_scale=1.0, zero_grad=True):
    n = p.numel()
    rc = L.load().m3p_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), L.ptr(w16), n, lr, beta1, beta2,
                                eps, weight_decay, step_size, L.ptr(gnorm_sq), max_norm, grad_scale, int(zero_grad),
                                L.stream())
    L.check(rc, 'm3p_adam_step')


class StepGuard:
    """Device state of the non-finite guard (include/m3p_hip.h, m3p_step_guard) in ONE buffer, so that a reconcile is one
    host read: counters {attempts, skipped_total, skipped_in_a_row} (int64), the ring of norms (float64 x 64), the ring of
    skip flags (int32 x 64) and the current step's `skip` word that the guarded update launches read."""
    RING = 64                 # M3P_GUARD_RING
    MAX_ARENAS = 8            # M3P_GUARD_MAX_ARENAS
    _COUNTERS, _NORMS, _RING, _SKIP, _BYTES = 0, 32, 32 + 8 * 64, 32 + 8 * 64 + 4 * 64, 32 + 8 * 64 + 4 * 64 + 16

    def __init__(self, device):
        self.buf = torch.zeros(self._BYTES, dtype=torch.uint8, device=device)
        self.counters = self.buf[self._COUNTERS:self._COUNTERS + 24].view(torch.int64)
        self.norm_ring = self.buf[self._NORMS:self._RING].view(torch.float64)
        self.ring = self.buf[self._RING:self._SKIP].view(torch.int32)
        self.skip = self.buf[self._SKIP:self._SKIP + 4].view(torch.int32)

    def read(self):
        """One device-to-host copy -> (counters [3], norms [64], flags [64]) as Python lists."""
        host = self.buf.cpu()
        return (host[self._COUNTERS:self._COUNTERS + 24].view(torch.int64).tolist(), host[self._NORMS:self._RING].view(torch.float64).tolist(),
                host[self._RING:self._SKIP].view(torch.int32).tolist())


def step_guard(gnorm_sqs, grad_scale, attempt, guard):
    """The guard's single-thread launch: guard.skip = any of the device scalars `gnorm_sqs` non-finite; rings and counters."""
    n = len(gnorm_sqs)
    ptrs = (C.c_void_p * max(n, 1))(*[t.data_ptr() for t in gnorm_sqs])
    rc = L.load().m3p_step_guard(ptrs, n, grad_scale, int(attempt), guard.skip.data_ptr(), guard.ring.data_ptr(),
                                 guard.norm_ring.data_ptr(), guard.counters.data_ptr(), L.stream())
    L.check(rc, 'm3p_step_guard')


def adam_step_ranges(p, g, m, v, w16, pieces, lr, beta1, beta2, eps, weight_decay, gnorm_sq=None, max_norm=0.0, grad_scale=1.0,
                     skip=None):
    """One launch of the fused Adam update over several pieces of the flat arenas: pieces = [(start, end, step_size, zero_grad)].
    skip: the guard's device word (m3p_adam_step_ranges_guarded), or None for the unguarded entry point."""
    pieces = [q for q in pieces if q[1] > q[0]]
    if not pieces:
        return
    n = len(pieces)
    starts = (C.c_longlong * n)(*[int(a) for a, _, _, _ in pieces])
    counts = (C.c_longlong * n)(*[int(b - a) for a, b, _, _ in pieces])
    steps = (C.c_float * n)(*[float(st) for _, _, st, _ in pieces])
    zeros = (C.c_int * n)(*[int(bool(z)) for _, _, _, z in pieces])
    if skip is not None:
        rc = L.load().m3p_adam_step_ranges_guarded(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), L.ptr(w16), starts, counts, steps,
                                                   zeros, n, lr, beta1, beta2, eps, weight_decay, L.ptr(gnorm_sq), max_norm, grad_scale,
                                                   skip.data_ptr(), L.stream())
        return L.check(rc, 'm3p_adam_step_ranges_guarded')
    rc = L.load().m3p_adam_step_ranges(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), L.ptr(w16), starts, counts, steps, zeros, n,
                                       lr, beta1, beta2, eps, weight_decay, L.ptr(gnorm_sq), max_norm, grad_scale, L.stream())
    L.check(rc, 'm3p_adam_step_ranges')


def _ema_pieces(pieces):
    n = len(pieces)
    starts = (C.c_longlong * max(n, 1))(*[int(a) for a, _ in pieces])
    counts = (C.c_longlong * max(n, 1))(*[int(b) - int(a) for a, b in pieces])
    return starts, counts, n


def ema_update(p, ema, pieces, w, skip=None):
    """ema += w * (p - ema) over the pieces [(start, end)] of two flat fp32 arenas (m3p_ema_update; the rule's fp32 arithmetic
    is in include/m3p_hip.h).  w: 1 - decay, rounded to fp32 here.  skip: the guard's device word or None."""
    starts, counts, n = _ema_pieces(pieces)
    if n == 0:
        return
    rc = L.load().m3p_ema_update(p.data_ptr(), ema.data_ptr(), starts, counts, n, float(w), L.ptr(skip), L.stream())
    L.check(rc, 'm3p_ema_update')


def ema_swap(p, ema, w16, pieces):
    """p <-> ema over the pieces [(start, end)], w16 = bf16(new p) (m3p_ema_swap); w16 may be None."""
    starts, counts, n = _ema_pieces(pieces)
    if n == 0:
        return
    L.check(L.load().m3p_ema_swap(p.data_ptr(), ema.data_ptr(), L.ptr(w16), starts, counts, n, L.stream()), 'm3p_ema_swap')


LAMB_MAX_CLASSES = 32          # M3P_LAMB_MAX_CLASSES of include/m3p_hip.h
_LAMB_PIECE_BYTES = 32         # M3P_LAMB_PIECE_BYTES


class LambTable:
    """The piece table of the three LAMB launches (include/m3p_hip.h): validated and laid out by m3p_lamb_table_build on the
    host, then - with `device` - copied once to device memory from pinned staging on the current stream, beside the
    workspaces sized for it (the workgroups' partial sums, the per-tensor norms).  pieces = [(start, end, tensor id,
    zero_grad, class id)] in arena order.  Built once per set of pieces and kept by the caller."""

    def __init__(self, pieces, n_tensors, n_classes, arena_elems, device=None, max_blocks=0):
        n = len(pieces)
        self.pieces = [tuple(int(x) for x in q) for q in pieces]
        self.n_pieces, self.n_tensors, self.n_classes = n, int(n_tensors), int(n_classes)
        starts = (C.c_longlong * max(n, 1))(*[q[0] for q in self.pieces])
        counts = (C.c_longlong * max(n, 1))(*[q[1] - q[0] for q in self.pieces])
        tids = (C.c_int * max(n, 1))(*[q[2] for q in self.pieces])
        zeros = (C.c_int * max(n, 1))(*[int(bool(q[3])) for q in self.pieces])
        cls = (C.c_int * max(n, 1))(*[q[4] for q in self.pieces])
        host_pieces = torch.zeros(max(n, 1) * _LAMB_PIECE_BYTES, dtype=torch.uint8)
        host_tblk = torch.zeros(max(self.n_tensors, 0) + 1, dtype=torch.int32)
        n_blocks = C.c_int(0)
        rc = L.load().m3p_lamb_table_build(starts, counts, tids, zeros, cls, n, self.n_tensors, self.n_classes, int(arena_elems),
                                           int(max_blocks), host_pieces.data_ptr(), host_tblk.data_ptr(), C.byref(n_blocks))
        L.check(rc, 'm3p_lamb_table_build')
        self.n_blocks = n_blocks.value
        self.blk0 = host_pieces.view(torch.int32).view(n, 8)[:, 7].tolist() + [self.n_blocks]     # first workgroup of each piece
        self.tensor_blk0 = host_tblk.tolist()
        self.dev_pieces = self.dev_tblk = self.partials = self.norms = None
        if device is not None:
            self._staging = (host_pieces.pin_memory(), host_tblk.pin_memory())     # alive until the copies have run
            self.dev_pieces = self._staging[0].to(device, non_blocking=True)
            self.dev_tblk = self._staging[1].to(device, non_blocking=True)
            self.partials = torch.empty(2 * self.n_blocks, dtype=torch.float64, device=device)
            self.norms = torch.zeros((self.n_tensors, 2), dtype=torch.float64, device=device)

    def quads_per_thread(self):
        """The most 16-byte quads one thread of the update launch adds into its running sums, per piece."""
        return [-(-((e - s) // 4) // (256 * (b1 - b0))) for (s, e, _, _, _), b0, b1 in zip(self.pieces, self.blk0, self.blk0[1:])]


def _lamb_classes(classes, n_classes):
    """classes = [(rbc1, rbc2, wd_t, adapt_t)] -> the four host arrays of the C entries."""
    assert len(classes) == n_classes, (len(classes), n_classes)
    n = len(classes)
    return ((C.c_float * n)(*[float(c[0]) for c in classes]), (C.c_float * n)(*[float(c[1]) for c in classes]),
            (C.c_float * n)(*[float(c[2]) for c in classes]), (C.c_int * n)(*[int(bool(c[3])) for c in classes]))


def lamb_update(p, g, m, v, table, classes, beta1, beta2, eps, gnorm_sq=None, max_norm=0.0, grad_scale=1.0, skip=None):
    """First LAMB launch: m, v updated, r written over g, the workgroups' (sum p^2, sum r^2) into table.partials.
    skip (here and in the two launches below): the guard's device word -> the _guarded entry point; None -> the unguarded one."""
    rbc1, rbc2, wd, adapt = _lamb_classes(classes, table.n_classes)
    if skip is not None:
        rc = L.load().m3p_lamb_update_guarded(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), table.dev_pieces.data_ptr(),
                                              table.n_pieces, table.n_blocks, rbc1, rbc2, wd, adapt, table.n_classes, beta1, beta2, eps,
                                              L.ptr(gnorm_sq), max_norm, grad_scale, table.partials.data_ptr(), skip.data_ptr(), L.stream())
        return L.check(rc, 'm3p_lamb_update_guarded')
    rc = L.load().m3p_lamb_update(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), table.dev_pieces.data_ptr(), table.n_pieces,
                                  table.n_blocks, rbc1, rbc2, wd, adapt, table.n_classes, beta1, beta2, eps, L.ptr(gnorm_sq),
                                  max_norm, grad_scale, table.partials.data_ptr(), L.stream())
    L.check(rc, 'm3p_lamb_update')


def lamb_norms(table, skip=None):
    """Second launch: table.norms[t] = (sum p^2, sum r^2) over tensor t's workgroups, fp64, in a fixed order."""
    if skip is not None:
        rc = L.load().m3p_lamb_norms_guarded(table.partials.data_ptr(), table.dev_tblk.data_ptr(), table.n_tensors, table.norms.data_ptr(),
                                             skip.data_ptr(), L.stream())
        return L.check(rc, 'm3p_lamb_norms_guarded')
    rc = L.load().m3p_lamb_norms(table.partials.data_ptr(), table.dev_tblk.data_ptr(), table.n_tensors, table.norms.data_ptr(), L.stream())
    L.check(rc, 'm3p_lamb_norms')


def lamb_apply(p, r, w16, table, classes, lr, skip=None):
    """Third launch: p -= lr * phi_t * r with phi_t from table.norms; bf16 copy refreshed, r zeroed where the piece says so."""
    _, _, _, adapt = _lamb_classes(classes, table.n_classes)
    if skip is not None:
        rc = L.load().m3p_lamb_apply_guarded(p.data_ptr(), r.data_ptr(), L.ptr(w16), table.dev_pieces.data_ptr(), table.n_pieces,
                                             table.n_blocks, table.norms.data_ptr(), adapt, table.n_classes, lr, skip.data_ptr(), L.stream())
        return L.check(rc, 'm3p_lamb_apply_guarded')
    rc = L.load().m3p_lamb_apply(p.data_ptr(), r.data_ptr(), L.ptr(w16), table.dev_pieces.data_ptr(), table.n_pieces, table.n_blocks,
                                 table.norms.data_ptr(), adapt, table.n_classes, lr, L.stream())
    L.check(rc, 'm3p_lamb_apply')


def transpose_bf16(src, dst):
    """dst[c, r] = src[r, c]; dst may have a row pitch larger than rows (pad columns untouched)."""
    rows, cols = src.shape
    rc = L.load().m3p_transpose_bf16(src.data_ptr(), dst.data_ptr(), rows, cols, src.stride(0), dst.stride(0), L.stream())
    L.check(rc, 'm3p_transpose_bf16')


def gelu_fwd(u, grad_inplace=False):
    """h = gelu_erf(u).  With grad_inplace, u is overwritten by gelu_erf'(u) (bf16) for EPI_MUL in backward."""
    h = torch.empty_like(u)
    L.check(L.load().m3p_gelu_fwd(u.data_ptr(), h.data_ptr(), u.data_ptr() if grad_inplace else None, u.numel(), L.stream()),
            'm3p_gelu_fwd')
    return h


GQ_OFF, GQ_STEP = 27.0 / 201.0, 1.0 / 201.0       # the byte code of gelu' (csrc/common.hpp): gelu' ~ code * GQ_STEP - GQ_OFF


def gq_eligible(M, N):
    """Shapes whose FFN runs on the byte-derivative form: whole 256 x 256 tiles of the eight-wave kernel."""
    return M >= 1024 and M % 256 == 0 and N % 256 == 0 and N >= 512


def gelu_fwd_gq(u):
    """(h = gelu_erf(u) bf16 [M, N], gq uint8 [M * N]): gq holds gelu_erf'(u) as one byte per element in the fragment
    order of the eight-wave GEMM (include/m3p_hip.h: m3p_gelu_fwd_gq) - what gemm_nt(..., EPI_MULQ, aux=gq) multiplies by.
    u is dead afterwards."""
    _chk_bf16(u)
    M, N = u.shape
    assert u.is_contiguous() and gq_eligible(M, N), (M, N)
    h = torch.empty_like(u)
    gq = torch.empty((M * N,), dtype=torch.uint8, device=u.device)
    L.check(L.load().m3p_gelu_fwd_gq(u.data_ptr(), h.data_ptr(), gq.data_ptr(), M, N, L.stream()), 'm3p_gelu_fwd_gq')
    return h, gq


def gq_unpack(gq, M, N):
    """The decoded derivative as a float [M, N] matrix in row order (tests): inverse of the fragment-order layout."""
    t = gq.view(M // 256, N // 256, 2, 4, 8, 4, 16, 4, 4)       # tm, tn, wm, wn, i, fg, fr, j, r
    t = t.permute(0, 2, 4, 6, 1, 3, 7, 5, 8).reshape(M, N)     # rows: tm, wm, i, fr   cols: tn, wn, j, fg, r
    return t.float() * GQ_STEP - GQ_OFF


def gelu_fwd_q8(u, scale, amax=None):
    """(h = gelu_erf(u) bf16, h8 = e4m3(scale * h) uint8) in one pass; amax (fp32 [1]) is raised to max |h|."""
    h = torch.empty_like(u)
    h8 = torch.empty(u.shape, dtype=torch.uint8, device=u.device)
    L.check(L.load().m3p_gelu_fwd_q8(u.data_ptr(), h.data_ptr(), h8.data_ptr(), u.numel(), scale.data_ptr(), L.ptr(amax), L.stream()),
            'm3p_gelu_fwd_q8')
    return h, h8


def transpose_batch(desc, n_desc, max_tiles):
    L.check(L.load().m3p_transpose_batch_bf16(desc.data_ptr(), n_desc, max_tiles, L.stream()), 'm3p_transpose_batch_bf16')


def itm_head_fwd(first, W1_16, b1, w2, b2):
    """first: bf16 [B, d] (hidden[:, 0]); W1_16: bf16 [d, d] working copy of pooled_layer.dense.weight.
    Returns (h16 contiguous bf16 copy of the input rows, pooled fp32 [B, d], scores fp32 [B])."""
    _chk_bf16(first, W1_16)
    B, d = first.shape
    h16 = first.contiguous()
    pre = gemm_nt(h16, W1_16, L.EPI_BIAS, bias=b1)
    pooled = torch.empty((B, d), dtype=torch.float32, device=first.device)
    scores = torch.empty((B,), dtype=torch.float32, device=first.device)
    rc = L.load().m3p_itm_score_fwd(pre.data_ptr(), w2.data_ptr(), b2.data_ptr(), pooled.data_ptr(), scores.data_ptr(),
                                    B, d, L.stream())
    L.check(rc, 'm3p_itm_score_fwd')
    return h16, pooled, scores


def itm_head_bwd(dscores, h16, pooled, W1_16, w2, dW1, db1, dw2, db2):
    """Returns dh bf16 [B, d]; accumulates dW1 [d,d], db1, dw2 [d], db2 [1] (fp32) in place."""
    B, d = h16.shape
    dev = h16.device
    ldt = (B + 7) // 8 * 8
    dpre16 = torch.empty((B, d), dtype=BF16, device=dev)
    dpreT16 = torch.zeros((d, ldt), dtype=BF16, device=dev)
    assert dscores.dtype == torch.float32 and dscores.is_contiguous() and dscores.numel() == B
    rc = L.load().m3p_itm_score_bwd(dscores.data_ptr(), pooled.data_ptr(), w2.data_ptr(), dpre16.data_ptr(),
                                    dpreT16.data_ptr(), ldt, db1.data_ptr(), dw2.data_ptr(), db2.data_ptr(), B, d, L.stream())
    L.check(rc, 'm3p_itm_score_bwd')
    gemm_wgrad(dpre16, h16, dW1)                         # dW1[j][k] += sum_b dpre[b][j] h[b][k]
    dh32 = torch.zeros((B, d), dtype=torch.float32, device=dev)
    gemm_wgrad(dpreT16, W1_16, dh32, n=B)                # dh[b][k]  = sum_j dpre[b][j] W1[j][k]
    return dh32.to(BF16)


def gelu_bwd(dy, u):
    """du = dy * gelu_erf'(u) (bf16)."""
    _chk_bf16(dy, u)
    assert dy.shape == u.shape and dy.is_contiguous() and u.is_contiguous()
    du = torch.empty_like(dy)
    L.check(L.load().m3p_gelu_bwd(dy.data_ptr(), u.data_ptr(), du.data_ptr(), dy.numel(), L.stream()), 'm3p_gelu_bwd')
    return du


def mse_fwd_bwd(pred, tgt, grad_scale):
    """pred bf16 [n, c], tgt fp32 [n, c] -> (sum of squared errors as a 1-element fp32 tensor, dpred bf16 = 2 (pred - tgt) grad_scale)."""
    _chk_bf16(pred)
    n, c = pred.shape
    assert tgt.shape == (n, c) and tgt.dtype == torch.float32 and pred.stride(1) == 1 and tgt.stride(1) == 1
    dpred = torch.empty_like(pred)
    row_sq = torch.empty((n,), dtype=torch.float32, device=pred.device)
    rc = L.load().m3p_mse_fwd_bwd(pred.data_ptr(), pred.stride(0), tgt.data_ptr(), tgt.stride(0), dpred.data_ptr(),
                                  row_sq.data_ptr(), n, c, grad_scale, L.stream())
    L.check(rc, 'm3p_mse_fwd_bwd')
    return row_sq.sum().reshape(1), dpred



def dropout_rows(x, p_drop, seed, res=None, out=None, rng_ld=None, rng_col0=0):
    """out = (res or 0) + dropout(x) on a 2-D bf16 view (last dim contiguous; x / res / out may be column slices of
    wider buffers).  The keep bit of element (r, c) is rng.keep(r * rng_ld + rng_col0 + c): rng_ld defaults to
    x.shape[1].  out may be x."""
    _chk_bf16(x)
    rows, cols = x.shape
    assert x.stride(1) == 1 and (res is None or (res.dtype == BF16 and res.stride(1) == 1 and res.shape == x.shape))
    if out is None:
        out = torch.empty((rows, cols), dtype=BF16, device=x.device)
    assert out.dtype == BF16 and out.stride(1) == 1 and out.shape == x.shape
    th, ik = _drop_args(p_drop)
    rc = L.load().m3p_dropout_rows(x.data_ptr(), x.stride(0), L.ptr(res), res.stride(0) if res is not None else 0,
                                   out.data_ptr(), out.stride(0), rows, cols, cols if rng_ld is None else rng_ld, rng_col0,
                                   seed, th, ik, L.stream())
    L.check(rc, 'm3p_dropout_rows')
    return out


def glu_fwd(ab):
    """nn.GLU: ab bf16 [rows, 2d] -> ab[:, :d] * sigmoid(ab[:, d:])."""
    _chk_bf16(ab)
    rows, d2 = ab.shape
    assert ab.is_contiguous() and d2 % 2 == 0
    y = torch.empty((rows, d2 // 2), dtype=BF16, device=ab.device)
    L.check(L.load().m3p_glu_fwd(ab.data_ptr(), d2, y.data_ptr(), rows, d2 // 2, L.stream()), 'm3p_glu_fwd')
    return y


def glu_bwd(ab, dy):
    _chk_bf16(ab, dy)
    rows, d2 = ab.shape
    assert ab.is_contiguous() and dy.is_contiguous() and dy.shape == (rows, d2 // 2)
    dab = torch.empty_like(ab)
    L.check(L.load().m3p_glu_bwd(ab.data_ptr(), d2, dy.data_ptr(), dab.data_ptr(), rows, d2 // 2, L.stream()), 'm3p_glu_bwd')
    return dab
