"""The row kernels behind the shifted-exponential MLM head (csrc/heads.hip: ce_shift_*), each called on its own at the smallest
sizes that reach its loops and splits, against fp64 references on the device (GPU).

Every size is derived from the launcher's rule - constants copied below beside the line they come from - and each test asserts
the premise that puts it on the path it names.  Every element is held to a bound from the rounding model of tests/util.py; the
CPU tests of tests/test_parity_bounds.py show those bounds accepting an fp32 restatement of each kernel and rejecting a dropped
partial sum, a dropped tail, a row scaled by its neighbour's factor, an unwritten second trip and a lost repeat."""
import math

import pytest
import torch

from tests.util import (CE_LSE_SPLIT, CE_SHIFT, F32_OUT, KAPPA, U32, assert_accum_bound, assert_bits_equal, assert_shift_rows_bound,
                        poisoned_outputs, scale_rows_bound, shift_dh_bound, target_rows_bound)

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16

# --- the launchers' grid rules (m3p_amd/csrc/heads.hip) ------------------------------------------------------------------
THREADS = 256                     # every kernel here: __launch_bounds__(256)
TARGET_TRIP = 256                 # ce_shift_target_kernel: 64 lanes x 4 columns per trip of `c += 256`
PARTIAL_UNROLL_FROM = 13          # ce_shift_partial_kernel: a wave enters `b + 12 < b1` once its split holds 13 blocks
CE_RB, CE_CB = 64, 2048           # rows / columns of a tile of ce_shift_colsum_tile_kernel
COLSUM_SPLIT_FROM = 16            # m3p_ce_shift_colsum: the reduction over row groups splits 8 ways from 16 groups
SHIFT_MAXBLK = 2048               # ce_shift_blocks: blocks = min(ceil(n d / 4 / 256), 2048), one 4-element chunk per thread and trip
TARGET_ROWS_MAXBLK = 4096         # m3p_ce_shift_target_rows: blocks = min(ceil(n / 4), 4096), one row per wave and trip

WORST = {}                        # kernel -> the largest normalised error seen, printed by the last test of the module


def _note(name, worst):
    WORST[name] = max(WORST.get(name, 0.0), float(worst))
    print('%-40s worst error %.3g x its bound' % (name, float(worst)))


def _gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


# =====================================================================================================================
# (a) the target's own logit
# =====================================================================================================================
@pytest.mark.parametrize('d', [4, 260, 768, 1024])
def test_ce_shift_target_widths(d):
    """One lane group (d = 4), a ragged second trip of the wave's loop (260), three and four whole trips (768, 1024); five rows,
    so the second workgroup is partly idle; the first word, the last one and a repeated id."""
    from m3p_amd import ops
    n, V = 5, 300
    trips = -(-d // TARGET_TRIP)
    assert trips == {4: 1, 260: 2, 768: 3, 1024: 4}[d] and (d % TARGET_TRIP != 0) == (d in (4, 260))
    assert n % 4 != 0 and -(-n // 4) > 1                               # (four rows per workgroup)
    gen = _gen(d)
    h = torch.randn((n, d), device='cuda', generator=gen).to(BF16)
    emb = (torch.randn((V, d), device='cuda', generator=gen) * (1.2 / math.sqrt(d))).to(BF16)
    bias = torch.randn((V,), device='cuda', generator=gen) * 0.5
    y = torch.tensor([0, V - 1, 17, 17, 123], device='cuda')
    with poisoned_outputs():
        row_t, row_ref = ops.ce_shift_target(h, emb, bias, y)
    e64 = emb.double()[y]
    t64 = (h.double() * e64).sum(1) + bias.double()[y]
    at64 = (h.double().abs() * e64.abs()).sum(1) + bias.double()[y].abs()
    # a depth-d fp32 dot product plus the bias: bound (a) of test_shifted_exponential_epilogue_every_element
    err = (row_t.double() - t64).abs() / (KAPPA * math.sqrt(d) * U32 * at64 + F32_OUT * t64.abs() + 1e-300)
    _note('ce_shift_target_kernel d=%d' % d, torch.nan_to_num(err, nan=math.inf).max())
    assert float(torch.nan_to_num(err, nan=math.inf).max()) <= 1.0, err.tolist()
    assert_bits_equal(row_ref[:, 0].contiguous().view(torch.float32), row_t + CE_SHIFT, 'the shift is the target logit + 40')
    assert torch.equal(row_ref[:, 1].long(), y)


# =====================================================================================================================
# (b, c) block sums -> loss, s, q and the column sums
# =====================================================================================================================
E_COLS_MAX = 64 * 547             # widest synthetic e: [64, 35008]; the 3907-block case reads a narrower one (see below)


def _block_sum_case(n, n_blocks, seed):
    """stats fp32 [n_blocks, n], positive, block magnitudes spread over e^-2 .. e^2 inside a row, every row's sum scaled to
    e^-40 r_n with log r_n spread evenly over [-30, 30] (in a shuffled order); e bf16 [n, ld] of positive values with exact
    zeros among them.  The two are independent inputs of the launcher."""
    gen = _gen(seed)
    raw = torch.exp(torch.empty((n_blocks, n), dtype=torch.float64, device='cuda').uniform_(-2.0, 2.0, generator=gen))
    logr = torch.linspace(-30.0, 30.0, n, dtype=torch.float64, device='cuda')[torch.randperm(n, device='cuda', generator=gen)]
    stats = (raw / raw.sum(0) * torch.exp(logr - CE_SHIFT)).float().contiguous()
    # the logits of the 3907 blocks of a 250 002-word vocabulary are not materialised here: the column sums read e alone, and
    # their tiles are covered by the other sizes (64 .. 35 008 columns)
    ld = min(64 * n_blocks, E_COLS_MAX)
    e = torch.empty((n, ld), device='cuda').uniform_(0.0, 2.0, generator=gen).to(BF16)
    e[:, ::37] = 0
    e[torch.arange(n, device='cuda'), torch.randint(0, ld, (n,), device='cuda', generator=gen)] = 0
    return stats, e


@pytest.mark.parametrize('n,n_blocks', [(64, 1), (64, 31), (64, 33), (64, 80), (1024, 80), (64, 416), (64, 547), (64, 3907)])
def test_ce_shift_from_block_sums_synthetic(n, n_blocks):
    """Fewer blocks than splits (1, 31), empty trailing splits (33), the size of the `tiles` head (80), the first size whose
    waves run the unrolled loop (416 = 32 x 13), an unrolled part with a ragged tail (547), the block count of V = 250 002
    (3907); 1024 rows once, where the column sums' reduction over 16 row groups splits eight ways."""
    from m3p_amd import ops
    per = -(-n_blocks // CE_LSE_SPLIT)
    live_splits = -(-n_blocks // per)
    assert n % 64 == 0
    assert (n_blocks < CE_LSE_SPLIT) == (n_blocks in (1, 31))
    if n_blocks == 33:
        assert per == 2 and live_splits == 17                           # splits 17 .. 31 start past the last block
    if n_blocks == 416:
        assert per == PARTIAL_UNROLL_FROM and live_splits == CE_LSE_SPLIT
    assert (per >= PARTIAL_UNROLL_FROM) == (n_blocks in (416, 547, 3907))
    if n_blocks == 547:
        assert per == 18 and per % 16 != 0                              # waves 0 and 1: one unrolled trip, then one more block
    assert (-(-n // CE_RB) >= COLSUM_SPLIT_FROM) == (n == 1024)
    stats, e = _block_sum_case(n, n_blocks, 100 + n_blocks + n)
    ld = e.shape[1]
    if n_blocks in (33, 80, 547):
        assert ld % CE_CB != 0 and ld > CE_CB                           # a last column tile that is not whole
    # both branches of ce_shift_final_kernel (sum < e^-40 and beyond) hold at least a quarter of the rows
    small = float((stats.double().sum(0).cpu() < math.exp(-CE_SHIFT)).double().mean())
    assert 0.25 <= small <= 0.75, small
    gs = 1.0 / n
    with poisoned_outputs():
        loss_sum, row_loss, row_s, row_q, cs = ops.ce_shift_from_block_sums(e, stats, 1.0 / n, gs)
    what = 'ce_shift_from_block_sums n=%d n_blocks=%d' % (n, n_blocks)
    worst = assert_shift_rows_bound(row_loss, row_s, row_q, stats, gs, what)
    for k, w in worst.items():
        _note('ce_shift_partial/final_kernel %s n=%d blocks=%d' % (k, n, n_blocks), w)
    # the summed loss is the fp32 sum of the kernel's own rows times the scale
    ref_sum = float(row_loss.double().sum()) / n
    assert abs(float(loss_sum) - ref_sum) <= KAPPA * math.sqrt(n) * U32 * ref_sum + F32_OUT * ref_sum
    # the column sums over the kernel's own row_s, n terms each, all ld columns
    e64, s64 = e.double(), row_s.double()[:, None]
    assert cs.shape == (ld,)
    _note('ce_shift_colsum n=%d ld=%d' % (n, ld), assert_accum_bound(cs, (s64 * e64).sum(0), (s64.abs() * e64).sum(0), n, what=what + ': colsum'))


# =====================================================================================================================
# (d, f) the rows scaled by s_n, and the data gradient's epilogue
# =====================================================================================================================
def _row_case(n, d, seed, V=300):
    gen = _gen(seed)
    h = torch.randn((n, d), device='cuda', generator=gen).to(BF16)
    dh32 = torch.randn((n, d), device='cuda', generator=gen) * 3.0
    emb = (torch.randn((V, d), device='cuda', generator=gen) * 0.7).to(BF16)
    row_s = torch.randn((n,), device='cuda', generator=gen) * 2.0          # (both signs)
    row_q = torch.randn((n,), device='cuda', generator=gen)
    y = torch.randint(0, V, (n,), device='cuda', generator=gen)
    if n == 1:
        y[0] = V - 1
    else:
        y[0], y[1] = 0, V - 1                                              # the first and the last row of the matrix
        y[10:20] = 7                                                       # a run of equal ids
    g = torch.tensor([0.5], device='cuda')
    return h, dh32, emb, row_s, row_q, y, g


ROW_CASES = [(1, 4), (70, 260), (2112, 1024)]


def _assert_row_premise(n, d):
    chunks = n * d // 4
    assert (chunks > SHIFT_MAXBLK * THREADS) == ((n, d) == (2112, 1024))   # 540 672 chunks: some threads take a second trip
    assert ((d // 4) % 64 != 0) == ((n, d) != (2112, 1024))                # rows that do not end on a wave


@pytest.mark.parametrize('n,d', ROW_CASES)
def test_ce_shift_scale_rows(n, d):
    from m3p_amd import ops
    _assert_row_premise(n, d)
    h, _, _, row_s, _, _, g = _row_case(n, d, 7 * n + d)
    with poisoned_outputs():
        out = ops.ce_shift_scale_rows(h, row_s, g)
    worst, at = scale_rows_bound(out, h, row_s, 0.5)
    _note('ce_shift_scale_rows_kernel (%d, %d)' % (n, d), worst)
    assert worst <= 1.0, (worst, at)


@pytest.mark.parametrize('n,d', ROW_CASES)
def test_ce_shift_dh(n, d):
    from m3p_amd import ops
    _assert_row_premise(n, d)
    _, dh32, emb, row_s, row_q, y, g = _row_case(n, d, 11 * n + d)
    if n > 1:
        assert int(y[0]) == 0 and int(y[1]) == emb.shape[0] - 1 and bool((y[10:20] == 7).all())
    with poisoned_outputs():
        out = ops.ce_shift_dh(dh32, emb, y, row_s, row_q, g)
    worst, at = shift_dh_bound(out, dh32, emb[y], row_s, row_q, 0.5)
    _note('ce_shift_dh_kernel (%d, %d)' % (n, d), worst)
    assert worst <= 1.0, (worst, at)


# =====================================================================================================================
# (e) the targets' fp32 terms, added with atomics
# =====================================================================================================================
@pytest.mark.parametrize('pattern', ['one_id', 'ten_words', 'distinct'])
@pytest.mark.parametrize('n,d', [(3, 64), (257, 68), (16389, 64)])
def test_ce_shift_target_rows(n, d, pattern):
    """Three rows; a width that is ragged against the wave (68 = 64 + 4) over more than one workgroup; more rows than one
    trip of the capped grid covers (16 384).  Every row the same id (the deepest sum), ids drawn from ten words, all distinct.
    The kernel adds: it starts from random numbers, and what no row with a non-zero q_n names keeps its bits."""
    from m3p_amd import ops
    assert (n > 4 * TARGET_ROWS_MAXBLK) == (n == 16389) and (d % 64 != 0) == (d == 68)
    V = n + 11
    gen = _gen(13 * n + d + len(pattern))
    h = torch.randn((n, d), device='cuda', generator=gen).to(BF16)
    row_q = torch.randn((n,), device='cuda', generator=gen)
    row_q[::5] = 0.0                                                       # rows that add nothing
    if pattern == 'one_id':
        y = torch.full((n,), 5, dtype=torch.int64, device='cuda')
    elif pattern == 'ten_words':
        words = torch.tensor([0, V - 1, 3, 4, 5, 6, 7, V // 2, V - 3, V - 2], device='cuda')
        y = words[torch.randint(0, 10, (n,), device='cuda', generator=gen)]
    else:
        y = torch.randperm(V, device='cuda', generator=gen)[:n].contiguous()
        assert int(torch.bincount(y).max()) == 1
    g = torch.tensor([0.5], device='cuda')
    demb0 = torch.randn((V, d), device='cuda', generator=gen)
    dbias0 = torch.randn((V,), device='cuda', generator=gen)
    demb, dbias = demb0.clone(), dbias0.clone()
    ops.ce_shift_target_rows(h, y, row_q, g, demb, dbias)
    torch.cuda.synchronize()
    what = 'ce_shift_target_rows (%d, %d) %s' % (n, d, pattern)
    (we, at_e), (wb, at_b) = target_rows_bound(demb, dbias, demb0, dbias0, h, y, row_q, 0.5)
    _note('ce_shift_target_rows_kernel demb (%d, %d) %s' % (n, d, pattern), we)
    _note('ce_shift_target_rows_kernel dbias (%d, %d) %s' % (n, d, pattern), wb)
    assert we <= 1.0, (what, we, at_e)
    assert wb <= 1.0, (what, wb, at_b)
    live = torch.bincount(y[row_q != 0], minlength=V) > 0                  # words some row with a non-zero q_n names
    assert int((~live).sum()) >= 11
    if pattern == 'distinct':
        assert int((torch.bincount(y, minlength=V) > 0).sum()) > int(live.sum())      # named, but only by rows whose q_n is 0
    assert_bits_equal(demb[~live], demb0[~live], what + ': rows of demb that no contributing row names')
    assert_bits_equal(dbias[~live], dbias0[~live], what + ': entries of dbias that no contributing row names')


def test_zz_report_worst_normalised_errors():
    """Not a check: prints what the bounds above were reached by (run with -s or -rP)."""
    for k in sorted(WORST):
        print('worst normalised error  %-64s %.3f' % (k, WORST[k]))
