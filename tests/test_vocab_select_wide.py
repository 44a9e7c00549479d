"""Beam search beyond 8 beams on the device (csrc/select.hip: m3p_vocab_select_wide; ops.vocab_select_wide).

The contract is m3p_vocab_select's (tests/test_vocab_select.py), and so is the check: lse held to fp64 within 1e-5 on logits
with |x| <= 16, then indices equal and scores bit-equal to ref_select run on the kernel's own lse; NaN and inf planted behind
column V, outputs poisoned before the launch.  On uniform bf16 rows the k-th place of a row lies inside a class of equal
logits as a rule (V = 1000 values on a grid of a few hundred near the top), which is what the count selection's tie quota is
for.  The CPU part - the plan and the two-phase argument - is tests/test_vocab_select_wide_cpu.py."""
import numpy as np
import pytest
import torch

from tests.test_vocab_select import CHUNK, _beam_scores, _logits, ref_select
from tests.util import assert_bits_equal, poisoned_outputs


def _check(full, V, beam_scores, beam, k, what):
    """Run the wide entry on `full` (CPU bf16 [n, ld]) and hold it to the contract.  -> (scores, flat_idx, lse) as numpy."""
    from m3p_amd import ops
    n = full.shape[0]
    dev = full.cuda()
    bsc = None if beam_scores is None else torch.as_tensor(beam_scores, dtype=torch.float32).cuda()
    with poisoned_outputs():
        res = ops.vocab_select_wide(dev, V, bsc, beam, k)
    assert res is not None, what
    scores, flat_idx, lse = res
    torch.cuda.synchronize()
    assert scores.shape == (n // beam, k) and flat_idx.shape == (n // beam, k) and lse.shape == (n,)
    assert scores.dtype == torch.float32 and flat_idx.dtype == torch.int64 and lse.dtype == torch.float32
    ref_lse = torch.logsumexp(dev[:, :V].double(), dim=1)
    err = float((lse.double() - ref_lse).abs().max())
    print('%s: max |lse - fp64| = %.3g' % (what, err))
    assert err <= 1e-5, (what, err)
    x32 = full[:, :V].float().numpy()
    zeros = np.zeros(n, np.float32)
    exp_s, exp_i = ref_select(x32, lse.cpu().numpy(), zeros if beam_scores is None else np.asarray(beam_scores, np.float32), beam, k)
    got_i = flat_idx.cpu().numpy()
    assert np.array_equal(got_i, exp_i), (what, got_i.tolist(), exp_i.tolist())
    assert_bits_equal(scores.cpu(), torch.from_numpy(exp_s), what + ' scores')
    return scores.cpu().numpy(), got_i, lse.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('V,ld,bs,beam,k', [
    (1000, 1024, 3, 9, 18),                         # the narrowest wide beam, one partial chunk
    (2 * CHUNK + 2, 8448, 2, 12, 24),               # whole chunks plus two columns
    (2059, 2304, 2, 16, 32),                        # the chunk's second-half tail
    (1000, 1024, 2, 32, 64),                        # the widest
    (40, 40, 2, 16, 32),                            # K is most of the row
    (250002, 250112, 1, 10, 20),                    # the full width
    (1000, 1024, 1, 1, 17),                         # one row
])
def test_vocab_select_wide_shapes(V, ld, bs, beam, k):
    assert ld % 8 == 0 and V <= ld < V + 256
    n = bs * beam
    full, x = _logits(n, V, ld, seed=V + n)
    what = 'V %d bs %d beam %d k %d' % (V, bs, beam, k)
    _check(full, V, _beam_scores(n, 7), beam, k, what)
    # how many rows have their k-th place inside a class of equal logits (printed: the intended rule on these rows)
    srt = np.sort(x.float().numpy(), axis=1)[:, ::-1]
    if k < V:
        print('%s: %d of %d rows tie across the k-th place' % (what, int((srt[:, k - 1] == srt[:, k]).sum()), n))


@pytest.mark.gpu
@pytest.mark.parametrize('V,ld,bs,beam,k', [(1000, 1024, 3, 2, 4), (2 * CHUNK + 2, 8448, 2, 8, 16)])
def test_vocab_select_wide_equals_the_narrow_entry_bit_for_bit(V, ld, bs, beam, k):
    from m3p_amd import ops
    n = bs * beam
    full, _ = _logits(n, V, ld, seed=V + n + 1)
    dev = full.cuda()
    bsc = torch.from_numpy(_beam_scores(n, 9)).cuda()
    for b in (bsc, None):
        with poisoned_outputs():
            wide = ops.vocab_select_wide(dev, V, b, beam, k)
            narrow = ops.vocab_select(dev, V, b, beam, k)
        assert wide is not None and narrow is not None
        assert torch.equal(wide[1], narrow[1])
        assert_bits_equal(wide[0].cpu(), narrow[0].cpu(), 'scores')
        assert_bits_equal(wide[2].cpu(), narrow[2].cpu(), 'lse')


@pytest.mark.gpu
def test_vocab_select_wide_lse_has_the_narrow_bits_at_wide_k():
    from m3p_amd import ops
    V, ld, beam, k = 2 * CHUNK + 2, 8448, 9, 18
    full, _ = _logits(2 * beam, V, ld, seed=21)
    dev = full.cuda()
    wide = ops.vocab_select_wide(dev, V, None, beam, k)
    narrow = ops.vocab_select(dev, V, None, 1, 1)
    assert_bits_equal(wide[2].cpu(), narrow[2].cpu(), 'lse')


@pytest.mark.gpu
def test_vocab_select_wide_planted_cases():
    """Maxima at the ends of the row and at a chunk boundary, a class of equal logits across the chunks whose quota ends in the
    middle one, identical rows, rows at -1e9, the first step, a row with 10 finite logits, beam_scores = None."""
    V, ld, bs, beam, k = 2 * CHUNK + 2, 8448, 3, 9, 18
    n = bs * beam
    full, _ = _logits(n, V, ld, seed=11, amp=8.0)
    top = 12.0
    full[0, 0] = top                                    # sentence 0: the maximum in column 0,
    full[1, V - 1] = top                                # in column V - 1,
    full[2, 2 * CHUNK] = top                            # in the first column of the last chunk
    # sentence 1, beam 0: 4 above, then a class of 40 equal logits - 10 in chunk 0, 28 in chunk 1, 2 in chunk 2; the row's
    # quota of 18 - 4 = 14 ends at the 4th member inside the middle chunk
    above = [3, CHUNK + 1, CHUNK + 4000, V - 3]
    cls = [50 + 300 * i for i in range(10)] + [CHUNK + 17 + 100 * i for i in range(28)] + [2 * CHUNK, V - 1]
    r = beam
    for w in above:
        full[r, w] = top
    for w in cls:
        full[r, w] = 11.0
    full[2 * beam, 100], full[2 * beam, CHUNK + 904] = 11.0, 10.5      # sentence 2: beams 0 and 1 identical, equal beam scores
    full[2 * beam + 1] = full[2 * beam]
    bsc = np.zeros(n, np.float32)
    bsc[beam:2 * beam] = [0.0, -30.0, -30.0, -1e9, -30.0, -30.0, -30.0, -30.0, -30.0]
    bsc[2 * beam:] = [-1.0, -1.0, -3.0, -3.5, -4.0, -4.5, -5.0, -5.5, -6.0]
    _, idx, _ = _check(full, V, bsc, beam, k, 'planted')
    assert {0, 1 * V + V - 1, 2 * V + 2 * CHUNK} <= set(idx[0].tolist())
    # the other beams of sentence 1 score 30 below: beam 0 supplies all 18 - its 4 maxima by word, then the class by word
    assert idx[1].tolist() == sorted(above) + cls[:14]
    assert (idx[1] // V != 3).all()                                         # the row at -1e9 is never chosen
    got = idx[2].tolist()                                                   # equal entries: the lower beam first
    assert got[:4] == [100, V + 100, CHUNK + 904, V + CHUNK + 904]
    assert all(i - V in got[:j] for j, i in enumerate(got) if i // V == 1)
    # every row at -1e9 but one finite: the finite row supplies all k entries
    one = np.full(n, -1e9, np.float32)
    one[4::beam] = -2.0
    _, idx, _ = _check(full, V, one, beam, k, 'planted, one finite beam')
    assert (idx // V == 4).all()
    # the first step: beam 0 at 0, the others at -1e9 - all k from beam 0
    first = np.full(n, -1e9, np.float32)
    first[::beam] = 0.0
    _, idx, _ = _check(full, V, first, beam, k, 'planted, the first step')
    assert (idx // V == 0).all()
    # a row that holds 10 finite logits and -inf elsewhere (as banned words leave it); the other rows supply enough
    few = full.clone()
    keep = few[5, [7, 99, CHUNK - 1, CHUNK, CHUNK + 5, 6000, 2 * CHUNK - 1, 2 * CHUNK, V - 2, V - 1]].clone()
    few[5, :V] = float('-inf')
    few[5, [7, 99, CHUNK - 1, CHUNK, CHUNK + 5, 6000, 2 * CHUNK - 1, 2 * CHUNK, V - 2, V - 1]] = keep
    sc, idx, _ = _check(few, V, _beam_scores(n, 3), beam, k, 'planted, 10 finite logits in a row')
    assert np.isfinite(sc).all()
    # beam_scores = None is zeros
    _check(full, V, None, beam, k, 'planted, no beam scores')


@pytest.mark.gpu
def test_vocab_select_wide_is_reproducible():
    from m3p_amd import ops
    V, ld, beam, k = 2 * CHUNK + 2, 8448, 12, 24
    n = 2 * beam
    full, _ = _logits(n, V, ld, seed=33)
    dev = full.cuda()
    bsc = torch.from_numpy(_beam_scores(n, 5)).cuda()
    a = ops.vocab_select_wide(dev, V, bsc, beam, k)
    b = ops.vocab_select_wide(dev, V, bsc, beam, k)
    assert torch.equal(a[1], b[1])
    assert_bits_equal(a[0].cpu(), b[0].cpu(), 'scores')
    assert_bits_equal(a[2].cpu(), b[2].cpu(), 'lse')


@pytest.mark.gpu
def test_vocab_select_wide_declines_more_than_max_k():
    from m3p_amd import lib as L
    from m3p_amd import ops
    max_k = ops.vocab_select_wide_max_k()
    assert max_k == 64
    full, _ = _logits(2, 1000, 1024, seed=3)
    dev = full.cuda()
    assert ops.vocab_select_wide(dev, 1000, None, 1, max_k + 1) is None
    assert ops.vocab_select_wide(dev, 1000, None, 1, max_k) is not None
    small, _ = _logits(2, 40, 40, seed=4)
    with pytest.raises(L.M3PError):
        ops.vocab_select_wide(small.cuda(), 40, None, 1, 41)
