"""Word selection of the decoding loops (csrc/select.hip: m3p_vocab_select) and the owner table of the in-place beam caches
(m3p_amd/decoder.py: advance_owner).

The contract: lse[r] = the fp32 log-sum-exp of row r over its V columns; the score of entry (r, w) is
fl32(fl32(float(logit[r, w]) - lse[r]) + beam_scores[r]); per sentence the kernel returns the first k of its beam * V entries
under the total order T = (score descending, beam ascending, logit descending, word ascending), flat_idx = beam * V + word.
The reference below implements T with a lexsort on fp32 scores computed exactly as specified.  On the GPU lse is held to
fp64 within 1e-5 (logits with |x| <= 16: |lse| <= 32, where a few fp32 ulps are 4e-6 each, plus the error of a tree sum over
<= 2^18 positive terms), and the selection is then compared - indices equal, scores bit for bit - with the reference run on
the kernel's own lse."""
import numpy as np
import pytest
import torch

from tests.util import assert_bits_equal, poisoned_outputs

BF16 = torch.bfloat16
CHUNK = 4096                    # VS_CHUNK of csrc/select.hip


def ref_select(logits, lse, beam_scores, beam, k):
    """logits float32 [n, V] (bf16 values), lse float32 [n], beam_scores float32 [n] -> (scores float32 [bs, k], flat_idx
    int64 [bs, k]) under T."""
    logits = np.asarray(logits, dtype=np.float32)
    n, V = logits.shape
    bs = n // beam
    score = (logits - np.asarray(lse, np.float32)[:, None]).astype(np.float32)
    score = (score + np.asarray(beam_scores, np.float32)[:, None]).astype(np.float32)
    out_s, out_i = np.empty((bs, k), np.float32), np.empty((bs, k), np.int64)
    beam_id = np.repeat(np.arange(beam), V)
    word = np.tile(np.arange(V), beam)
    for s in range(bs):
        sc = score[s * beam:(s + 1) * beam].reshape(-1)
        lg = logits[s * beam:(s + 1) * beam].reshape(-1)
        order = np.lexsort((word, -lg, beam_id, -sc))[:k]          # (the last key is the primary one)
        out_s[s], out_i[s] = sc[order], beam_id[order] * V + word[order]
    return out_s, out_i


def _lse32(logits):
    x = np.asarray(logits, dtype=np.float64)
    m = x.max(1)
    return (m + np.log(np.exp(x - m[:, None]).sum(1))).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_reference_order_on_a_planted_example():
    V, beam, k = 6, 3, 7
    x = np.array([[1.0, 3.0, 3.0, -2.0, 0.5, 3.0],          # equal logits inside a row: words 1, 2, 5
                  [1.0, 3.0, 3.0, -2.0, 0.5, 3.0],          # the same row again, the same beam score
                  [9.0, 8.0, 7.0, 6.0, 5.0, 4.0]],          # at -1e9: every score collapses to -1e9
                 dtype=np.float32)
    bsc = np.array([-0.5, -0.5, -1e9], dtype=np.float32)
    lse = _lse32(x)
    sc, idx = ref_select(x, lse, bsc, beam, k)
    # the three equal maxima of beam 0 by word, then those of beam 1 (equal scores: the lower beam first), then the next logit
    assert idx[0].tolist() == [1, 2, 5, V + 1, V + 2, V + 5, 0]
    assert (sc[0, :6] == sc[0, 0]).all() and sc[0, 6] < sc[0, 0]
    # against a plain sort of tuples
    score = ((x - lse[:, None]).astype(np.float32) + bsc[:, None]).astype(np.float32)
    assert (score[2] == np.float32(-1e9)).all()
    every = sorted(((-float(score[b, w]), b, -float(x[b, w]), w) for b in range(beam) for w in range(V)))
    sc_all, idx_all = ref_select(x, lse, bsc, beam, beam * V)
    assert idx_all[0].tolist() == [b * V + w for _, b, _, w in every]
    assert sc_all[0].tolist() == [-s for s, _, _, _ in every]
    # inside the collapsed row the order falls back to (logit descending, word ascending)
    assert idx_all[0, -V:].tolist() == [2 * V + w for w in range(V)]
    # two sentences are ranked independently
    sc2, idx2 = ref_select(np.concatenate([x, x[::-1]]), np.concatenate([lse, lse[::-1]]), np.concatenate([bsc, bsc]), beam, 2)
    # (the second: beam 0 is the row 9, 8, ... - its 9 leads, its 8 already scores below the 3.0 of beam 1)
    assert idx2[0].tolist() == [1, 2] and idx2[1].tolist() == [0, V + 1]


# 4 sentences x beam 3; rows of a sentence are consecutive.  Sentence 3 is "done" from step 6 on: the search loop hands it
# all-zero entries.  Repeats (a beam that survives twice), identity steps and permutations are all there.
_BEAM_IDX = [
    [0, 0, 0, 3, 3, 3, 6, 6, 6, 9, 9, 9],             # the first step: every beam continues beam 0
    [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11],           # identity
    [1, 0, 0, 5, 5, 4, 8, 7, 6, 10, 10, 9],
    [2, 2, 1, 3, 4, 5, 6, 6, 6, 11, 9, 10],
    [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11],           # identity
    [2, 1, 0, 4, 3, 3, 7, 7, 8, 9, 9, 11],
    [1, 1, 1, 5, 4, 3, 6, 8, 7, 0, 0, 0],             # sentence 3 done
    [0, 2, 1, 3, 3, 3, 8, 8, 6, 0, 0, 0],
    [0, 0, 2, 4, 5, 3, 6, 7, 8, 0, 0, 0],
    [0, 1, 2, 3, 4, 5, 6, 7, 8, 0, 0, 0],             # identity for the live sentences
    [2, 0, 1, 5, 5, 5, 7, 6, 6, 0, 0, 0],
    [1, 2, 2, 3, 5, 4, 8, 6, 7, 0, 0, 0],
    [0, 0, 1, 4, 4, 3, 6, 6, 7, 0, 0, 0],
]


def test_advance_owner_keeps_the_reordered_cache():
    """A cache gathered through the owner table is, at every step, the cache index_select keeps."""
    from m3p_amd.decoder import advance_owner
    n, cap = 12, 16
    assert len(_BEAM_IDX) >= 12 and len(_BEAM_IDX) + 1 <= cap
    moved = torch.zeros((n, cap), dtype=torch.long)                 # re-ordered after every step, as the torch path does
    fixed = torch.zeros((n, cap), dtype=torch.long)                 # never re-ordered
    owner = torch.arange(n, dtype=torch.int32)[:, None].expand(n, cap).contiguous()
    cols = torch.arange(cap)[None, :].expand(n, cap)
    for step, bi in enumerate(_BEAM_IDX):
        tag = 1000 * (step + 1) + torch.arange(n)                   # what the step writes: position `step` of every row
        moved[:, step] = tag
        fixed[:, step] = tag
        got = fixed[owner.long(), cols]
        assert torch.equal(got[:, :step + 1], moved[:, :step + 1]), step
        beam_idx = torch.tensor(bi)
        moved = moved.index_select(0, beam_idx)
        new = advance_owner(owner, beam_idx, step + 1)
        assert new.dtype == torch.int32 and new.shape == owner.shape and new.data_ptr() != owner.data_ptr()
        owner = new
        assert torch.equal(fixed[owner.long(), cols][:, :step + 1], moved[:, :step + 1]), step
        assert owner[:, step + 1].tolist() == list(range(n))


# ------------------------------------------------------------------------------------------------------------------ GPU
def _logits(n, V, ld, seed, amp=16.0):
    """bf16 [n, ld] on the device, |x| <= amp in the V real columns, NaN / +inf alternating behind them; and the fp32 values."""
    g = torch.Generator().manual_seed(seed)
    x = ((torch.rand((n, V), generator=g) * 2 - 1) * amp).to(BF16)
    full = torch.empty((n, ld), dtype=BF16)
    full[:, :V] = x
    full[:, V::2] = float('nan')
    full[:, V + 1::2] = float('inf')
    return full, x


def _check(full, V, beam_scores, beam, k, what):
    """Run the kernels on `full` (CPU bf16 [n, ld]) and hold them to the contract.  -> (scores, flat_idx) as numpy."""
    from m3p_amd import ops
    n = full.shape[0]
    dev = full.cuda()
    bsc = None if beam_scores is None else torch.as_tensor(beam_scores, dtype=torch.float32).cuda()
    with poisoned_outputs():
        res = ops.vocab_select(dev, V, bsc, beam, k)
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
    return scores.cpu().numpy(), got_i


def _beam_scores(n, seed):
    return -np.random.RandomState(seed).uniform(0, 5, size=n).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize('V,ld,bs,beam,k', [
    (1000, 1024, 3, 2, 4),                          # one partial chunk
    (2 * CHUNK + 2, 8448, 2, 3, 6),                 # whole chunks plus two extra columns
    (1000, 1024, 1, 1, 1),                          # a single row
    (1000, 1024, 2, 8, 16),                         # the widest beam
    (250002, 250112, 2, 4, 8),                      # the full vocabulary width
    (2059, 2304, 2, 3, 6),                          # a chunk's second half: one whole load, a 3-column tail, the rest past V
])
def test_vocab_select_shapes(V, ld, bs, beam, k):
    assert ld % 256 == 0 and V <= ld < V + 256
    n = bs * beam
    full, _ = _logits(n, V, ld, seed=V + n)
    _check(full, V, _beam_scores(n, 7), beam, k, 'V %d bs %d beam %d k %d' % (V, bs, beam, k))


@pytest.mark.gpu
def test_vocab_select_planted_cases():
    """Maxima at the ends of the row and at a chunk boundary, equal maxima across chunks, identical rows, a row at -1e9."""
    V, ld, bs, beam, k = 2 * CHUNK + 2, 8448, 3, 3, 6
    n = bs * beam
    full, _ = _logits(n, V, ld, seed=11, amp=8.0)
    top = 12.0
    full[0, 0] = top                                    # sentence 0: the maximum in column 0,
    full[1, V - 1] = top                                # in column V - 1,
    full[2, 2 * CHUNK] = top                            # in the first column of the last chunk
    for w in (5, CHUNK + 7, V - 1):                     # sentence 1, beam 0: three equal maxima in three chunks
        full[3, w] = top
    full[6, 100], full[6, CHUNK + 904] = 11.0, 10.5      # sentence 2: beams 0 and 1 identical, with equal beam scores
    full[7] = full[6]
    bsc = np.array([0.0, 0.0, 0.0, -0.25, -0.5, -1e9, -1.0, -1.0, -3.0], dtype=np.float32)
    _, idx = _check(full, V, bsc, beam, k, 'planted')
    assert {0, 1 * V + V - 1, 2 * V + 2 * CHUNK} <= set(idx[0].tolist())
    assert idx[1, :3].tolist() == [5, CHUNK + 7, V - 1]                     # equal scores of one beam: by word
    assert (idx[1] // V != 2).all()                                         # the row at -1e9 is never chosen
    got = idx[2].tolist()                                                   # equal entries: the lower beam first
    assert got[:4] == [100, V + 100, CHUNK + 904, V + CHUNK + 904]
    assert all(i - V in got[:j] for j, i in enumerate(got) if i // V == 1) and all(i // V < 2 for i in got)
    # every row at -1e9 but one finite: the finite row supplies all k entries
    _, idx = _check(full, V, np.array([-1e9, -2.0, -1e9] * 3, dtype=np.float32), beam, k, 'planted, one finite beam')
    assert (idx // V == 1).all()
    # beam_scores = None is zeros
    _check(full, V, None, beam, k, 'planted, no beam scores')
    _check(full, V, None, 1, 1, 'planted, greedy')


@pytest.mark.gpu
def test_vocab_select_declines_more_than_max_k():
    from m3p_amd import ops
    max_k = ops.vocab_select_max_k()
    assert max_k >= 16
    full, _ = _logits(2, 1000, 1024, seed=3)
    dev = full.cuda()
    assert ops.vocab_select(dev, 1000, None, 1, max_k + 1) is None
    assert not ops.vocab_select_takes(2, 1000, 1024, 1, max_k + 1) and ops.vocab_select_takes(2, 1000, 1024, 1, max_k)
    assert ops.vocab_select(dev, 1000, None, 1, max_k) is not None
