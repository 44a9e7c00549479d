"""Beam search beyond 8 beams (csrc/select.hip: m3p_vocab_select_wide; ops.vocab_select_wide) - the part that needs no GPU.

The plan of the wide entry, and the two-phase argument the kernels rest on, in NumPy: inside one row the score
fl32(fl32(x - lse) + beam_score) is a monotone (non-decreasing) function of the logit x, so the total order T of
tests/test_vocab_select.py restricted to a row is (logit descending, word ascending) whatever lse and the beam score are.
A sentence's first k entries under T therefore lie in the union of every row's first k entries under (logit descending,
word ascending) - phase 1, the count selection of m3p_vocab_sample_wide - and T over that union (phase 2, one sort of
beam * k entries) returns what T over all beam * V entries returns."""
import numpy as np
import pytest
import torch

from tests.test_vocab_select import _lse32, ref_select

BF16 = torch.bfloat16


# ------------------------------------------------------------------------------------------------------------ the plan
def test_wide_plan_takes_the_wide_beams():
    from m3p_amd import ops
    assert ops.vocab_select_wide_max_k() == 64
    V, ld = 1000, 1024
    for beam in (9, 32):
        for k in (17, 18, 64):
            assert ops.vocab_select_wide_takes(3 * beam, V, ld, beam, k) is True, (beam, k)
    assert ops.vocab_select_wide_takes(1, V, ld, 1, 1) is True and ops.vocab_select_wide_takes(16, V, ld, 8, 16) is True
    assert ops.vocab_select_wide_takes(10, 250002, 250112, 10, 20) is True


def test_wide_plan_declines_beyond_its_bounds():
    from m3p_amd import ops
    V, ld = 1000, 1024
    assert ops.vocab_select_wide_takes(18, V, ld, 9, 65) is False
    assert ops.vocab_select_wide_takes(66, V, ld, 33, 64) is False
    assert ops.vocab_select_wide_takes(66, V, ld, 33, 66) is False
    # 32-bit block and candidate indices: n * chunks * 16 >= 2^31
    assert ops.vocab_select_wide_takes(32 * 70000, 250002, 250112, 32, 64) is False


def test_wide_plan_raises_on_malformed_shapes():
    from m3p_amd import lib as L
    from m3p_amd import ops
    V, ld = 1000, 1024
    for shape in ((19, V, ld, 9, 18),               # n % beam != 0
                  (18, V, 992, 9, 18),              # ld < V
                  (18, 40, 40, 9, 41),              # k > V: a row supplies at most V entries to its own first k
                  (18, 40, 40, 9, 65),              # ... which is malformed before it is too wide
                  (18, V, 1028, 9, 18),             # ld % 8 != 0
                  (18, V, ld, 9, 0), (0, V, ld, 9, 18)):
        with pytest.raises(L.M3PError):
            ops.vocab_select_wide_takes(*shape)


def test_the_narrow_plan_is_unchanged():
    from m3p_amd import ops
    assert ops.vocab_select_max_k() == 16
    assert ops.vocab_select_takes(18, 1000, 1024, 9, 17) is False
    assert ops.vocab_select_takes(2, 1000, 1024, 1, 17) is False
    assert ops.vocab_select_takes(16, 1000, 1024, 8, 16) is True


def test_the_workspace_holds_both_phases():
    from m3p_amd import lib as L
    lib = L.load()
    n, V, beam, k = 18, 8194, 9, 18
    need = lib.m3p_vocab_select_wide_workspace_bytes(n, V, beam, k)
    chunks = 3
    # the count selection's workspace, then the chunks' (max, sum) and one candidate per chunk
    assert need >= lib.m3p_vocab_sample_wide_workspace_bytes(n, V, k) + n * chunks * 12
    assert lib.m3p_vocab_select_wide_workspace_bytes(0, V, beam, k) == 0


def test_the_decoder_dispatch_constants():
    from m3p_amd import decoder
    assert decoder.BEAM_SELECT_WIDE_MIN_K == 17 == decoder.VOCAB_SELECT_MAX_K + 1
    assert decoder.BEAM_SELECT_WIDE_MAX_K in range(0, 65)


# ------------------------------------------------------------------------------------------------ the two-phase argument
def two_phase_select(logits, lse, beam_scores, beam, k):
    """ref_select by the kernels' route: each row's first k words under (logit descending, word ascending) by a stable sort,
    then T over those beam * k entries alone."""
    logits = np.asarray(logits, dtype=np.float32)
    n, V = logits.shape
    assert k <= V
    bs = n // beam
    lse = np.asarray(lse, np.float32)
    bsc = np.asarray(beam_scores, np.float32)
    keep = np.stack([np.argsort(-logits[r], kind='stable')[:k] for r in range(n)])           # [n, k] words
    out_s, out_i = np.empty((bs, k), np.float32), np.empty((bs, k), np.int64)
    for s in range(bs):
        rows = np.arange(s * beam, (s + 1) * beam)
        word = keep[rows].reshape(-1)
        beam_id = np.repeat(np.arange(beam), k)
        lg = logits[rows[:, None], keep[rows]].reshape(-1)
        sc = (lg - np.repeat(lse[rows], k)).astype(np.float32)
        sc = (sc + np.repeat(bsc[rows], k)).astype(np.float32)
        order = np.lexsort((word, -lg, beam_id, -sc))[:k]
        out_s[s], out_i[s] = sc[order], beam_id[order] * V + word[order]
    return out_s, out_i


def _rows(n, V, seed, amp=16.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand((n, V), generator=g) * 2 - 1) * amp).to(BF16).float().numpy()


def _same(x, bsc, beam, k):
    lse = _lse32(x)
    exp_s, exp_i = ref_select(x, lse, bsc, beam, k)
    got_s, got_i = two_phase_select(x, lse, bsc, beam, k)
    assert np.array_equal(got_i, exp_i)
    assert np.array_equal(got_s.view(np.uint32), exp_s.view(np.uint32))
    return exp_i


def test_two_phases_equal_the_full_order_on_random_rows():
    V, beam, k, bs = 1000, 9, 18, 3
    x = _rows(bs * beam, V, seed=5)
    bsc = -np.random.RandomState(7).uniform(0, 5, size=bs * beam).astype(np.float32)
    idx = _same(x, bsc, beam, k)
    assert len(set((idx[0] // V).tolist())) > 1                  # more than one beam supplies entries


def test_two_phases_equal_the_full_order_with_a_class_across_the_kth_place():
    V, beam, k, bs = 1000, 9, 18, 2
    x = _rows(bs * beam, V, seed=6, amp=4.0)
    for r in range(bs * beam):                                   # 5 above, then a class of 30 equal logits: places 6 .. 35
        x[r, 800 + 10 * r:800 + 10 * r + 5] = 9.0
        x[r, 100 + r:700 + r:20] = 6.0
    assert ((x == 6.0).sum(1) == 30).all()
    bsc = np.zeros(bs * beam, np.float32)
    bsc[1::2] = -0.5
    idx = _same(x, bsc, beam, k)
    # of a row's class only its lowest words enter (13 of 30 fit behind the 5 above)
    for s in range(bs):
        for i in idx[s]:
            b, w = divmod(int(i), V)
            r = s * beam + b
            assert x[r, w] == 9.0 or w in (100 + r + 20 * np.arange(13))


def test_two_phases_equal_the_full_order_at_the_first_step():
    V, beam, k, bs = 1000, 9, 18, 2
    x = _rows(bs * beam, V, seed=8)
    bsc = np.full(bs * beam, -1e9, np.float32)
    bsc[::beam] = 0.0
    idx = _same(x, bsc, beam, k)
    assert (idx // V == 0).all()                                 # all k come from beam 0
