"""m3p_ema_update and m3p_ema_swap (csrc/optim.hip; the contract in include/m3p_hip.h) on buffers with sentinel elements in
front of, between and behind the pieces: the update against the NumPy twin of tests/test_ema_cpu.py to the bit, the guard's
skip word, the refusals, and the swap with its bf16 copy.

Shapes: the launcher deals at most EMA_MAXBLK blocks of 256 threads, and a thread takes EMA_Q quads per trip of its loop.  Up
to EMA_MAXBLK * 256 quads every thread has one quad and the second slot of a trip stays empty; beyond, the second slot fills;
beyond EMA_Q * EMA_MAXBLK * 256 quads the loop takes a second trip.  The cases stand on both sides of both borders."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_ema_cpu import ema_twin, w_of
from tests.util import assert_bits_equal

pytestmark = pytest.mark.gpu

EMA_Q, EMA_MAXBLK, THREADS, EMA_MAX_RANGES = 2, 4096, 256, 32      # csrc/optim.hip
ONE_SLOT = EMA_MAXBLK * THREADS * 4                                  # elements up to which a thread has at most one quad
ONE_TRIP = EMA_Q * ONE_SLOT                                          # elements up to which the loop takes one trip
POISON = -0x01010101                                                 # the bits 0xFEFEFEFF of every sentinel element (-1.7e38 as fp32)


def _spread(sizes, gap=4, first=4):
    out, pos = [], first
    for n in sizes:
        out.append((pos, pos + n))
        pos += n + gap
    return out


CASES = {
    'one_quad': _spread([4], first=8),
    'quads_255_and_257': _spread([4 * 255, 4 * 257]),
    'second_slot_begins': _spread([ONE_SLOT + 12]),
    'second_trip_begins': _spread([ONE_TRIP + 4]),
    'thirty_three_pieces': _spread([4 * (1 + (7 * k) % 19) for k in range(EMA_MAX_RANGES + 1)], gap=8),
    'zero_length_pieces': [(4, 4), (8, 40), (44, 44), (48, 52), (60, 60), (64, 64 + 4 * 300), (2000, 2000)],
    'quad_aligned_not_64_aligned': [(4, 200), (212, 1000), (1004, 1004 + 4 * 513)],
}


def _buffers(pieces, seed, with_w16=False):
    """p, ema (and w16) long enough for the pieces plus a sentinel tail; the pieces hold random values of mixed magnitude,
    every other element the poison pattern."""
    n = max(b for _, b in pieces) + 8
    rs = np.random.RandomState(seed)
    p = np.full(n, POISON, dtype=np.int32).view(np.float32)
    e = p.copy()
    for a, b in pieces:
        e[a:b] = (rs.standard_normal(b - a) * np.exp(rs.uniform(-8, 4, b - a))).astype(np.float32)
        p[a:b] = (e[a:b] * (1 + 0.01 * rs.standard_normal(b - a)) + 1e-4 * rs.standard_normal(b - a)).astype(np.float32)
    out = [torch.from_numpy(p).cuda(), torch.from_numpy(e).cuda()]
    if with_w16:
        out.append(torch.full((n,), -258, dtype=torch.int16, device='cuda').view(torch.bfloat16))      # 0xFEFE everywhere
    return out, p, e


def _outside(n, pieces):
    keep = torch.ones(n, dtype=torch.bool)
    for a, b in pieces:
        keep[a:b] = False
    return keep.cuda()


def _raw(fn, p_ptr, e_ptr, w16_ptr, pieces, w=None, skip_ptr=None):
    """The C entry points with the pieces exactly as given (start, count) - no wrapper in between.  -> return code."""
    from m3p_amd import lib as L
    n = len(pieces)
    starts = (C.c_longlong * max(n, 1))(*[a for a, _ in pieces])
    counts = (C.c_longlong * max(n, 1))(*[c for _, c in pieces])
    if fn == 'update':
        return L.load().m3p_ema_update(p_ptr, e_ptr, starts, counts, n, w, skip_ptr, L.stream())
    return L.load().m3p_ema_swap(p_ptr, e_ptr, w16_ptr, starts, counts, n, L.stream())


# ---- 6. the update against the twin ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('decay', [0.9, 0.9999])
@pytest.mark.parametrize('case', sorted(CASES))
def test_update_equals_the_twin_to_the_bit(case, decay):
    """Bit for bit, against the twin WITH contraction.  Decided by reading the ISA of ema_update_kernel (both instantiations) as
    the Makefile builds it (hipcc --cuda-device-only -S with its flags; --save-temps compiles the device code another way
    and shows another answer): per quad v_sub_f32 x 4, then v_pk_fma_f32 x 2, no separate product - the source asks for the
    fused multiply-add by name (__builtin_fmaf), since -ffp-contract=fast fuses a separate product and sum whatever a
    pragma says.  fp32 denormals are kept (float_denorm_mode_32 = 3), as NumPy keeps them."""
    from m3p_amd import ops
    pieces = CASES[case]
    (p, ema), p0, e0 = _buffers(pieces, seed=len(case))
    w = w_of(decay)
    ops.ema_update(p, ema, pieces, float(w))
    torch.cuda.synchronize()
    want = e0.copy()
    for a, b in pieces:
        want[a:b] = ema_twin(e0[a:b], p0[a:b], w, contract=True)
    assert_bits_equal(ema, torch.from_numpy(want), 'ema after the update, %s (sentinels included)' % case)
    assert_bits_equal(p, torch.from_numpy(p0), 'p after the update, %s' % case)
    loose = sum(int((want[a:b].view(np.int32) != ema_twin(e0[a:b], p0[a:b], w).view(np.int32)).sum()) for a, b in pieces)
    print('%s, decay %g: %d elements where three roundings would differ from the fused form' % (case, decay, loose))
    moved = sum(int((want[a:b].view(np.int32) != e0[a:b].view(np.int32)).sum()) for a, b in pieces)
    assert moved > 0.5 * sum(b - a for a, b in pieces), 'the case moves the EMA'


# ---- 7. the skip word -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['quads_255_and_257', 'thirty_three_pieces', 'second_slot_begins'])
def test_skip_word(case):
    from m3p_amd import ops
    pieces = CASES[case]
    (p, ema), p0, e0 = _buffers(pieces, seed=5)
    w = float(w_of(0.99))
    skip = torch.ones(1, dtype=torch.int32, device='cuda')
    ops.ema_update(p, ema, pieces, w, skip=skip)
    torch.cuda.synchronize()
    assert_bits_equal(ema, torch.from_numpy(e0), 'ema after a skipped update')
    assert_bits_equal(p, torch.from_numpy(p0), 'p after a skipped update')
    assert int(skip) == 1
    skip.zero_()
    ops.ema_update(p, ema, pieces, w, skip=skip)
    plain = torch.from_numpy(e0).cuda()
    ops.ema_update(p, plain, pieces, w)
    torch.cuda.synchronize()
    assert_bits_equal(ema, plain, 'guarded update with the word at 0 against the unguarded one')
    assert not torch.equal(ema.view(torch.int32), torch.from_numpy(e0).cuda().view(torch.int32))


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------
BAD = {
    'start_not_a_multiple_of_4': dict(pieces=[(8, 16), (30, 8)]),
    'count_not_a_multiple_of_4': dict(pieces=[(8, 16), (32, 6)]),
    'negative_count': dict(pieces=[(8, 16), (32, -4)]),
    'negative_start': dict(pieces=[(-4, 8)]),
    'null_p': dict(pieces=[(8, 16)], p=None),
    'null_ema': dict(pieces=[(8, 16)], ema=None),
    'misaligned_p': dict(pieces=[(8, 16)], p=4),
    'misaligned_ema': dict(pieces=[(8, 16)], ema=8),
    'no_pieces': dict(pieces=[]),
}


@pytest.mark.parametrize('fn', ['update', 'swap'])
@pytest.mark.parametrize('bad', sorted(BAD))
def test_refusals_change_nothing(bad, fn):
    """M3P_EINVAL (-1) before any launch: the valid first piece of a list with a bad second one stays as it was, too."""
    spec = BAD[bad]
    rs = np.random.RandomState(1)
    p0, e0 = rs.standard_normal(64).astype(np.float32), rs.standard_normal(64).astype(np.float32)
    p, ema = torch.from_numpy(p0).cuda(), torch.from_numpy(e0).cuda()
    w16 = torch.full((64,), 3.0, dtype=torch.bfloat16, device='cuda')
    ptr = lambda t, key: None if (key in spec and spec[key] is None) else t.data_ptr() + spec.get(key, 0)      # noqa: E731
    rc = _raw(fn, ptr(p, 'p'), ptr(ema, 'ema'), w16.data_ptr(), spec['pieces'], w=0.5)
    torch.cuda.synchronize()
    assert rc == -1, '%s, %s: expected M3P_EINVAL, got %d' % (fn, bad, rc)
    assert_bits_equal(p, torch.from_numpy(p0), 'p after the refused call')
    assert_bits_equal(ema, torch.from_numpy(e0), 'ema after the refused call')
    assert bool((w16 == 3.0).all())


def test_misaligned_skip_and_w16_are_refused():
    p, ema = torch.zeros(64, device='cuda'), torch.ones(64, device='cuda')
    w16 = torch.zeros(64, dtype=torch.bfloat16, device='cuda')
    word = torch.zeros(2, dtype=torch.int32, device='cuda')
    assert _raw('update', p.data_ptr(), ema.data_ptr(), None, [(8, 16)], w=0.5, skip_ptr=word.data_ptr() + 2) == -1
    assert _raw('swap', p.data_ptr(), ema.data_ptr(), w16.data_ptr() + 2, [(8, 16)]) == -1
    torch.cuda.synchronize()
    assert bool((ema == 1).all()) and bool((p == 0).all())


# ---- 9. the swap ------------------------------------------------------------------------------------------------------------------
SPECIAL = np.array([
    0x3F7FFFFF, 0x3F7F8000, 0x3F7F7FFF, 0x3F808000, 0x3F818000, 0x3F80FFFF,      # rounds up into the next exponent; ties to even both ways
    0x7F7FFFFF, 0xFF7FFFFF,                                                      # the largest finite values: round to +-inf
    0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x007FFFFF, 0x807FFFFF, 0x80000001, 0x00018000,      # denormals
    0x00000000, 0x80000000, 0x7F800000, 0xFF800000,                              # +-0, +-inf
    0x7FC00000, 0x7FC12345, 0xFFC00000, 0x7F812345, 0xFFFFFFFF, 0x7F800001,      # NaNs: quiet, with payload, negative, signalling
    0x3F800000, 0xBF800000, 0x40490FDB, 0x00800000,
], dtype=np.uint32).view(np.float32)


def _assert_bf16_of(w16, x, what):
    """w16 = bf16(x) to the bit.  Every lane that is not a NaN - finite values, denormals, signed zeros, infinities - against
    torch's own conversion of the same tensor on the device.  A NaN lane against the rule of the conversion instruction behind
    Vec4<bf16>::store (v_cvt_pk_bf16_f32): sign and the upper payload bits pass through and the quiet bit is set, bits >> 16 |
    0x0040.  torch's conversion cannot be the reference there: it replaces every NaN by 0x7FC0, sign and payload lost."""
    nan = torch.isnan(x)
    assert_bits_equal(w16[~nan], x[~nan].to(torch.bfloat16), what + ' (lanes that are not NaN)')
    want = ((x[nan].view(torch.int32) >> 16) | 0x40).to(torch.int16)
    assert_bits_equal(w16[nan].view(torch.int16), want, what + ' (NaN lanes: sign and payload passed through, quieted)')
    assert bool(torch.isnan(w16[nan].float()).all())


@pytest.mark.parametrize('case', sorted(CASES))
def test_swap_exchanges_and_rounds(case):
    """p and ema trade places to the bit (NaN payloads, infinities, denormals and signed zeros pass through), w16 is the bf16
    rounding of the new p (`_assert_bf16_of`), and a second swap restores all three."""
    from m3p_amd import ops
    pieces = CASES[case]
    (p, ema, w16), p0, e0 = _buffers(pieces, seed=11, with_w16=True)
    # the special values into the EMA side (it becomes the new p, which w16 follows) of every piece that holds them, and a few
    # into p
    for a, b in pieces:
        k = min(b - a, SPECIAL.size)
        e0[a:a + k] = SPECIAL[:k]
        p0[b - k:b] = SPECIAL[:k][::-1]
    p.copy_(torch.from_numpy(p0)); ema.copy_(torch.from_numpy(e0))
    w0 = w16.clone()
    ops.ema_swap(p, ema, w16, pieces)
    torch.cuda.synchronize()
    want_p, want_e = p0.copy(), e0.copy()
    for a, b in pieces:
        want_p[a:b], want_e[a:b] = e0[a:b], p0[a:b]
    assert_bits_equal(p, torch.from_numpy(want_p), 'p after the swap, %s' % case)
    assert_bits_equal(ema, torch.from_numpy(want_e), 'ema after the swap, %s' % case)
    outside = _outside(p.numel(), pieces)
    assert_bits_equal(w16[outside], w0[outside], 'w16 outside the pieces, %s' % case)
    inside = ~outside
    _assert_bf16_of(w16[inside], p[inside], 'w16 against bf16(new p), %s' % case)
    first = w16.clone()
    ops.ema_swap(p, ema, w16, pieces)
    torch.cuda.synchronize()
    assert_bits_equal(p, torch.from_numpy(p0), 'p after the second swap')
    assert_bits_equal(ema, torch.from_numpy(e0), 'ema after the second swap')
    _assert_bf16_of(w16[inside], p[inside], 'w16 after the second swap')
    assert_bits_equal(w16[outside], w0[outside], 'w16 outside the pieces after the second swap')
    ops.ema_swap(p, ema, w16, pieces)
    torch.cuda.synchronize()
    assert_bits_equal(w16, first, 'w16 after the third swap against the first')


def test_swap_rounds_to_nearest_even_by_the_book():
    """The same conversion against round-to-nearest-even written out on the bits (finite values and infinities)."""
    from m3p_amd import ops
    vals = SPECIAL[~np.isnan(SPECIAL)]
    vals = np.concatenate([vals, np.zeros((-vals.size) % 4, dtype=np.float32)])
    ema = torch.from_numpy(vals.copy()).cuda()
    p = torch.zeros_like(ema)
    w16 = torch.zeros(vals.size, dtype=torch.bfloat16, device='cuda')
    ops.ema_swap(p, ema, w16, [(0, vals.size)])
    torch.cuda.synchronize()
    u = vals.view(np.uint32).astype(np.uint64)
    rne = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    assert np.array_equal(w16.view(torch.int16).cpu().numpy().view(np.uint16), rne)


def test_swap_without_a_bf16_copy():
    from m3p_amd import ops
    pieces = CASES['quads_255_and_257']
    (p, ema), p0, e0 = _buffers(pieces, seed=2)
    ops.ema_swap(p, ema, None, pieces)
    torch.cuda.synchronize()
    want_p, want_e = p0.copy(), e0.copy()
    for a, b in pieces:
        want_p[a:b], want_e[a:b] = e0[a:b], p0[a:b]
    assert_bits_equal(p, torch.from_numpy(want_p), 'p')
    assert_bits_equal(ema, torch.from_numpy(want_e), 'ema')
