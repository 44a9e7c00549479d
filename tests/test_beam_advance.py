"""ops.beam_advance (csrc/beam.hip: the hypothesis bookkeeping of a beam-search step on the device) against its host twin
decoder.beam_advance_host, on the candidate streams of tests/test_beam_advance_cpu.py - which holds the twin to the loop over
decoder.BeamHypotheses.  The streams run step by step through both; after EVERY step every output (beam_scores, beam_words,
beam_idx, the re-ordered `generated`, the owner table of decoder.advance_owner) and every state tensor must be equal, scores as
bits (fp32 and fp64).  Beyond the CPU file's shapes: beam 32 (k = 64, the widest the kernel takes) and max_len 70 with the
first <EOS> at step 66, so that the token copy and the re-ordering stride more than one pass of the wave's 64 lanes."""
import numpy as np
import pytest
import torch

from m3p_amd import decoder
from tests.test_beam_advance_cpu import EOS, PAD, Case, Twin, drive, hand_made_cases, random_cases

BITS = {'hyp_score': np.int64, 'hyp_sum': np.int32}


class Device:
    """ops.beam_advance with its state, the two `generated` buffers and the two owner tables on the GPU."""

    def __init__(self, c):
        from m3p_amd import ops
        self.c, self.ops = c, ops
        n = c.bs * c.beam
        self.state = ops.beam_state(c.bs, c.beam, c.max_len, PAD, 'cuda')
        norm, self.norm_max = decoder.beam_norms(c.max_len, c.lp)
        self.norm = torch.from_numpy(norm).cuda()
        self.gen = torch.full((c.max_len, n), PAD, dtype=torch.long, device='cuda')
        self.gen[0] = EOS
        self.gen_spare = self.gen.clone()
        self.owner = torch.arange(n, dtype=torch.int32, device='cuda')[:, None].expand(n, c.max_len).contiguous()
        self.owner_spare = self.owner.clone()

    def step(self, next_scores, next_words, generated, cur_len):
        c = self.c
        assert np.array_equal(self.gen.cpu().numpy(), generated), 'the device did not start the step from the host\'s tokens'
        res = self.ops.beam_advance(torch.from_numpy(next_scores).cuda(), torch.from_numpy(next_words).cuda(), self.gen,
                                    self.gen_spare, self.owner, self.owner_spare, self.state, cur_len, c.max_len, EOS, PAD, c.V,
                                    c.beam, c.es, self.norm, self.norm_max)
        assert res is not None
        self.gen, self.gen_spare = self.gen_spare, self.gen
        self.owner, self.owner_spare = self.owner_spare, self.owner
        return tuple(t.cpu().numpy() for t in res)

    def host_state(self):
        return {k: v.cpu().numpy() for k, v in self.state.items()}

    def lists(self):
        from tests.test_beam_advance_cpu import state_lists
        return state_lists(self.host_state())

    def dones(self):
        return [bool(d) for d in self.state['done'].cpu().tolist()]


def _against_the_twin(c):
    twin, dev = Twin(c), Device(c)
    n = c.bs * c.beam
    owner = [np.tile(np.arange(n, dtype=np.int32)[:, None], (1, c.max_len))]

    def after_step(cur_len, sc, idx, generated, nxt, out):
        where = (c.name, 'step', cur_len)
        assert np.array_equal(dev.gen.cpu().numpy(), nxt), where + ('generated',)
        new = owner[0][out[2]]                                      # decoder.advance_owner
        new[:, cur_len] = np.arange(n, dtype=np.int32)
        owner[0] = new
        assert np.array_equal(dev.owner.cpu().numpy(), new), where + ('owner',)
        got = dev.host_state()
        for name in decoder.HYP_STATE:
            a, b = twin.state[name], got[name]
            assert a.dtype == b.dtype and a.shape == b.shape, where + (name,)
            if name in BITS:
                a, b = a.view(BITS[name]), b.view(BITS[name])
            assert np.array_equal(a, b), where + (name,)
    steps = drive(c, twin, dev, after_step)
    torch.cuda.synchronize()
    return steps, twin


WIDE = random_cases(beams=(32,))
LONG = [Case('long-beam%d-lp%g-es%d' % (beam, lp, es), beam, lp, es, max_len=70, seed=70 + beam,
             eos_ranks=lambda cur, s: [] if cur < 66 else None)
        for beam, lp, es in ((1, 1.0, False), (3, 0.6, True), (16, 2, False), (32, 0, False))]


@pytest.mark.gpu
@pytest.mark.parametrize('c', random_cases() + WIDE, ids=repr)
def test_random_streams_equal_the_twin(c):
    _, twin = _against_the_twin(c)
    assert not twin.state['status'].any()


@pytest.mark.gpu
@pytest.mark.parametrize('c', hand_made_cases(), ids=repr)
def test_hand_made_streams_equal_the_twin(c):
    _against_the_twin(c)


@pytest.mark.gpu
@pytest.mark.parametrize('c', LONG, ids=repr)
def test_long_streams_copy_more_than_one_pass_of_lanes(c):
    steps, twin = _against_the_twin(c)
    assert steps >= 66 and int(twin.state['hyp_len'].max()) > 64


@pytest.mark.gpu
def test_shapes_beyond_the_limits_are_declined():
    from m3p_amd import lib as L
    from m3p_amd import ops
    assert ops.beam_advance_takes(3, 32, 64, 1025)
    assert not ops.beam_advance_takes(3, 33, 66, 10)
    assert not ops.beam_advance_takes(3, 32, 65, 10)
    assert not ops.beam_advance_takes(3, 2, 4, 1026)
    with pytest.raises(L.M3PError):
        ops.beam_advance_takes(0, 2, 4, 10)
    # the op itself answers None and writes nothing
    c = Case('declined', 33, 1.0, False, bs=1, V=11, max_len=4)
    dev = Device(c)
    sc = torch.zeros((1, 66), dtype=torch.float32, device='cuda')
    idx = torch.arange(66, device='cuda')[None, :].contiguous()
    before = dev.host_state()
    assert dev.ops.beam_advance(sc, idx, dev.gen, dev.gen_spare, dev.owner, dev.owner_spare, dev.state, 1, c.max_len, EOS, PAD, c.V,
                                c.beam, c.es, dev.norm, dev.norm_max) is None
    after = dev.host_state()
    assert all(np.array_equal(before[k], after[k]) for k in before)


@pytest.mark.gpu
def test_too_few_continuations_set_status():
    """One beam's <EOS> twice - more <EOS> than a real selection gives - leaves one continuation for two beams."""
    c = Case('too-few', 2, 1.0, False, bs=1, V=11, max_len=6)
    twin, dev = Twin(c), Device(c)
    gen = np.full((c.max_len, 2), PAD, dtype=np.int64)
    gen[0] = EOS
    sc = np.array([[-1, -2, -3, -4]], dtype=np.float32)
    idx = np.array([[EOS, c.V + EOS, EOS, 5]], dtype=np.int64)
    a, b = twin.step(sc, idx, gen, 1), dev.step(sc, idx, gen, 1)
    assert twin.state['status'].tolist() == [1] and dev.state['status'].cpu().tolist() == [1]
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    got = dev.host_state()
    for name in decoder.HYP_STATE:
        assert np.array_equal(twin.state[name], got[name]), name
    from m3p_amd import lib as L
    with pytest.raises(L.M3PError):
        decoder._beam_result(got, 1, False, EOS, PAD, torch.device('cpu'))
