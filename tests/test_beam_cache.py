"""Beam search over caches that stay in place (m3p_amd/decoder.py, csrc/decode.hip: m3p_attn_query_owner_fwd) and the word
selection kernels inside the two search loops (csrc/select.hip).

- the owner kernel equals m3p_attn_query_fwd on the materialised gather bit for bit;
- decoder_forward over an in-place cache (cache['owner'] / cache['beam'], the source's keys / values once per sentence) equals
  decoder_forward over a cache re-ordered with index_select and a source expanded per beam, step by step;
- generate_beam and greedy generate on the select path meet the criteria tests/test_decoder.py applies against the
  reference's golden vectors, and give the tokens of the torch path (decoder.VOCAB_SELECT_MAX_K = 0)."""
import numpy as np
import pytest
import torch

from m3p_amd import synth
from tests.test_decoder import G, _agree_until_near_tie, _hip_model
from tests.util import poisoned_outputs

BF16 = torch.bfloat16
TAGS = list(synth.DECODER_CASES)
BEAM_TAGS = [t for t in TAGS if synth.DECODER_CASES[t]['beam_size']]


# ------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.gpu
@pytest.mark.parametrize('H,dh', [(4, 32), (4, 64), (12, 32), (12, 64)])
def test_owner_kernel_equals_the_plain_kernel_on_the_gather(H, dh):
    from m3p_amd import ops
    B, R, d = 6, 9, H * dh                         # R rows of keys / values for B query sequences
    g = torch.Generator(device='cuda').manual_seed(100 * H + dh)
    for Lk in (1, 9, 70, 1024):                    # below 64 lanes, above them, and QA_MAX_KEYS of csrc/decode.hip
        pool = torch.randn(R, Lk + 3, 2 * d, device='cuda', generator=g).to(BF16)
        per_key = torch.randint(0, R, (B, Lk + 2), device='cuda', generator=g).to(torch.int32)       # (row pitch != Lk)
        per_seq = torch.randint(0, R, (B,), device='cuda', generator=g).to(torch.int32)
        cols = torch.arange(Lk, device='cuda')[None, :].expand(B, Lk)
        gathers = ((per_key, pool[per_key[:, :Lk].long(), cols].contiguous()), (per_seq, pool[per_seq.long()].contiguous()))
        for Tq in (1, 3):
            q = torch.randn(B * Tq, d, device='cuda', generator=g).to(BF16)
            klen = torch.randint(1, Lk + 1, (B,), device='cuda', generator=g).to(torch.int32)
            klen[0], klen[1] = 1, Lk
            modes = [dict(klen=klen, causal=False, pos0=0)]
            if Tq <= Lk:
                modes.append(dict(klen=None, causal=True, pos0=Lk - Tq))
            for mode in modes:
                for owner, gathered in gathers:
                    with poisoned_outputs():
                        ref = ops.attn_query_fwd(q, gathered, mode['klen'], B, Tq, H, dh, Lk, causal=mode['causal'], pos0=mode['pos0'])
                        got = ops.attn_query_fwd(q, pool, mode['klen'], B, Tq, H, dh, Lk, causal=mode['causal'], pos0=mode['pos0'],
                                                 owner=owner)
                    assert not bool(torch.isnan(ref.float()).any())
                    assert torch.equal(got, ref), (H, dh, Lk, Tq, mode['causal'], owner.dim())


# ------------------------------------------------------------------------------------------------------ decoder_forward
def _beam_script(bs, beam, steps, done_sentence, done_from, seed):
    """beam_idx vectors as the search loop builds them: every row continues a row of its own sentence (repeats, identity
    steps and permutations); the sentence marked done gets zeros."""
    rs = np.random.RandomState(seed)
    out = []
    for t in range(steps):
        v = []
        for s in range(bs):
            if s == done_sentence and t >= done_from:
                v += [0] * beam
            elif t == 0:
                v += [s * beam] * beam                                 # the first step: only beam 0 is alive
            elif t % 4 == 1:
                v += [s * beam + b for b in range(beam)]               # identity
            else:
                v += [s * beam + int(b) for b in rs.randint(0, beam, size=beam)]
        out.append(v)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('tag', ['multi', 'wide'])
def test_decoder_forward_in_place_cache_equals_the_reordered_cache(tag):
    """Two caches through nine single-token steps under one scripted beam_idx sequence: one re-ordered with index_select over a
    source expanded per beam, one in place (owner table, the source once per sentence).  Hidden states of the live sentences
    must be torch.equal at every step.

    The projection of the source is where the two could part: the GEMM picks its kernel by the row count (M <= 128: the
    split-K skinny kernel, above it the 128 x 128 tile kernel), and 'wide' has bs * S = 60 rows against bs * beam * S = 240.
    Projected on 60 rows, 4 of 81920 cached elements per layer came out one bf16 ulp off the expanded run's and the hidden
    states parted at step 2 (176 of 2048 elements, max |diff| 0.0156); decoder_forward therefore projects on the expanded row
    count and keeps one copy per sentence.  The failure message counts the cached source elements that differ."""
    from m3p_amd import decoder
    m, c, sd, src_enc, src_len, _, _ = _hip_model(tag)
    bs, beam, steps, max_len = c['bs'], c['beam_size'], 9, 12
    n = bs * beam
    done_sentence = bs - 1
    script = _beam_script(bs, beam, steps, done_sentence, 5, seed=c['seed'])
    assert len(script) >= 8 and any(v != list(range(n)) for v in script)
    live = torch.tensor([r // beam != done_sentence for r in range(n)], device='cuda')
    rs = np.random.RandomState(c['seed'] + 5)
    words = torch.from_numpy(rs.randint(3, c['n_words'], size=(steps, n))).cuda()
    src_x = src_enc.unsqueeze(1).expand((bs, beam) + src_enc.shape[1:]).contiguous().view((n,) + src_enc.shape[1:])
    len_x = src_len.unsqueeze(1).expand(bs, beam).contiguous().view(-1)
    generated = torch.full((max_len, n), synth.PAD, dtype=torch.long, device='cuda')
    generated[0] = synth.EOS
    positions = torch.arange(max_len, device='cuda')[:, None].expand(max_len, n)
    langs = None if c['tgt_lang_id'] is None else torch.full((max_len, n), c['tgt_lang_id'], dtype=torch.long, device='cuda')
    moved = {'slen': 0, 'max_len': max_len}
    fixed = {'slen': 0, 'max_len': max_len, 'beam': beam,
             'owner': torch.arange(n, dtype=torch.int32, device='cuda')[:, None].expand(n, max_len).contiguous()}
    with torch.no_grad():
        for t, bi in enumerate(script):
            cur = t + 1
            lengths = torch.full((n,), cur, dtype=torch.long, device='cuda')
            lg = None if langs is None else langs[:cur]
            a = decoder.decoder_forward(m, generated[:cur], lengths, src_x, len_x, positions[:cur], lg, moved)
            b = decoder.decoder_forward(m, generated[:cur], lengths, src_enc, len_x, positions[:cur], lg, fixed)
            assert a.shape == b.shape == (1, n, c['emb_dim']) and moved['slen'] == fixed['slen'] == cur
            assert not bool(torch.isnan(a[0][live].float()).any())
            if not torch.equal(a[0][live], b[0][live]):
                diff = (a[0][live].float() - b[0][live].float()).abs()
                # where the inputs of the step already differ: the source keys / values of the two caches, layer by layer
                rows = live.nonzero().view(-1)
                kv_diff = [int((moved[('cross', i)][rows] != fixed[('cross', i)][rows // beam]).sum()) for i in range(c['n_dec_layers'])]
                assert False, ('%s step %d: %d of %d elements differ, max |diff| %.3g; elements of the projected source that differ '
                               'between the caches, per layer: %s of %d' % (tag, t, int((diff > 0).sum()), diff.numel(), float(diff.max()),
                                                                         kv_diff, moved[('cross', 0)][rows].numel()))
            beam_idx = torch.tensor(bi, dtype=torch.long, device='cuda')
            generated = generated[:, beam_idx]
            generated[cur] = words[t]
            for k in list(moved.keys()):
                if isinstance(k, tuple):
                    moved[k] = moved[k].index_select(0, beam_idx)
            fixed['owner'] = decoder.advance_owner(fixed['owner'], beam_idx, cur)
    # the in-place cache holds the source once per sentence
    assert fixed[('cross', 0)].shape[0] == bs and moved[('cross', 0)].shape[0] == n


# ---------------------------------------------------------------------------------------------------------- end to end
def _spy_beam_idx(monkeypatch):
    """Record every beam_idx the search loop hands to advance_owner."""
    from m3p_amd import decoder
    seen = []
    real = decoder.advance_owner

    def spy(owner, beam_idx, next_pos):
        seen.append(beam_idx.tolist())
        return real(owner, beam_idx, next_pos)
    monkeypatch.setattr(decoder, 'advance_owner', spy)
    return seen


@pytest.mark.gpu
@pytest.mark.parametrize('tag', BEAM_TAGS)
def test_generate_beam_select_path_vs_reference_and_torch_path(tag, monkeypatch):
    from m3p_amd import decoder
    m, c, sd, src_enc, src_len, _, _ = _hip_model(tag)
    assert 2 * c['beam_size'] <= decoder.VOCAB_SELECT_MAX_K
    seen = _spy_beam_idx(monkeypatch)
    n_equal = n_total = 0
    outs = {}
    for lp, es in ((1.0, False), (0.6, True)):
        with torch.no_grad():
            dec, tl = m.generate_beam(src_enc, src_len, c['tgt_lang_id'], c['beam_size'], lp, es, max_len=c['max_len'])
        outs[(lp, es)] = (dec.cpu(), tl.cpu())
        key = '%s.beam_lp%.1f_es%d' % (tag, lp, es)
        ref, ref_len = G[key], G[key + '_len']
        dec, tl = dec.cpu().numpy(), tl.cpu().numpy()
        assert dec.shape[1] == ref.shape[1] and ((dec == synth.EOS).sum(0) == 2).all() and (dec[0] == synth.EOS).all()
        for b in range(ref.shape[1]):
            n_total += 1
            n_equal += int(tl[b] == ref_len[b] and np.array_equal(dec[:tl[b], b], ref[:ref_len[b], b]))
    assert n_equal >= n_total - 1, (n_equal, n_total)
    assert seen, 'the select path did not run'
    # the torch path on the same inputs: the same tokens and lengths
    monkeypatch.setattr(decoder, 'VOCAB_SELECT_MAX_K', 0)
    n_seen = len(seen)
    for (lp, es), (dec, tl) in outs.items():
        with torch.no_grad():
            dec0, tl0 = m.generate_beam(src_enc, src_len, c['tgt_lang_id'], c['beam_size'], lp, es, max_len=c['max_len'])
        assert torch.equal(tl0.cpu(), tl) and torch.equal(dec0.cpu(), dec), (tag, lp, es, dec0.cpu().t().tolist(), dec.t().tolist())
    assert len(seen) == n_seen, 'VOCAB_SELECT_MAX_K = 0 must send the loop to the torch path'


@pytest.mark.gpu
def test_the_beam_fixtures_reorder_their_beams(monkeypatch):
    """Fixture sanity: some step of some case has a beam_idx that is not the identity - otherwise the in-place cache of the
    end-to-end test above is never exercised."""
    seen = _spy_beam_idx(monkeypatch)
    moved = {}
    for tag in BEAM_TAGS:
        m, c, sd, src_enc, src_len, _, _ = _hip_model(tag)
        del seen[:]
        with torch.no_grad():
            m.generate_beam(src_enc, src_len, c['tgt_lang_id'], c['beam_size'], 1.0, False, max_len=c['max_len'])
        n = c['bs'] * c['beam_size']
        # (the first step always maps every beam to beam 0, whose rows alone are alive: count the steps behind it)
        moved[tag] = sum(v != list(range(n)) for v in seen[1:])
    assert any(moved.values()), moved


@pytest.mark.gpu
@pytest.mark.parametrize('tag', TAGS)
def test_generate_greedy_select_path_vs_reference_and_torch_path(tag, monkeypatch):
    from m3p_amd import decoder, ops
    m, c, sd, src_enc, src_len, _, _ = _hip_model(tag)
    calls = []
    real, rule = ops.vocab_select, decoder.VOCAB_SELECT_MAX_K
    monkeypatch.setattr(ops, 'vocab_select', lambda *a, **kw: calls.append(a[3:]) or real(*a, **kw))
    with torch.no_grad():
        gen, gen_len = m.generate(src_enc, src_len, c['tgt_lang_id'], max_len=c['max_len'])
    assert calls and all(a == (1, 1) for a in calls)
    ref, ref_len, margins = G[tag + '.greedy'], G[tag + '.greedy_len'], G[tag + '.greedy_margin']
    g, gl = gen.cpu().numpy(), gen_len.cpu().numpy()
    assert g.shape[1] == ref.shape[1] and (g[0] == synth.EOS).all() and ((g == synth.EOS).sum(0) == 2).all()
    _agree_until_near_tie(g, ref, margins, tol=0.02)
    exact = [b for b in range(ref.shape[1]) if margins[:, b].min() >= 0.02]
    assert exact
    for b in exact:
        assert gl[b] == ref_len[b] and np.array_equal(g[:gl[b], b], ref[:ref_len[b], b])
    # the torch path: the same tokens and lengths
    monkeypatch.setattr(decoder, 'VOCAB_SELECT_MAX_K', 0)
    n_calls = len(calls)
    with torch.no_grad():
        gen0, gen_len0 = m.generate(src_enc, src_len, c['tgt_lang_id'], max_len=c['max_len'])
    assert len(calls) == n_calls
    assert torch.equal(gen_len0, gen_len) and torch.equal(gen0, gen), (tag, gen0.t().tolist(), gen.t().tolist())
    # sampling stays on the torch path and keeps its random stream
    monkeypatch.setattr(decoder, 'VOCAB_SELECT_MAX_K', rule)
    torch.manual_seed(5)
    with torch.no_grad():
        s1, l1 = m.generate(src_enc, src_len, c['tgt_lang_id'], max_len=c['max_len'], sample_temperature=0.7)
    monkeypatch.setattr(decoder, 'VOCAB_SELECT_MAX_K', 0)
    torch.manual_seed(5)
    with torch.no_grad():
        s2, l2 = m.generate(src_enc, src_len, c['tgt_lang_id'], max_len=c['max_len'], sample_temperature=0.7)
    assert len(calls) == n_calls and torch.equal(s1, s2) and torch.equal(l1, l2)
