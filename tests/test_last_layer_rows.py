"""The last encoder layer on the rows the heads read (functional.OutputRows).

With a row hint, EncoderFn runs everything after attention in the last layer - out_lin, LayerNorm 1, the FFN, LayerNorm 2
and their backward - on the gathered rows only.  Checked here: parity with the oracle at the bars of
tests/test_model_parity.py with the hint on; the hint changes nothing beyond the order of fp32 sums; ragged row sets; the
eligibility rule; the row-mapped dropout of the GEMM epilogue and of LayerNorm backward bit for bit; the fill-and-place
kernel; three trainer steps."""
import numpy as np
import pytest
import torch

from m3p_amd import synth
from tests.util import assert_bits_equal, encoder_keep_masks, poisoned_outputs, randn_bf16, randn_f32, rel_l2

BF16 = torch.bfloat16
gpu = pytest.mark.gpu

# the parity module's configurations and model builder ('tiles': two layers, M = 16 384, 256 * 17 = 4 352 selected rows;
# 'tiles768': one layer - the pruned layer also feeds the embedding backward -, M = 20 992, 128 * 33 = 4 224 -> 4 352)
COMPACT_CFGS = ['tiles', 'tiles768']


def _parity():
    import tests.test_model_parity as mp
    return mp


def _hint(cfg, batch):
    from m3p_amd import functional as Fn
    return Fn.OutputRows.from_masks(cfg['B'], cfg['T'] + cfg['R'], cfg['R'], pred_mask=batch['pred_mask'])


class _NtSpy:
    """Shapes and epilogues of every ops.gemm_nt launch."""

    def __init__(self, monkeypatch):
        from m3p_amd import ops
        self.shapes = []
        real = ops.gemm_nt

        def nt(a, w, epilogue=0, **kw):
            self.shapes.append((epilogue, a.shape[0], kw.get('n') or w.shape[0], a.shape[1]))
            return real(a, w, epilogue, **kw)
        monkeypatch.setattr(ops, 'gemm_nt', nt)

    def assert_compact(self, n, d, ran=True):
        from m3p_amd import lib as L
        for e in (L.EPI_BIAS_GELUQ, L.EPI_MULQ):
            assert ((e, n, 4 * d, d) in self.shapes) == ran, (e, n, sorted(set(self.shapes)))


def _step(cfg, batch, p, hint, monkeypatch=None):
    """One forward + backward of the MLM + ITM losses on a fresh model -> dict(out, mlm, bce, grads, model, spy)."""
    mp = _parity()
    m, P, sd = mp._build(cfg, dropout=p)
    m.train()
    spy = _NtSpy(monkeypatch) if monkeypatch is not None else None
    m.arena().zero_grad()
    dev, R = 'cuda', cfg['R']
    out = m('jointfwd', x=batch['x'].to(dev), lengths=batch['lengths'].to(dev), x_img=batch['x_img'].to(dev),
            lengths_img=batch['lengths_img'].to(dev), causal=False, langs=None, image_loc=batch['image_loc'].to(dev),
            refine_image=False, out_rows=hint)
    _, mlm = m('predict', tensor=out[R:], pred_mask=batch['pred_mask'].to(dev), y=batch['y'].to(dev), get_scores=False)
    rel = m('predict', tensor=out.transpose(0, 1), is_relation=True)
    onehot = torch.eye(2, device=dev)[batch['pos_labels'].to(dev)].reshape(-1)
    bce = torch.nn.functional.binary_cross_entropy_with_logits(rel.view(-1).float(), onehot)
    (mlm + bce).backward()
    torch.cuda.synchronize()
    grads = {n: q.grad.detach().clone() for n, q in m.named_parameters() if n in sd and q.grad is not None}
    return dict(out=out.detach(), mlm=float(mlm), bce=float(bce), grads=grads, model=m, sd=sd, spy=spy)


_ORACLE = {}


def _oracle(cfg_name, cfg, batch, sd, p, keeps, key=None):
    """Losses, output and every parameter gradient of the oracle (cached: the comparisons below share them)."""
    from oracle import ref_cpu as O
    key = (cfg_name, p) if key is None else key
    if key not in _ORACLE:
        names = list(sd.keys())
        leaves = {n: sd[n].clone().requires_grad_(True) for n in names}
        kw = dict(dropout=p, attention_dropout=p, keeps=keeps) if p > 0 else {}
        res = O.pretrain_losses(leaves, cfg['n_layers'], cfg['n_heads'], batch, cfg['R'], **kw)
        grads = dict(zip(names, torch.autograd.grad(res['total'], [leaves[n] for n in names])))
        _ORACLE[key] = dict(out=res['out'].detach(), mlm=float(res['mlm']), itm=float(res['itm']), grads=grads)
    return _ORACLE[key]


def _selected(out, hint):
    """(selected rows [n_rows, d], the rest) of an (S, B, d) encoder output, rows b * S + s."""
    S, B, d = out.shape
    flat = out.transpose(0, 1).reshape(B * S, d)
    sel = hint._host[0][:hint.n_rows].long().to(flat.device)
    rest = torch.ones(B * S, dtype=torch.bool, device=flat.device)
    rest[sel] = False
    return flat[sel], flat[rest], sel


def _grad_errors(grads, ref):
    """name -> distance of a gradient from the oracle's: relative L2, k_lin.bias (true gradient 0) absolute against the
    q_lin.bias scale - the per-tensor measure of tests/test_model_parity.py."""
    qb = float(ref['attentions.0.q_lin.bias'].norm())
    return {n: (float(g.norm()) / (qb + 1e-30) if '.k_lin.bias' in n else rel_l2(g, ref[n])) for n, g in grads.items()}


@gpu
@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('cfg_name', COMPACT_CFGS)
def test_compact_last_layer_vs_oracle(cfg_name, p, monkeypatch):
    """test_gradients_vs_oracle / test_dropout_on_training_step_vs_oracle_fed_the_same_masks with the hint on, at their
    bars: selected output rows rel_l2 < 1e-2, losses within 5e-3, every gradient within 5e-2; and the compact path ran."""
    mp = _parity()
    cfg = mp._cfg(cfg_name)
    batch = synth.make_batch(cfg['T'], cfg['R'], cfg['B'], cfg['n_words'], cfg['n_pred'], seed=7)
    hint = _hint(cfg, batch)
    assert hint.n == 4352 and 2 * hint.n <= hint.M
    r = _step(cfg, batch, p, hint, monkeypatch)
    r['spy'].assert_compact(hint.n, cfg['emb_dim'])
    m = r['model']
    keeps = encoder_keep_masks(m, m._fwd_counter, cfg['B'], cfg['T'], cfg['R'], p, p) if p > 0 else None
    ref = _oracle(cfg_name, cfg, batch, r['sd'], p, keeps)
    got, rest, sel = _selected(r['out'], hint)
    want = ref['out'].transpose(0, 1).reshape(-1, cfg['emb_dim'])[sel.cpu()]
    err_out = rel_l2(got.float(), want)
    print('%s p=%.1f: out rows %.3e, mlm %.3e, itm %.3e' % (cfg_name, p, err_out, abs(r['mlm'] - ref['mlm']), abs(r['bce'] - ref['itm'])))
    assert bool(torch.isfinite(got.float()).all()) and bool(torch.isnan(rest.float()).all())
    assert err_out < 1e-2
    assert abs(r['mlm'] - ref['mlm']) < 5e-3 and abs(r['bce'] - ref['itm']) < 5e-3
    errs = _grad_errors(r['grads'], ref['grads'])
    assert set(errs) == set(ref['grads'])
    bad = [(n, e) for n, e in errs.items() if e > 5e-2]
    assert not bad, bad


def _assert_no_further_from_oracle(on, off, ref, what):
    """Hint on is no further from the oracle than hint off plus one quarter of that distance, per gradient tensor
    (k_lin.bias, whose true gradient is zero: the absolute bar 5e-2 of the q_lin.bias scale); the forward is the same kernels
    on the same rows with the same dropout decisions: equal losses (asserted here; the callers assert bit-identical rows).
    Returns (largest on-vs-off rel_l2, largest oracle distance off, largest oracle distance on) over the gradients."""
    e_on, e_off = _grad_errors(on['grads'], ref['grads']), _grad_errors(off['grads'], ref['grads'])
    assert set(e_on) == set(e_off)
    d_onoff = {n: rel_l2(on['grads'][n], off['grads'][n]) for n in e_on if '.k_lin.bias' not in n}
    worst = max(d_onoff, key=d_onoff.get)
    print('%s: gradients on-vs-off max rel_l2 %.3e (%s); from the oracle: off max %.3e, on max %.3e; '
          'losses on (%.6f, %.6f) off (%.6f, %.6f) oracle (%.6f, %.6f)' % (
              what, d_onoff[worst], worst, max(e_off.values()), max(e_on.values()), on['mlm'], on['bce'], off['mlm'], off['bce'],
              ref['mlm'], ref['itm']))
    # the losses come from bit-identical rows through the same head kernels: equal, which also meets the 1.25 rule
    assert on['mlm'] == off['mlm'] and on['bce'] == off['bce'], (on['mlm'], off['mlm'], on['bce'], off['bce'])
    # k_lin.bias has a true gradient of zero: both "distances" are the rounding noise of bias sums gathered with atomics, and
    # nothing bounds the ratio of two noise norms - held to the absolute bar of tests/test_model_parity.py instead
    bad = [(n, e_on[n], e_off[n]) for n in e_on if (e_on[n] > 5e-2 if '.k_lin.bias' in n else e_on[n] > 1.25 * e_off[n])]
    assert not bad, bad
    return d_onoff[worst], max(e_off.values()), max(e_on.values())


@gpu
@pytest.mark.parametrize('cfg_name', COMPACT_CFGS)
def test_hint_on_against_hint_off(cfg_name, monkeypatch):
    """Same model, seed, batch, dropout 0.1, with and without the hint.  The bar is not invented: every gradient with the
    hint on must be no further from the oracle than the same gradient with the hint off, plus one quarter of that distance
    (room for reordered fp32 sums and the different K-chunking of the weight gradients, nothing more); the selected output
    rows are the same kernels on the same data and must be bit-identical at dropout 0.1 - which they are only if every keep
    decision of the compact launches is the full launch's (that the decisions are also the NumPy twin's, element by element, is
    asserted on the kernels: test_row_mapped_dropout_of_the_gemm_epilogue / _of_layernorm_backward); losses are equal.

    Measured on the MI355X (largest over all gradient tensors; on-vs-off relative L2 | distance from the oracle, hint off |
    distance from the oracle, hint on):
        tiles              6.6e-07 .. 6.9e-07 | 1.072e-02 | 1.072e-02
        tiles768           9.8e-07 .. 2.0e-04 | 6.914e-03 .. 6.919e-03 | 6.916e-03 .. 6.919e-03
        tiles, ragged set  2.7e-04 .. 3.1e-04 | 9.335e-03 .. 9.342e-03 | 9.313e-03 .. 9.322e-03     (test_ragged_row_set)
    (two runs each; the e-04 entries are bias sums gathered with fp32 atomics, whose order differs from run to run of one
    tree as well);
    losses equal to the last bit in all three."""
    mp = _parity()
    cfg = mp._cfg(cfg_name)
    p = 0.1
    batch = synth.make_batch(cfg['T'], cfg['R'], cfg['B'], cfg['n_words'], cfg['n_pred'], seed=7)
    hint = _hint(cfg, batch)
    on = _step(cfg, batch, p, hint, monkeypatch)
    on['spy'].assert_compact(hint.n, cfg['emb_dim'])
    off = _step(cfg, batch, p, None)
    m = on['model']
    assert m._fwd_counter == off['model']._fwd_counter and m.base_seed == off['model'].base_seed
    keeps = encoder_keep_masks(m, m._fwd_counter, cfg['B'], cfg['T'], cfg['R'], p, p)
    got, _, sel = _selected(on['out'], hint)
    full = off['out'].transpose(0, 1).reshape(-1, cfg['emb_dim'])
    assert bool(torch.isfinite(full.float()).all())
    assert_bits_equal(got.contiguous(), full[sel].contiguous(), 'selected output rows, hint on against hint off')
    ref = _oracle(cfg_name, cfg, batch, on['sd'], p, keeps)
    _assert_no_further_from_oracle(on, off, ref, cfg_name)


def _ragged_batch(cfg):
    """'tiles' with 20 masked tokens per sequence, then: none in sequence 0, three fewer in every fourth sequence."""
    batch = synth.make_batch(cfg['T'], cfg['R'], cfg['B'], cfg['n_words'], 20, seed=11)
    x, labels = batch['x'].clone(), batch['x_labels'].clone()
    for b in range(cfg['B']):
        pos = torch.nonzero(labels[:, b] != -1).view(-1)
        drop = pos if b == 0 else (pos[:3] if b % 4 == 1 else pos[:0])
        x[drop, b] = labels[drop, b]
        labels[drop, b] = -1
    batch.update(x=x, x_labels=labels, pred_mask=labels != -1, y=labels[labels != -1])
    return batch


@gpu
def test_ragged_row_set(monkeypatch):
    """Different numbers of masked tokens per sequence, one sequence with none, a total that is not a multiple of 256: rows
    inside the set are finite, rows outside NaN, and the pad rows change no gradient (hint on against the same batch on the
    full path, by the rule of test_hint_on_against_hint_off)."""
    mp = _parity()
    cfg = mp._cfg('tiles')
    batch = _ragged_batch(cfg)
    per_seq = batch['pred_mask'].sum(0)
    assert int(per_seq[0]) == 0 and len(set(per_seq.tolist())) >= 3
    hint = _hint(cfg, batch)
    assert hint.n_rows == int(per_seq.sum()) + cfg['B'] and hint.n_rows % 256 != 0 and hint.n == 5376
    p = 0.1
    on = _step(cfg, batch, p, hint, monkeypatch)
    on['spy'].assert_compact(hint.n, cfg['emb_dim'])
    off = _step(cfg, batch, p, None)
    got, rest, sel = _selected(on['out'], hint)
    assert bool(torch.isfinite(got.float()).all()) and bool(torch.isnan(rest.float()).all())
    full = off['out'].transpose(0, 1).reshape(-1, cfg['emb_dim'])
    assert_bits_equal(got.contiguous(), full[sel].contiguous(), 'selected output rows of the ragged set')
    m = on['model']
    keeps = encoder_keep_masks(m, m._fwd_counter, cfg['B'], cfg['T'], cfg['R'], p, p)
    ref = _oracle('tiles', cfg, batch, on['sd'], p, keeps, key=('tiles-ragged', p))
    _assert_no_further_from_oracle(on, off, ref, 'tiles, ragged')


def test_eligibility_rule():
    """n < 4 096 or 2 n > M: the full path (CPU: the decision function alone)."""
    from m3p_amd import functional as Fn
    assert Fn.compact_rows_eligible(5120, 41984) == 5120
    assert Fn.compact_rows_eligible(4224, 20992) == 4352 and Fn.compact_rows_eligible(4352, 16384) == 4352
    assert Fn.compact_rows_eligible(3841, 41984) == 4096 and Fn.compact_rows_eligible(3840, 41984) == 0
    assert Fn.compact_rows_eligible(256, 41984) == 0 and Fn.compact_rows_eligible(0, 41984) == 0
    assert Fn.compact_rows_eligible(4096, 8192) == 4096 and Fn.compact_rows_eligible(4097, 8192) == 0
    assert Fn.compact_rows_eligible(5120, 10239) == 0
    # the row set itself: ascending selected rows, pad entries outside the set, the inverse map
    flags = torch.zeros(16384, dtype=torch.bool)
    flags[::4] = True
    flags[5] = True
    r = Fn.OutputRows(flags)
    idx, inv = r._host
    assert (r.M, r.n_rows, r.n) == (16384, 4097, 4352) and idx.dtype == torch.int32 and inv.dtype == torch.int32
    assert torch.equal(idx[:r.n_rows].long(), torch.nonzero(flags).view(-1)) and not bool(flags[idx[r.n_rows:].long()].any())
    assert idx.unique().numel() == r.n
    assert torch.equal(inv[idx[:r.n_rows].long()], torch.arange(r.n_rows, dtype=torch.int32)) and int((inv >= 0).sum()) == r.n_rows
    small = Fn.OutputRows.from_masks(4, 10, 3, pred_mask=torch.zeros(7, 4, dtype=torch.bool))
    assert small.n_rows == 4 and small.n == 0
    both = Fn.OutputRows.from_masks(2, 5, 2, pred_mask=torch.tensor([[1, 0], [0, 0], [0, 1]]), region_labels=torch.tensor([[-1, 3], [-1, -1]]))
    assert torch.nonzero(both.flags).view(-1).tolist() == [0, 1, 2, 5, 9] and both.n_rows == 5


@gpu
def test_ineligible_hint_takes_the_full_path(monkeypatch):
    """A hint with too few rows (the first rows alone) returns a fully valid output and launches nothing at a compact size."""
    mp = _parity()
    cfg = mp._cfg('tiles')
    batch = synth.make_batch(cfg['T'], cfg['R'], cfg['B'], cfg['n_words'], cfg['n_pred'], seed=7)
    from m3p_amd import functional as Fn
    hint = Fn.OutputRows.from_masks(cfg['B'], cfg['T'] + cfg['R'], cfg['R'])
    assert hint.n_rows == cfg['B'] and hint.n == 0
    r = _step(cfg, batch, 0.1, hint, monkeypatch)
    M = cfg['B'] * (cfg['T'] + cfg['R'])
    assert all(s[1] in (M, cfg['B'] * cfg['n_pred'], cfg['B']) for s in r['spy'].shapes), sorted(set(r['spy'].shapes))
    assert bool(torch.isfinite(r['out'].float()).all())


@gpu
@pytest.mark.parametrize('M,n,N,K,kern', [(8192, 4096, 768, 768, 'KERN_NT_W8'), (8192, 4096, 768, 3072, 'KERN_NT_W4'),
                                          (8192, 4096, 256, 1024, 'KERN_NT_RING'), (900, 320, 136, 64, 'KERN_NT_128')])
def test_row_mapped_dropout_of_the_gemm_epilogue(M, n, N, K, kern):
    """gemm_nt(EPI_BIAS_DROP_RES, rng_rows) on gathered rows = the same rows of the launch over all rows, bit for bit (same
    kernel, same K loop, same keep decisions): eight-wave, four-wave, ring and generic kernels."""
    from m3p_amd import lib as L, ops
    lib = L.load()
    assert lib.m3p_gemm_nt_plan(M, N, K, L.EPI_BIAS_DROP_RES) == getattr(L, kern) == lib.m3p_gemm_nt_plan(n, N, K, L.EPI_BIAS_DROP_RES)
    a, _ = randn_bf16((M, K), 1)
    w, _ = randn_bf16((N, K), 2, scale=K ** -0.5)
    res, _ = randn_bf16((M, N), 3)
    bias, _ = randn_f32((N,), 4)
    idx = torch.from_numpy(np.sort(np.random.RandomState(5).permutation(M)[:n]).astype(np.int32)).cuda()
    with poisoned_outputs():
        full = ops.gemm_nt(a, w, L.EPI_BIAS_DROP_RES, bias=bias, aux=res, seed=1234, p_drop=0.1)
        part = ops.gemm_nt(a[idx.long()].contiguous(), w, L.EPI_BIAS_DROP_RES, bias=bias, aux=res[idx.long()].contiguous(),
                           seed=1234, p_drop=0.1, rng_rows=idx)
        plain = ops.gemm_nt(a[idx.long()].contiguous(), w, L.EPI_BIAS_DROP_RES, bias=bias, aux=res[idx.long()].contiguous(),
                            seed=1234, p_drop=0.1)
    assert_bits_equal(part, full[idx.long()].contiguous(), 'row-mapped dropout (%s)' % kern)
    assert not torch.equal(plain, part)          # (without the map the launch draws the decisions of rows 0 .. n - 1)
    # ... and they are the NumPy twin's decisions for the rows' positions in the FULL tensor: a dropped element is exactly the
    # residual; a kept one differs from it (but for the few whose product rounds away against the residual)
    from m3p_amd import rng
    keep = torch.from_numpy(rng.keep_mask(M * N, 1234, 0.1, (M, N)))[idx.long().cpu()].cuda()
    same = part == res[idx.long()]
    assert bool(same[~keep].all()), 'an element the twin drops was kept'
    assert float(same[keep].float().mean()) < 1e-2, 'elements the twin keeps were dropped'
    assert abs(float((~keep).float().mean()) - 0.1) < 1e-2


@gpu
@pytest.mark.parametrize('d', [768, 256])
def test_row_mapped_dropout_of_layernorm_backward(d):
    """dx and dx_drop of m3p_layernorm_bwd_rows on gathered rows = those rows of the launch over all rows, bit for bit
    (d = 768: the half-wave kernel; 256: the generic one); the column sums agree to fp32 summation order."""
    from m3p_amd import ops
    M, n = 6000, 2048
    x, _ = randn_bf16((M, d), 1)
    dy, _ = randn_bf16((M, d), 2)
    g, _ = randn_f32((d,), 3)
    b, _ = randn_f32((d,), 4)
    _, mean, rstd = ops.layernorm_fwd(x, g, b)
    idx = torch.from_numpy(np.sort(np.random.RandomState(5).permutation(M)[:n]).astype(np.int32)).cuda()
    il = idx.long()
    zeros = lambda: torch.zeros(d, dtype=torch.float32, device='cuda')       # noqa: E731
    dy_sel = torch.zeros_like(dy)
    dy_sel[il] = dy[il]
    with poisoned_outputs():
        gf, bf, cf = zeros(), zeros(), zeros()
        dx_f, dd_f = ops.layernorm_bwd(dy_sel, None, x, g, mean, rstd, None, gf, bf, dbias_drop=cf, want_drop=True, seed=77, p_drop=0.1)
        gp, bp, cp = zeros(), zeros(), zeros()
        dx_p, dd_p = ops.layernorm_bwd(dy[il].contiguous(), None, x[il].contiguous(), g, mean[il].contiguous(), rstd[il].contiguous(),
                                       None, gp, bp, dbias_drop=cp, want_drop=True, seed=77, p_drop=0.1, rng_rows=idx)
    assert_bits_equal(dx_p, dx_f[il].contiguous(), 'dx')
    assert_bits_equal(dd_p, dd_f[il].contiguous(), 'dx_drop')
    from m3p_amd import rng
    keep = torch.from_numpy(rng.keep_mask(M * d, 77, 0.1, (M, d)))[il.cpu()].cuda()      # the twin, at the rows of the full tensor
    assert bool((dd_p[~keep] == 0).all()), 'an element the twin drops was kept'
    assert float((dd_p[keep] == 0).float().mean()) < 1e-2, 'elements the twin keeps were dropped'
    assert abs(float((~keep).float().mean()) - 0.1) < 1e-2
    for got, want, what in ((gp, gf, 'dgamma'), (bp, bf, 'dbeta'), (cp, cf, 'dbias_drop')):
        assert rel_l2(got, want) < 1e-5, what       # (the rows outside the set add exact zeros to the full launch's sums)


@gpu
@pytest.mark.parametrize('M,n,d', [(41984, 5120, 768), (1000, 300, 264)])
def test_place_rows(M, n, d):
    """One pass writes the fill value everywhere and the compact rows in their places; indices outside [0, n) count as not
    selected."""
    from m3p_amd import ops
    src, _ = randn_bf16((n, d), 1)
    rows = np.sort(np.random.RandomState(2).permutation(M)[:n - 7])          # the last 7 compact rows are pad entries
    inv = torch.full((M,), -1, dtype=torch.int32)
    inv[torch.from_numpy(rows)] = torch.arange(n - 7, dtype=torch.int32)
    inv[int(np.setdiff1d(np.arange(M), rows)[0])] = n + 5                       # out of range: treated as -1
    inv = inv.cuda()
    for bits in (0, ops.BF16_NAN_BITS):
        with poisoned_outputs():
            out = ops.place_rows(src, inv, M, bits)
        want = torch.zeros((M, d), dtype=BF16, device='cuda') if bits == 0 else torch.full((M, d), float('nan'), dtype=BF16, device='cuda')
        want[torch.from_numpy(rows).cuda()] = src[:n - 7]
        assert out.shape == (M, d)
        if bits == 0:
            assert_bits_equal(out, want, 'place_rows, zero fill')
        else:
            sel = torch.zeros(M, dtype=torch.bool, device='cuda')
            sel[torch.from_numpy(rows).cuda()] = True
            assert_bits_equal(out[sel].contiguous(), want[sel].contiguous(), 'place_rows, placed rows')
            assert bool(torch.isnan(out[~sel].float()).all())


LOSS_ULPS = 16      # bar of the trainer comparison below, in spacings of fp32 at the loss's value


@gpu
def test_three_trainer_steps_with_and_without_the_hint(monkeypatch):
    """XTrainer.pretrain_under_step x 3 at a compact-eligible size ('tiles', dropout 0.1), with the hint, without it, and
    without it a second time (what two runs of the SAME path differ by: the order of sums gathered with atomics).

    The bar comes from what test_hint_on_against_hint_off measured: one forward + backward gives losses equal to the last
    bit and gradients within 3e-04 relative L2, no more than two runs of one tree differ by.  Step 1 is a forward on untouched
    weights: equal.  Adam then moves every weight by lr * m / (sqrt(v) + eps), in which a relative change of the gradient
    of that size is a relative change of the same size of a step of 1e-4: the later losses, fp32 means of thousands of rows,
    can differ by their own rounding and no more - LOSS_ULPS = 16 spacings of fp32 at the loss's value (1.5e-05 at 8.57,
    9.5e-07 at 0.69).  A last-layer gradient that is wrong or missing under the hint moves the weights of that layer by
    the whole step and the loss by 1e-4 and more.
    Measured on the MI355X, in fp32 spacings per step (CMLM, t2i), two runs of the test: hint on against hint off (0, 0),
    (0, 0), (0, 3) in one and (0, 0) three times in the other; hint off against hint off (0, 0) three times."""
    from m3p_amd.trainer import XTrainer
    mp = _parity()
    cfg = mp._cfg('tiles')
    B, R = cfg['B'], cfg['R']
    batch = synth.make_batch(cfg['T'], R, B, cfg['n_words'], cfg['n_pred'])
    img = batch['x_img'].transpose(0, 1).contiguous()
    loc = batch['image_loc'].transpose(0, 1).contiguous()
    tup = ((batch['x'], batch['lengths'], batch['x_labels']),
           (img, torch.ones(B, R, dtype=torch.long), loc, torch.full((B, R), -1), batch['pos_labels'].tolist(), None, None))
    runs = {}
    for name, hint_on in (('on', True), ('off', False), ('off2', False)):
        m, P, sd = mp._build(cfg, dropout=0.1)
        for k, v in dict(optimizer='adam_inverse_sqrt,beta1=0.9,beta2=0.98,lr=0.0001', clip_grad_norm=5, amp=-1, fp16=False,
                         accumulate_gradients=1, multi_gpu=False, epoch_size=100, cross_mlm_steps=[('google', 'img')],
                         cross_mrm_steps=[], cross_mrfr_steps=[], cross_clcm_steps=[], sample_n=2, refine_image=False,
                         multi_cls_loss_weight=0, bin_cls_loss_weight=1, batch_size=B, dump_path='/nonexistent_m3p_dump').items():
            setattr(P, k, v)
        tr = XTrainer(m, {}, P)
        with pytest.MonkeyPatch.context() as patch:
            spy = _NtSpy(patch)
            if not hint_on:
                patch.setattr(XTrainer, '_output_rows', staticmethod(lambda *a, **kw: None))
            losses = []
            for step in range(3):
                tr.pretrain_under_step(tup, 'google', 't2i', 'en', 1.0, 1.0, 1.0, 1.0)
                losses.append((float(tr.stats['CMLM-google'][-1]), float(tr.stats['t2i-google'][-1])))
                tr.iter()
            spy.assert_compact(4352, cfg['emb_dim'], ran=hint_on)
        runs[name] = losses
    ulps = lambda a, b: abs(a - b) / float(np.spacing(np.float32(max(abs(a), abs(b)))))       # noqa: E731
    for name in ('on', 'off', 'off2'):
        print('trainer losses, hint %-4s:' % name, runs[name])
    print('hint on  vs off , fp32 spacings per step (CMLM, t2i):', [(ulps(a[0], b[0]), ulps(a[1], b[1])) for a, b in zip(runs['on'], runs['off'])])
    print('hint off vs off2, fp32 spacings per step (CMLM, t2i):', [(ulps(a[0], b[0]), ulps(a[1], b[1])) for a, b in zip(runs['off'], runs['off2'])])
    assert all(np.isfinite(v) for run in runs.values() for pair in run for v in pair)
    assert runs['on'][0] == runs['off'][0]
    for a, b in zip(runs['on'], runs['off']):
        assert ulps(a[0], b[0]) <= LOSS_ULPS and ulps(a[1], b[1]) <= LOSS_ULPS, (runs['on'], runs['off'])
