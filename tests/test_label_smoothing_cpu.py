"""Label smoothing of the vocabulary head, the parts that need no GPU: the identity the kernels implement
(m3p_amd.functional.label_smoothing_ref) against PyTorch's own cross_entropy(label_smoothing=eps) in fp64, and the
``params.label_smoothing`` field of the model."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from m3p_amd import synth
from m3p_amd.functional import label_smoothing_ref
from m3p_amd.model.transformer import TransformerModel

N, D, V = 7, 16, 37


def _case():
    gen = torch.Generator().manual_seed(4242)
    h = torch.randn(N, D, dtype=torch.float64, generator=gen)
    emb = torch.randn(V, D, dtype=torch.float64, generator=gen)
    bias = torch.randn(V, dtype=torch.float64, generator=gen)
    y = torch.tensor([0, V - 1, 5, 5, 11, 0, 23])           # target 0, target V - 1, repeats
    return h, emb, bias, y


@pytest.mark.parametrize('eps', [0.1, 0.3])
@pytest.mark.parametrize('g', [1.0, -0.75])
def test_correction_reproduces_torch_label_smoothing(eps, g):
    h, emb, bias, y = _case()

    def grads(ls):
        hh, ee, bb = (t.clone().requires_grad_(True) for t in (h, emb, bias))
        loss = F.cross_entropy(hh @ ee.t() + bb, y, label_smoothing=ls)
        (g * loss).backward()
        return loss.detach(), hh.grad, ee.grad, bb.grad

    plain, smooth = grads(0.0), grads(eps)
    corr = label_smoothing_ref(h, emb, bias, y, eps, g=g)
    for name, p, c, s in zip(('loss', 'dh', 'demb', 'dbias'), plain, corr, smooth):
        err = float((p + c - s).abs().max())
        assert err <= 1e-12, '%s: plain + correction is off PyTorch\'s smoothed value by %.3g' % (name, err)
    # the correction is not a rounding-size quantity: the test would notice its absence
    assert float((smooth[1] - plain[1]).abs().max()) > 1e-4


def _params(**extra):
    return synth.model_params(64, 2, 1, 100, **extra)


@pytest.mark.parametrize('eps', [-0.1, 1.0])
def test_out_of_range_raises(eps):
    with pytest.raises(ValueError):
        TransformerModel(_params(label_smoothing=eps), is_encoder=True, with_output=True, is_crossModal=True)


def test_field_and_default():
    assert _params().label_smoothing == 0.0
    assert TransformerModel(_params(), True, True, is_crossModal=True).label_smoothing == 0.0
    assert TransformerModel(_params(label_smoothing=0.1), True, True, is_crossModal=True).label_smoothing == pytest.approx(0.1)


def test_old_style_params_without_the_attribute():
    p = _params()
    old = SimpleNamespace(**{k: v for k, v in vars(p).items() if k != 'label_smoothing'})
    assert not hasattr(old, 'label_smoothing')
    assert TransformerModel(old, True, True, is_crossModal=True).label_smoothing == 0.0
