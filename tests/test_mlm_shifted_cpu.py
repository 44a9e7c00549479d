"""The algebra of the MLM head without a gradient pass over the logits, restated in torch fp64 and compared with autograd on
F.cross_entropy(mean) (no GPU needed).

Softmax is invariant under a per-row shift and its normaliser is a per-row scalar.  With t_n the target's own logit and
c_n = t_n + SHIFT the vocabulary projection stores e[n, v] = exp(x[n, v] - c_n), an exact 0 at the target column, and
  Sigma_n = sum_v e[n, v] + exp(-SHIFT),  lse_n = c_n + log Sigma_n,  loss_n = lse_n - t_n,
  s_n = gs / Sigma_n,  q_n = gs * expm1(t_n - lse_n)                                   (gs = 1 / n_rows)
  db = g * sum_n s_n e[n, :],  db[y_n] += g q_n
  dE = e^T x (g s_n H[n, :]),  dE[y_n, :] += g q_n H[n, :]
  dH[n, :] = g * (s_n (e x E)[n, :] + q_n E[y_n, :])
(csrc/heads.hip, csrc/gemm.hip: epilogue_half_exp)."""
import math

import torch

SHIFT = 40.0


def _shifted_head(H, E, b, y, g, shift=SHIFT, dtype=torch.float64):
    """loss (mean), dH, dE, db of the tied projection + cross-entropy by the shifted-exponential algebra."""
    n = H.shape[0]
    rows = torch.arange(n)
    gs = 1.0 / n
    x = (H @ E.t() + b).to(dtype)
    t = x[rows, y]
    c = t + shift
    e = torch.exp(x - c[:, None])
    e[rows, y] = 0.0                                     # the target column is kept out of e
    sigma = e.sum(1) + torch.exp(torch.tensor(-shift, dtype=dtype))
    lse = c + torch.log(sigma)
    loss_n = lse - t
    s = gs / sigma
    q = gs * torch.expm1(t - lse)
    db = g * (s[:, None] * e).sum(0)
    db.index_add_(0, y, g * q)
    dE = e.t() @ (g * s[:, None] * H.to(dtype))
    dE.index_add_(0, y, g * q[:, None] * H.to(dtype))
    dH = g * (s[:, None] * (e @ E.to(dtype)) + q[:, None] * E.to(dtype)[y])
    return loss_n, dH, dE, db


def test_shifted_exponential_algebra_equals_autograd_of_cross_entropy():
    n, V, d = 8, 37, 16
    gen = torch.Generator().manual_seed(5)
    H = torch.randn((n, d), generator=gen, dtype=torch.float64).requires_grad_(True)
    E = torch.randn((V, d), generator=gen, dtype=torch.float64).requires_grad_(True)
    b = torch.randn((V,), generator=gen, dtype=torch.float64).requires_grad_(True)
    y = torch.tensor([3, 36, 3, 0, 17, 36, 3, 9])        # ids repeat across rows; id V - 1 is among them
    g = 0.7                                              # the upstream gradient of the loss
    loss = torch.nn.functional.cross_entropy(H @ E.t() + b, y, reduction='mean')
    dH_ref, dE_ref, db_ref = torch.autograd.grad(loss, [H, E, b], grad_outputs=torch.tensor(g, dtype=torch.float64))
    loss_n, dH, dE, db = _shifted_head(H.detach(), E.detach(), b.detach(), y, g)
    assert abs(float(loss_n.mean()) - float(loss)) < 1e-12
    for got, ref in ((dH, dH_ref), (dE, dE_ref), (db, db_ref)):
        assert float((got - ref).abs().max()) < 1e-12


def test_the_window_of_the_shift_in_fp32():
    """fp32 row sums of bf16-rounded exponentials: a row whose target sits 100 nats below the maximum stays finite and right;
    past x_max - t > 88.7 - ln(count of such columns) + SHIFT the sum overflows and the loss is NON-FINITE, never finite and wrong."""
    V = 37

    def row_loss(gap):
        x = torch.zeros(V, dtype=torch.float64)
        x[1:] = gap                                       # every other column `gap` nats above the target (column 0)
        e = torch.exp((x - (x[0] + SHIFT)).float()).to(torch.bfloat16).float()      # what the epilogue stores
        e[0] = 0.0
        sigma = e.sum(dtype=torch.float32) + torch.exp(torch.tensor(-SHIFT, dtype=torch.float32))
        return float(SHIFT + torch.log(sigma)), float(torch.logsumexp(x, 0) - x[0])

    got, ref = row_loss(100.0)
    assert math.isfinite(got) and abs(got - ref) < 2.0 ** -8 + 1e-4          # (one bf16 rounding of the stored values)
    limit = math.log(torch.finfo(torch.float32).max) - math.log(V - 1) + SHIFT      # 88.7 - ln 36 + 40
    got, _ = row_loss(limit - 0.5)
    assert math.isfinite(got)
    got, _ = row_loss(limit + 0.5)
    assert not math.isfinite(got)
    # the smallest value a row is guaranteed to hold at full precision: the row maximum is at least the target's logit
    assert math.exp(-SHIFT) > 2.0 ** -126 * 2.0 ** 60     # e^-40 sits 47 nats (2^67) above bf16's smallest normal number
