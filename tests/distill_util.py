"""Shared by tests/test_distill.py (CPU) and tests/test_distill_gpu.py: the float64 oracle of the reference's ``DistillClipLoss``
(src/open_clip/loss.py:187-223), written from its formula

    contrastive = (CE(l_img, arange) + CE(l_txt, arange)) / 2
    distill     = (D(t_img, l_img) + D(t_txt, l_txt)) / 2,   D(t, l) = mean_r(lse(l_r) - sum_j softmax(t_r)_j l_rj)

on the gathered features (l = student logits, t = teacher logits, both from the same ``get_logits``), the CPU stand-in for the HIP compute seam with
a ``distill`` method, and the rank emulation's collectives for a loss that gathers two different packed widths."""
import torch

from tests.rank_emulation import Collectives
from tests.test_dist_loss_gloo import CpuPairTerm

F64 = torch.float64


class CpuDistillPairTerm(CpuPairTerm):
    """``CpuPairTerm`` with the ``grad=`` keyword and the ``distill`` method of open_clip_amd.loss._PairTerm"""

    def __init__(self, X, Y, scale, grad=True):
        super().__init__(X, Y, scale)
        self.wants_grad = grad

    def distill(self, teacher_term, loss_scale, grad_scale, acc):
        assert self.wants_grad and not teacher_term.wants_grad, "the teacher's term, and only it, is built with grad=False"
        l, t = self.logits, teacher_term.logits
        q = torch.softmax(t, -1)
        acc[0] += ((torch.logsumexp(l, -1) - (q * l).sum(-1)) * loss_scale).sum()
        self.G = (torch.softmax(l, -1) - q) * grad_scale
        acc[1] += (self.G * l).sum()


class PackedCollectives(Collectives):
    """``gathered`` is the widest packed gather, [W*B, 2E + 2E_t] = student image | text | teacher image | text; a narrower request ([W*B, 2E], the
    contrastive part's) is served from its leading columns"""

    def all_gather(self, out, inp, comm=None):
        assert out.shape[0] == self.gathered.shape[0] and out.shape[1] <= self.gathered.shape[1]
        out.copy_(self.gathered[:, :out.shape[1]])


def distill_rows_f64(l, t):
    """per-row distillation term lse(l) - sum_j softmax(t)_j l_j, in float64"""
    l, t = l.to(F64), t.to(F64)
    return torch.logsumexp(l, -1) - (torch.softmax(t, -1) * l).sum(-1)


def reference_losses(I, T, s, DI, DT, ds):
    """(contrastive, distill) of the reference formula on whole (gathered) feature matrices, in float64, differentiable in I, T, s"""
    li = (s * I) @ T.t()
    ti = (ds * DI.to(F64)) @ DT.to(F64).t()
    lab = torch.arange(I.shape[0], device=I.device)
    c = (torch.nn.functional.cross_entropy(li, lab) + torch.nn.functional.cross_entropy(li.t(), lab)) / 2
    d = (distill_rows_f64(li, ti).mean() + distill_rows_f64(li.t(), ti.t()).mean()) / 2
    return c, d


def reference_grads(I, T, s, DI, DT, ds, wc=1.0, wd=1.0):
    """float64 autograd of wc * contrastive + wd * distill -> (contrastive, distill, dI, dT, dscale)"""
    I, T = I.detach().to(F64).requires_grad_(True), T.detach().to(F64).requires_grad_(True)
    s = torch.as_tensor(s).detach().to(F64).clone().requires_grad_(True)
    c, d = reference_losses(I, T, s, DI.detach(), DT.detach(), torch.as_tensor(ds).detach().to(F64))
    (wc * c + wd * d).backward()
    return c.detach(), d.detach(), I.grad, T.grad, s.grad


def bf16_round(x):
    return x.to(torch.bfloat16).to(F64)


def distill_on_rounded_operands(I, T, s, DI, DT, ds, rows=None, weight=None, ideal=False):
    """The distillation term and its gradients in float64 on the operands the device multiplies: logits = bf16(s X) @ bf16(Y)^T for both models, the
    gradients through the same rounded rows (dX = s G @ bf16(Y), dY = G^T @ bf16(s X)).  ``rows`` = (lo, hi): only those rows of both directions (one
    rank's share of the row-sharded / local forms; the columns are everything), ``weight`` = the loss and gradient weight per row (default
    0.5 / number of rows).  ``ideal=True``: G is rounded once to bf16 before the products -- the error an implementation that stores G in bf16
    cannot avoid.  Returns dict(loss, dI_rows, dT_rows, dI_cols, dT_cols, dscale, gl_abs): gradients through the row operands [hi - lo, E] and
    through the column operands [N, E]; gl_abs = sum |G * logits| (the magnitude d/dscale is judged against)."""
    N = I.shape[0]
    lo, hi = rows if rows is not None else (0, N)
    w = weight if weight is not None else 0.5 / (hi - lo)
    s64, ds64 = float(s), float(ds)
    Is, Ts, I16, T16 = bf16_round(I.float() * s), bf16_round(T.float() * s), bf16_round(I), bf16_round(T)
    DIs, DTs, DI16, DT16 = bf16_round(DI.float() * ds), bf16_round(DT.float() * ds), bf16_round(DI), bf16_round(DT)
    out = {"loss": 0.0, "dscale": 0.0, "gl_abs": 0.0}
    grads = {}
    for name, Xs, Y16, DXs, DY16 in (("img", Is, T16, DIs, DT16), ("txt", Ts, I16, DTs, DI16)):
        l, t = Xs[lo:hi] @ Y16.t(), DXs[lo:hi] @ DY16.t()
        out["loss"] += float(distill_rows_f64(l, t).sum() * w)
        G = (torch.softmax(l, -1) - torch.softmax(t, -1)) * w
        out["dscale"] += float((G * l).sum() / s64)
        out["gl_abs"] += float((G * l).abs().sum())
        if ideal:
            G = bf16_round(G)
        grads[name] = (s64 * (G @ Y16), G.t() @ Xs[lo:hi])  # (through the rows' operand, through the columns' operand)
    out["dI_rows"], out["dT_cols"] = grads["img"]
    out["dT_rows"], out["dI_cols"] = grads["txt"]
    return out


def rel_l2(got, ref):
    got, ref = got.detach().to(F64).cpu(), ref.detach().to(F64).cpu()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))
