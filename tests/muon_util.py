"""The Muon update as a float64 oracle, and a bf16-storage emulation of it (helper module of tests/test_muon.py and tests/test_muon_gpu.py).

Oracle (float64 throughout, no rounding anywhere):
    g = grad * clip_coef;  buf += (1 - momentum) (g - buf);  u = g + momentum (buf - g) if nesterov else buf
    X = u / (||u||_F + 1e-7), held as [min, max];  ns_steps times:  A = X X^T;  B = b A + c A A;  X = a X + B X
    w = w (1 - lr wd) - lr scale X        scale = 0.2 sqrt(max(r, c))  |  sqrt(max(1, r / c))
Emulation: the same statements with X, A and B rounded to bf16 after each one (float64 accumulation) -- the coarsest storage the optimizer may use.
Its distance from the oracle is the yardstick of the GPU tests: a kernel may round at other (legal) points, so it gets twice that distance plus
2^-9 (one bf16 rounding of the result), computed per input, never a constant."""
import math

import torch

NS = (3.4445, -4.7750, 2.0315)
PARITY_SHAPES = ((64, 64), (64, 192), (192, 64), (96, 160), (40, 72), (352, 588))
PARITY_KINDS = ("gaussian", "scaled_columns")


def rb(x):
    """float64 -> nearest bf16 value, as float64"""
    return x.float().to(torch.bfloat16).double()


def parity_input(shape, kind, seed, device="cpu"):
    """seeded full-rank inputs: Gaussian, and Gaussian with its columns scaled by logspace(0, -3)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    if kind == "scaled_columns":
        x = x * torch.logspace(0, -3, shape[1], dtype=torch.float64)
    else:
        assert kind == "gaussian"
    return x.float().to(device)


def low_rank_input(shape, rank, seed, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape[0], rank, generator=g, dtype=torch.float64) @ torch.randn(rank, shape[1], generator=g, dtype=torch.float64)).float().to(device)


def partial_permutation(shape, k, seed, scale=1.0, device="cpu"):
    """s * P: k nonzeros, no two in one row or column"""
    g = torch.Generator().manual_seed(seed)
    rows = torch.randperm(shape[0], generator=g)[:k]
    cols = torch.randperm(shape[1], generator=g)[:k]
    p = torch.zeros(shape, dtype=torch.float32)
    p[rows, cols] = scale
    return p.to(device)


def newton_schulz(u, ns_steps=5, emulate=False):
    """u float64 [r, c] -> the orthogonalised matrix in u's orientation"""
    a, b, c = NS
    r = (lambda t: rb(t)) if emulate else (lambda t: t)
    x = u / (u.norm() + 1e-7)
    tall = u.shape[0] > u.shape[1]
    x = r(x.t() if tall else x)
    for _ in range(ns_steps):
        A = r(x @ x.t())
        B = r(b * A + c * (A @ A))
        x = r(a * x + B @ x)
    return x.t() if tall else x


def lr_scale(adjust_lr, rows, cols):
    return 0.2 * math.sqrt(max(rows, cols)) if adjust_lr == "match_rms_adamw" else math.sqrt(max(1.0, rows / cols))


def direction(grad, buf, momentum, nesterov, clip_coef=1.0):
    """(new buffer, update direction), float64"""
    g = grad.double() * clip_coef
    buf = buf + (1.0 - momentum) * (g - buf)
    return buf, (g + momentum * (buf - g)) if nesterov else buf


def muon_update(w, grad, buf, lr, weight_decay, momentum, nesterov, ns_steps, adjust_lr, clip_coef=1.0, emulate=False):
    """one step on one weight (any ndim >= 2, used as [shape[0], -1]); all float64; returns (new w, new buf)"""
    rows = w.shape[0]
    buf, u = direction(grad.reshape(rows, -1), buf.reshape(rows, -1), momentum, nesterov, clip_coef)
    x = newton_schulz(u, ns_steps, emulate)
    cols = u.shape[1]
    new = w.double().reshape(rows, -1) * (1.0 - lr * weight_decay) - lr * lr_scale(adjust_lr, rows, cols) * x
    return new.reshape(w.shape), buf.reshape(w.shape)


def clip_coef(grads, max_norm):
    """torch.nn.utils.clip_grad_norm_'s coefficient from the global norm over ``grads``, float64"""
    if max_norm is None:
        return 1.0
    total = math.sqrt(sum(float(g.double().pow(2).sum()) for g in grads))
    return min(1.0, max_norm / (total + 1e-6))


def rel_err(got, want):
    return float((got.double() - want.double()).norm() / want.double().norm())


def bound(err_emulation):
    return 2.0 * err_emulation + 2.0 ** -9


def scalar_recursion(k, ns_steps=5, emulate=False):
    """the singular value of s * P / ||s * P|| (= 1 / sqrt(k), k times) under the iteration: sigma <- a sigma + b sigma^3 + c sigma^5 in float64;
    ``emulate``: with every stored quantity (X, A, B) rounded to bf16, as a kernel that stores them in bf16 computes it"""
    a, b, c = NS
    if not emulate:
        s = 1.0 / math.sqrt(k)
        for _ in range(ns_steps):
            s = a * s + b * s ** 3 + c * s ** 5
        return s
    r = lambda v: float(rb(torch.tensor(v, dtype=torch.float64)))
    s = r(1.0 / (math.sqrt(k) + 1e-7))
    for _ in range(ns_steps):
        A = r(s * s)
        B = r(b * A + c * A * A)
        s = r(a * s + B * s)
    return s
