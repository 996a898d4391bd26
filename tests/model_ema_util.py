"""The float64 oracle of the model EMA tests (tests/test_model_ema.py, tests/test_model_ema_gpu.py) and the bound the kernel is held to.

Oracle: ``e + (1 - decay) * (p - e)`` in double, from the fp32 values.

Bound per element: ``2^-22 * (|e| + |p|)``.  The kernel (ocn_ema_lerp_multi, include/openclip_hip.h) rounds to fp32 three times -- the difference
``d = p - e`` (error <= 2^-24 |d| <= 2^-24 (|e| + |p|)), the product with the weight and the final sum (together <= 2^-24 of the result plus 2^-24 w |d|,
or one rounding where the compiler contracts them into an fma) -- and the weight itself (or ``1 - weight``) is an fp32 rounding of the Python double
(<= 2^-24 relative, i.e. <= 2^-24 |d| in the result).  The sum stays below 4 * 2^-24 * (|e| + |p|) = 2^-22 (|e| + |p|) with a slack of less than 2x.
It is derived, not measured; an indexing or weight mistake moves an element by about ``weight * |p - e|``, orders of magnitude more."""
import torch


def lerp_oracle(e, p, decay):
    e, p = e.detach().double(), p.detach().double()
    return e + (1.0 - decay) * (p - e)


def lerp_bound(e, p):
    return 2.0 ** -22 * (e.detach().double().abs() + p.detach().double().abs())


def assert_within(name, got, oracle, bound):
    """every element of ``got`` within ``bound`` of ``oracle`` (all float64, same shape); prints the worst ratio before it asserts"""
    err = (got.detach().double() - oracle).abs()
    assert torch.isfinite(got).all(), f"{name}: non-finite"
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{name}: worst |got - oracle| / bound = {ratio:.3f}, max abs err {float(err.max()) if err.numel() else 0.0:.3e}")
    bad = int((err > bound).sum())
    assert bad == 0, f"{name}: {bad} of {err.numel()} elements beyond 2^-22 (|e| + |p|) (worst ratio {ratio:.3f})"
