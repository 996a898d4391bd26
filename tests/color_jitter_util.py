"""The float64 oracle of ``ocn_color_jitter_u8`` and the rule by which an output is judged against it.  Written from the definition in
include/openclip_hip.h (up to four steps in the plan's order, each ending in a clamp, grayscale behind them, rounded once).  Neither torchvision nor
PIL is needed: the definition is the project's own.

The acceptance rule, DELTA = 2**-9: an output value must equal round(255 * oracle) wherever the oracle's fractional part (in levels) is at least DELTA
away from .5; inside that band either neighbour is accepted.  Where DELTA comes from: the same chain restated in numpy fp32 (``chain(..., dtype=
np.float32)``) differs from the float64 one by at most 2.9e-4 to 3.5e-4 levels, depending on the seeds -- measured over all 24 orders, on noise and on
low-contrast images (where the hue step amplifies most), factors in 0.6-1.4, hue +-0.1, with and without grayscale.  2**-9 = 1.95e-3 leaves 5x to 7x
for what the kernel does differently from that restatement: fma contraction, hardware reciprocals (1 ulp), multiplications by the rounded 1/255 and
1/6.  On those inputs 0.3 % to 0.4 % of the oracle's values lie in the band on average and 0.75 % at
most.  tests/test_color_jitter.py re-measures the fp32 restatement and asserts that it stays within DELTA / 4.  The band
must not be able to hide a failure, so every comparison also asserts, on the oracle alone, that at most MAX_BAND_FRACTION of its values lie inside
it; very small images have few values, so a launch's images are judged together."""
import itertools

import numpy as np

DELTA = 2.0 ** -9
MAX_BAND_FRACTION = 0.02
BRIGHTNESS, CONTRAST, SATURATION, HUE = 1, 2, 3, 4
GRAY_BIT = 1 << 12
ORDERS = list(itertools.permutations((BRIGHTNESS, CONTRAST, SATURATION, HUE)))  # all 24


def make_plan(steps, gray=False):
    """plan entry: the step codes of ``steps`` (at most 4) from the low bits up, bit 12 = grayscale"""
    assert len(steps) <= 4
    return sum(int(c) << (3 * k) for k, c in enumerate(steps)) + (GRAY_BIT if gray else 0)


def plan_steps(plan):
    """(step codes in execution order without the 'nothing' codes, grayscale)"""
    codes = [(int(plan) >> (3 * k)) & 7 for k in range(4)]
    return [c for c in codes if 1 <= c <= 4], bool(int(plan) & GRAY_BIT)


def gray_of(x):
    return x.dtype.type(0.2989) * x[..., 0] + x.dtype.type(0.587) * x[..., 1] + x.dtype.type(0.114) * x[..., 2]


def hue_step(x, h):
    """rgb -> hsv, hh <- (hh + h) mod 1, hsv -> rgb, in x's dtype"""
    T = x.dtype.type
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    maxc, minc = x.max(axis=-1), x.min(axis=-1)
    cr = maxc - minc
    eq = maxc == minc
    one = np.ones_like(maxc)
    s = cr / np.where(eq, one, maxc)
    crd = np.where(eq, one, cr)
    rc, gc, bc = (maxc - r) / crd, (maxc - g) / crd, (maxc - b) / crd
    isr, isg = maxc == r, maxc == g
    hh = np.where(isr, bc - gc, T(0)) + np.where(isg & ~isr, T(2) + rc - bc, T(0)) + np.where(~isg & ~isr, T(4) + gc - rc, T(0))
    hh = np.fmod(hh / T(6) + T(1), T(1))
    hh = hh + T(h)
    hh = hh - np.floor(hh)
    hh = np.where(hh >= 1, T(0), hh)  # (hh + h) mod 1 lies in [0, 1)
    v = maxc
    i = np.floor(T(6) * hh)
    f = T(6) * hh - i
    i = i.astype(np.int64) % 6
    clamp = lambda a: np.clip(a, T(0), T(1))  # noqa: E731
    p, q, t = clamp(v * (T(1) - s)), clamp(v * (T(1) - s * f)), clamp(v * (T(1) - s * (T(1) - f)))
    table = np.stack([np.stack(c, axis=-1) for c in ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))])  # [6, ..., 3]
    return np.take_along_axis(table, i[None, ..., None].repeat(3, axis=-1), axis=0)[0]


def chain(img_u8, factors, plan, dtype=np.float64, clamp_steps=True):
    """one image uint8 [H, W, 3] -> ``dtype`` [H, W, 3] in [0, 1], unrounded.  ``clamp_steps=False`` leaves out the clamps between the steps (what
    the clamp tests compare with)"""
    T = np.dtype(dtype).type
    x = np.asarray(img_u8).astype(dtype) / T(255)
    fac = [T(v) for v in np.asarray(factors, dtype=np.float32)]  # the kernel's factors are fp32 values
    clamp = (lambda a: np.clip(a, T(0), T(1))) if clamp_steps else (lambda a: a)
    steps, gray = plan_steps(plan)
    for c in steps:
        if c == BRIGHTNESS:
            x = clamp(fac[0] * x)
        elif c == CONTRAST:
            m = gray_of(x).mean(dtype=dtype)
            x = clamp(fac[1] * x + (T(1) - fac[1]) * m)
        elif c == SATURATION:
            x = clamp(fac[2] * x + (T(1) - fac[2]) * gray_of(x)[..., None])
        else:
            x = hue_step(np.clip(x, T(0), T(1)), fac[3])
    if gray:
        x = np.repeat(gray_of(x)[..., None], 3, axis=-1)
    return x


def oracle(img_u8, factors, plan):
    """img uint8 [B, H, W, 3], factors [B, 4], plan [B] -> float64 [B, H, W, 3] in LEVELS (255 x), unrounded"""
    img_u8, factors, plan = np.asarray(img_u8), np.asarray(factors), np.asarray(plan)
    return np.stack([255.0 * chain(img_u8[b], factors[b], plan[b]) for b in range(img_u8.shape[0])])


def assert_matches(out_u8, ref, what=""):
    """the acceptance rule of this module's docstring on a whole launch; prints its figures before it asserts"""
    out = np.asarray(out_u8).astype(np.int64)
    ref = np.clip(np.asarray(ref, dtype=np.float64), 0.0, 255.0)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    lo = np.floor(ref)
    band = np.abs(ref - lo - 0.5) < DELTA
    frac = float(band.mean())
    exact = np.rint(ref).astype(np.int64)  # ties to even
    wrong = np.where(band, (out != lo) & (out != lo + 1), out != exact)
    print(f"color_jitter {what}: {out.size} values, {int(band.sum())} in the +-{DELTA} band ({frac:.4%}), {int(wrong.sum())} wrong, "
          f"max |out - oracle| {float(np.abs(out - ref).max()):.6f}")
    assert frac <= MAX_BAND_FRACTION, f"{what}: {frac:.3%} of the oracle's values lie in the band: the inputs cannot judge the kernel"
    assert not wrong.any(), f"{what}: {int(wrong.sum())} of {out.size} values differ from the oracle, first at {tuple(np.argwhere(wrong)[0])}: " \
                            f"got {out[tuple(np.argwhere(wrong)[0])]}, oracle {ref[tuple(np.argwhere(wrong)[0])]:.6f}"


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def all_orders_case(seed=1, H=9, W=11):
    """48 images of H x W noise: every order of the four steps once without and once with grayscale, every image with factors of its own, none
    dyadic (brightness / contrast / saturation in 0.6-1.4, hue in +-0.1)"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (48, H, W, 3), dtype=np.uint8)
    plan = np.array([make_plan(o, gray) for gray in (False, True) for o in ORDERS], dtype=np.int32)
    factors = np.empty((48, 4), dtype=np.float32)
    factors[:, :3] = 0.6 + 0.8 * (rng.integers(1, 1000, (48, 3)) / 1000.0) + 1e-4 / 3
    factors[:, 3] = -0.1 + 0.2 * (rng.integers(1, 1000, 48) / 1000.0) + 1e-4 / 3
    return img, factors, plan
