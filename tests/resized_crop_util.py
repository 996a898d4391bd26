"""The float64 oracle of ``ocn_resized_crop_u8`` and the rule by which an output is judged against it.  Written from the definition in
include/openclip_hip.h (crop, then antialiased bicubic resize, rounded once); tests/test_resized_crop.py checks it against
``F.interpolate(..., mode="bicubic", antialias=True)`` in float64 before it judges anything.

The acceptance rule, DELTA = 2**-9: an output value must equal round(clamp(oracle, 0, 255)) wherever the oracle's fractional part is at least DELTA
away from .5; inside that band either neighbour is accepted.  Where DELTA comes from: sum |wy| |wx| * 255 is at most about 430 (the negative lobes
make sum |w| about 1.3 per axis); a 17 + 17 tap chain has about 40 fp32 roundings of 2**-24 relative, plus the fp32 rounding of the weights:
together about 1e-3 < 2**-9 (fp32 against fp64 measures 3.3e-5 for 8 x 10 taps).  The band must not be able to hide a failure, so every comparison
also asserts, on the oracle alone, that at most MAX_BAND_FRACTION of its values lie inside it."""
import numpy as np

DELTA = 2.0 ** -9
MAX_BAND_FRACTION = 0.02
MAX_RATIO = 4  # a box side above MAX_RATIO x the output side is clamped by the kernel


def cubic(x):
    """Keys' cubic convolution kernel with a = -0.5"""
    x = np.abs(np.asarray(x, dtype=np.float64))
    return np.where(x < 1.0, (1.5 * x - 2.5) * x * x + 1.0, np.where(x < 2.0, ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0, 0.0))


def axis_matrix(n, m):
    """float64 [m, n]: row o holds the normalised weights of output index o over the n input positions"""
    scale = n / m
    support = 2.0 * max(scale, 1.0)
    inv = 1.0 / max(scale, 1.0)
    W = np.zeros((m, n), dtype=np.float64)
    for o in range(m):
        center = scale * (o + 0.5)
        lo = max(0, int(center - support + 0.5))
        hi = min(n, int(center + support + 0.5))
        k = np.arange(lo, hi)
        w = cubic((k - center + 0.5) * inv)
        W[o, lo:hi] = w / w.sum()
    return W


def tap_counts(n, m):
    W = axis_matrix(n, m)
    return [int(np.count_nonzero(W[o])) for o in range(m)]


def oracle_crop(crop, size):
    """crop: [h, w, 3] (any real dtype) -> float64 [Ho, Wo, 3], unrounded and unclamped"""
    Ho, Wo = (size, size) if isinstance(size, int) else size
    c = np.asarray(crop, dtype=np.float64)
    rows = np.tensordot(axis_matrix(c.shape[0], Ho), c, axes=(1, 0))           # [Ho, w, 3]
    return np.tensordot(axis_matrix(c.shape[1], Wo), rows, axes=(1, 1)).transpose(1, 0, 2)  # [Wo, Ho, 3] -> [Ho, Wo, 3]


def oracle(src, boxes, size):
    """src uint8 [B, Hs, Ws, 3], boxes [B, 4] = (top, left, height, width), every box inside its source -> float64 [B, Ho, Wo, 3]"""
    src, boxes = np.asarray(src), np.asarray(boxes)
    out = []
    for b in range(src.shape[0]):
        t, l, h, w = (int(v) for v in boxes[b])
        assert 0 <= t and 0 <= l and h > 0 and w > 0 and t + h <= src.shape[1] and l + w <= src.shape[2], (t, l, h, w)
        out.append(oracle_crop(src[b, t:t + h, l:l + w], size))
    return np.stack(out)


def oracle_clamped(src, boxes, size):
    """what the kernel documents for a box the host-side check would refuse: a side is forced into [1, MAX_RATIO * output side] (anchored at the
    top-left corner) and every source coordinate into the image (the edge pixel repeated)"""
    Ho, Wo = (size, size) if isinstance(size, int) else size
    src, boxes = np.asarray(src), np.asarray(boxes)
    out = []
    for b in range(src.shape[0]):
        t, l, h, w = (int(v) for v in boxes[b])
        h, w = min(max(h, 1), MAX_RATIO * Ho), min(max(w, 1), MAX_RATIO * Wo)
        rows = np.clip(t + np.arange(h), 0, src.shape[1] - 1)
        cols = np.clip(l + np.arange(w), 0, src.shape[2] - 1)
        out.append(oracle_crop(src[b][rows][:, cols], size))
    return np.stack(out)


def assert_matches(out_u8, ref, what=""):
    """the acceptance rule of this module's docstring; prints its figures before it asserts"""
    out = np.asarray(out_u8).astype(np.int64)
    ref = np.clip(np.asarray(ref, dtype=np.float64), 0.0, 255.0)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    lo = np.floor(ref)
    band = np.abs(ref - lo - 0.5) < DELTA
    frac = float(band.mean())
    exact = np.rint(ref).astype(np.int64)  # ties to even
    wrong = np.where(band, (out != lo) & (out != lo + 1), out != exact)
    print(f"resized_crop {what}: {out.size} values, {int(band.sum())} in the +-{DELTA} band ({frac:.4%}), {int(wrong.sum())} wrong, "
          f"max |out - oracle| {float(np.abs(out - ref).max()):.6f}")
    assert frac <= MAX_BAND_FRACTION, f"{what}: {frac:.3%} of the oracle's values lie in the band: the inputs cannot judge the kernel"
    assert not wrong.any(), f"{what}: {int(wrong.sum())} of {out.size} values differ from the oracle, first at {tuple(np.argwhere(wrong)[0])}: " \
                            f"got {out[tuple(np.argwhere(wrong)[0])]}, oracle {ref[tuple(np.argwhere(wrong)[0])]:.6f}"
