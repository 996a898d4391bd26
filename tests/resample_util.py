"""The float64 oracle of ``ocn_resample_u8``, written from the definition in include/openclip_hip.h: per image and axis a window of the source, the
length R of the virtually resized axis and the slice of it that is the output; pixels outside the resized image are the fill colour.  The axis
weights, the acceptance rule (DELTA = 2**-9, at most 2 % of the oracle's values in the band, asserted on the oracle alone) and their derivation are
those of tests/resized_crop_util.py: the arithmetic is the same, tap for tap.  tests/test_resample.py checks this oracle against
``F.interpolate(..., mode="bicubic", antialias=True)`` in float64 before it judges anything."""
import numpy as np

from tests.resized_crop_util import DELTA, MAX_BAND_FRACTION, MAX_RATIO, assert_matches, axis_matrix, cubic  # noqa: F401  (re-exported)

SIZES = [(75, 100), (100, 75), (37, 121), (128, 40), (31, 29), (64, 64), (33, 47), (50, 30), (29, 31), (96, 32), (32, 96), (45, 45)]
MAX_SOURCE, MAX_RESIZED, ALIGN = 8192, 4096, 16


def noise_images(seed, sizes=SIZES):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def pack(images, arena_bytes=None, align=ALIGN):
    """the images one behind the other at multiples of ``align`` -> (arena uint8 [bytes], offsets int64 [B]); the tail of the arena is zero"""
    offsets, off = [], 0
    for im in images:
        offsets.append(off)
        off = (off + im.size + align - 1) // align * align
    arena = np.zeros(off if arena_bytes is None else arena_bytes, dtype=np.uint8)
    for o, im in zip(offsets, images):
        arena[o:o + im.size] = im.reshape(-1)
    return arena, np.asarray(offsets, dtype=np.int64)


def axis_rows(n, R, o, m):
    """float64 [m, n] and bool [m]: row i holds the weights of resized index i + o over the n window positions; False where i + o lies outside [0, R)"""
    W = axis_matrix(n, R)
    r = np.arange(m) + o
    ok = (r >= 0) & (r < R)
    A = np.zeros((m, n), dtype=np.float64)
    A[ok] = W[r[ok]]
    return A, ok


def oracle_window(window, Rh, Rw, oy, ox, size, fill):
    """window: [nh, nw, 3] (any real dtype) -> float64 [Ho, Wo, 3], unrounded and unclamped; fill outside the resized image"""
    Ho, Wo = (size, size) if isinstance(size, int) else size
    c = np.asarray(window, dtype=np.float64)
    Ay, oky = axis_rows(c.shape[0], Rh, oy, Ho)
    Ax, okx = axis_rows(c.shape[1], Rw, ox, Wo)
    rows = np.tensordot(Ay, c, axes=(1, 0))                           # [Ho, nw, 3]
    out = np.tensordot(Ax, rows, axes=(1, 1)).transpose(1, 0, 2)      # [Wo, Ho, 3] -> [Ho, Wo, 3]
    out[~(oky[:, None] & okx[None, :])] = float(fill)
    return out


def oracle(arena, offsets, plan, size, fill=0):
    """arena uint8 [bytes], offsets [B], plan [B, 10] = (Hs, Ws, top, left, nh, nw, Rh, Rw, oy, ox), every window inside its source and every image
    inside the arena -> float64 [B, Ho, Wo, 3]"""
    arena, out = np.asarray(arena), []
    for off, p in zip(np.asarray(offsets).tolist(), np.asarray(plan).tolist()):
        Hs, Ws, top, left, nh, nw, Rh, Rw, oy, ox = p
        assert 0 <= top and 0 <= left and nh > 0 and nw > 0 and top + nh <= Hs and left + nw <= Ws and off >= 0 and off + Hs * Ws * 3 <= arena.size, (off, p)
        assert 1 <= Rh <= MAX_RESIZED and 1 <= Rw <= MAX_RESIZED, p  # (the definition holds at any side ratio; the kernel takes up to MAX_RATIO)
        img = arena[off:off + Hs * Ws * 3].reshape(Hs, Ws, 3)
        out.append(oracle_window(img[top:top + nh, left:left + nw], Rh, Rw, oy, ox, size, fill))
    return np.stack(out)


def oracle_clamped(arena, offsets, plan, size, fill=0):
    """what the kernel documents for offsets and plans the host-side check would refuse: Hs, Ws forced into [1, 8192], Rh, Rw into [1, 4096], a window
    side into [1, min(4 R, 8192)] (anchored at its top-left corner), the corner into +-32768, the output offset into +-4096; every source coordinate
    into the image (the edge pixel repeated); the offset into [0, arena_bytes - 4] and down to a multiple of 4, and every byte address then read into
    [0, arena_bytes)"""
    arena, out = np.asarray(arena), []
    clip = lambda v, lo, hi: min(max(int(v), lo), hi)  # noqa: E731
    for off, p in zip(np.asarray(offsets).tolist(), np.asarray(plan).tolist()):
        Hs, Ws = clip(p[0], 1, MAX_SOURCE), clip(p[1], 1, MAX_SOURCE)
        top, left = clip(p[2], -32768, 32768), clip(p[3], -32768, 32768)
        Rh, Rw = clip(p[6], 1, MAX_RESIZED), clip(p[7], 1, MAX_RESIZED)
        nh, nw = clip(p[4], 1, min(MAX_RATIO * Rh, MAX_SOURCE)), clip(p[5], 1, min(MAX_RATIO * Rw, MAX_SOURCE))
        oy, ox = clip(p[8], -MAX_RESIZED, MAX_RESIZED), clip(p[9], -MAX_RESIZED, MAX_RESIZED)
        off = clip(off, 0, arena.size - 4) & ~3
        rows = np.clip(top + np.arange(nh), 0, Hs - 1)
        cols = np.clip(left + np.arange(nw), 0, Ws - 1)
        addr = off + (rows[:, None, None] * Ws + cols[None, :, None]) * 3 + np.arange(3)[None, None, :]
        out.append(oracle_window(arena[np.clip(addr, 0, arena.size - 1)], Rh, Rw, oy, ox, size, fill))
    return np.stack(out)
