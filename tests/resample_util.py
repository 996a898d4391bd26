"""The float64 oracle of ``ocn_resample_u8``, written from the definition in include/openclip_hip.h: per image and axis a window of the source, the
length R of the virtually resized axis and the slice of it that is the output; pixels outside the resized image are the fill colour.  The axis
weights, the acceptance rule (DELTA = 2**-9, at most 2 % of the oracle's values in the band, asserted on the oracle alone) and their derivation are
those of tests/resized_crop_util.py: the arithmetic is the same, tap for tap.  tests/test_resample.py checks this oracle against
``F.interpolate(..., mode="bicubic", antialias=True)`` in float64 before it judges anything.

``golden_cases()`` are the inputs whose outputs tests/golden/resample_parent.npz records, once, from the library of the commit BEFORE the two kernels
became one routine (tools/resample_golden.py writes the file): the new library must give the same bytes."""
import os

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


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample_parent.npz")
SIX_BOXES = [(2, 2, 16, 16), (0, 0, 40, 52), (3, 5, 31, 37), (1, 7, 9, 11), (24, 36, 16, 16), (7, 9, 1, 1)]


def last_in_the_arena_case():
    """two noise images, the second with rows of 132 bytes (every row starts on a dword), flush with the arena's end, and a tile column of it whose
    span starts at byte 9 of a row: ragged + aligned rows + a span shifted by 1 + the arena-end clamp -> (arena, offsets, plan, size)"""
    rng = np.random.default_rng(31)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((31, 29), (20, 44))]
    arena, offsets = pack(images)
    assert arena.size == 5344 and offsets.tolist() == [0, 2704] and offsets[1] + 20 * 132 == arena.size
    plan = np.asarray([(31, 29, 2, 1, 27, 26, 17, 33, 0, 0), (20, 44, 1, 3, 19, 41, 17, 33, 0, 0)], dtype=np.int32)
    return arena, offsets, plan, (17, 33)


def golden_cases():
    """the inputs of the existing GPU tests, rebuilt from their seeds as numpy arrays: a list of dicts with 'name', 'size' and either 'src' uint8
    [B, Hs, Ws, 3], 'boxes' int32 [B, 4] and 'shift' (the bytes src starts into its allocation) for ``ops.resized_crop_u8``, or 'arena', 'offsets',
    'plan' and 'fill' for ``ops.resample_u8``"""
    import torch
    from open_clip_amd.input_pipeline import eval_resample_plan, train_resample_plan

    def crop(name, shape, seed, boxes, size, shift=0):
        src = np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)
        return {"name": name, "src": src, "boxes": np.asarray(boxes, dtype=np.int32), "size": size, "shift": shift}

    def ragged(name, arena, offsets, plan, size, fill):
        return {"name": name, "arena": arena, "offsets": np.asarray(offsets, dtype=np.int64), "plan": np.asarray(plan, dtype=np.int32), "size": size, "fill": fill}

    cases = [crop("crop_six_boxes", (6, 40, 52, 3), 1, SIX_BOXES, 16),
             crop("crop_70x70_to_23x16", (2, 70, 70, 3), 2, [(3, 5, 64, 64), (6, 0, 64, 64)], (23, 16)),
             crop("crop_tile_edge_17x33", (2, 40, 52, 3), 3, [(0, 0, 40, 52), (5, 4, 30, 41)], (17, 33)),
             crop("crop_bad_boxes", (3, 40, 52, 3), 6, [(-5, -4, 20, 24), (2, 1, 30, 45), (20, 30, 28, 25)], (12, 8)),
             crop("crop_src_one_byte_in", (2, 40, 52, 3), 7, [(0, 0, 40, 52), (3, 5, 31, 37)], (16, 20), shift=1)]
    sizes = torch.tensor(SIZES)
    arena, offsets = pack(noise_images(1234))
    for mode in ("shortest", "longest", "squash"):
        cases.append(ragged(f"ragged_eval_{mode}_to_32", arena, offsets, eval_resample_plan(sizes, 32, mode).numpy(), 32, 7))
    plan = train_resample_plan(sizes, 32, scale=(0.3, 1.0), generator=torch.Generator().manual_seed(2)).numpy().copy()
    for b, box in {0: (3, 5, 32, 32), 1: (7, 9, 1, 1), 2: (37 - 32, 121 - 32, 32, 32), 3: (128 - 56, 40 - 36, 56, 36), 4: (1, 7, 9, 11)}.items():
        plan[b, 2:6] = box
    cases.append(ragged("ragged_train_plans", arena, offsets, plan, 32, 0))
    plan, offs = bad_plans(offsets)
    cases.append(ragged("ragged_bad_plans", arena, offs, plan, 32, 7))
    a2, o2, p2, size = last_in_the_arena_case()
    cases.append(ragged("ragged_aligned_rows_last_in_the_arena", a2, o2, p2, size, 0))
    return cases


def bad_plans(offsets):
    """plans and offsets of the twelve SIZES images that the host-side check refuses (five of them) -> (plan int32 [12, 10], offsets int64 [12])"""
    import torch
    from open_clip_amd.input_pipeline import eval_resample_plan
    plan = eval_resample_plan(torch.tensor(SIZES), 32, "shortest").numpy().copy()
    offs = np.asarray(offsets).copy()
    plan[0, 2] = -3                                    # top = -3: the first row repeated (image 0 lies first: above it is the sentinel)
    plan[11, 0] += 2; plan[11, 4] += 2                 # noqa: E702  Hs two rows more than stored, in the LAST image: its end runs past the arena
    plan[5, 0] += 2; plan[5, 4] += 2                   # noqa: E702  ... and in one in the middle: the two rows are the next image's first bytes
    offs[10] = offsets[11] + 4096                      # an offset 4096 bytes past the last image: beyond the arena's end
    plan[6, 6] = 0                                     # R = 0: resampled as R = 1
    plan[7, 4] = 5 * plan[7, 6]                        # n = 5 R: resampled as n = 4 R (the rows below the source: its last row repeated)
    return plan, offs


def run_golden_case(case, dev):
    """one case of ``golden_cases()`` through ``ops`` on device ``dev`` -> uint8 numpy [B, Ho, Wo, 3]"""
    import torch
    from open_clip_amd import ops
    if "src" in case:
        src = torch.from_numpy(case["src"])
        buf = torch.zeros(src.numel() + case["shift"], dtype=torch.uint8, device=dev)
        view = buf[case["shift"]:].view(src.shape)
        view.copy_(src)
        return ops.resized_crop_u8(view, torch.from_numpy(case["boxes"]).to(dev), case["size"]).cpu().numpy()
    return ops.resample_u8(torch.from_numpy(case["arena"]).to(dev), torch.from_numpy(case["offsets"]).to(dev), torch.from_numpy(case["plan"]).to(dev),
                           case["size"], fill=case["fill"]).cpu().numpy()
