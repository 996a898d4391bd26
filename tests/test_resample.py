"""CPU: the float64 oracle of ``ocn_resample_u8`` is checked against torch before it judges the kernel; the host-side plan builders (the reference's
validation transform and its RandomResizedCrop, per image), the packer and the plan check; the argument checks of ``ops.resample_u8`` (which has no
CPU path) and of the library."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from open_clip_amd import ops
from open_clip_amd.input_pipeline import (DeviceBatchPipeline, check_resample_plan, eval_resample_plan, pack_images, random_resized_crop_boxes,
                                          train_resample_plan)
from tests import resample_util as U

MODES = ("shortest", "longest", "squash")
TARGETS = [32, (24, 40)]
SIZES_T = torch.tensor(U.SIZES)


def _hw(size):
    return (size, size) if isinstance(size, int) else size


@pytest.mark.parametrize("mode", MODES)
def test_oracle_is_torch_antialiased_bicubic_of_the_whole_image_windowed(mode):
    """rows oy .. oy + Ho, columns ox .. ox + Wo of F.interpolate(whole image, (Rh, Rw)) in float64; fill where the slice leaves the resized image"""
    images = U.noise_images(1234)
    arena, offsets = U.pack(images)
    worst = 0.0
    for size in TARGETS:
        Ho, Wo = _hw(size)
        plan = eval_resample_plan(SIZES_T, size, mode).numpy()
        mine = U.oracle(arena, offsets, plan, size, fill=7)
        for b, im in enumerate(images):
            Rh, Rw, oy, ox = (int(v) for v in plan[b, 6:])
            x = torch.from_numpy(im).permute(2, 0, 1)[None].double()
            full = F.interpolate(x, size=(Rh, Rw), mode="bicubic", antialias=True, align_corners=False)[0].permute(1, 2, 0).numpy()
            ref = np.full((Ho, Wo, 3), 7.0)
            y0, y1, x0, x1 = max(0, -oy), min(Ho, Rh - oy), max(0, -ox), min(Wo, Rw - ox)
            ref[y0:y1, x0:x1] = full[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
            worst = max(worst, float(np.abs(mine[b] - ref).max()))
    print(f"oracle vs F.interpolate float64, {mode}: max abs {worst:.3e}")
    assert worst <= 1e-9


def test_oracle_of_a_train_plan_is_the_crop_oracle():
    from tests import resized_crop_util as C
    src = np.random.default_rng(5).integers(0, 256, (3, 40, 52, 3), dtype=np.uint8)
    boxes = [(2, 2, 16, 16), (3, 5, 31, 37), (1, 7, 9, 11)]
    arena, offsets = U.pack(list(src))
    plan = [(40, 52, t, l, h, w, 16, 24, 0, 0) for t, l, h, w in boxes]
    assert np.array_equal(U.oracle(arena, offsets, plan, (16, 24)), C.oracle(src, boxes, (16, 24)))
    assert np.array_equal(U.oracle_clamped(arena, offsets, plan, (16, 24)), U.oracle(arena, offsets, plan, (16, 24)))  # a good plan: nothing to clamp


# ---- the plan rules, restated from the reference (transform.py:171-186, :211-248, :461-492 and torchvision's Resize(int) / CenterCrop) in plain Python ----
def _reference_plan(Hs, Ws, size, mode):
    Ho, Wo = _hw(size)
    if mode == "squash":
        return Ho, Wo, 0, 0
    if mode == "shortest" and Ho == Wo:
        short, long = (Ws, Hs) if Ws <= Hs else (Hs, Ws)
        new_short, new_long = Ho, int(Ho * long / short)
        Rw, Rh = (new_short, new_long) if Ws <= Hs else (new_long, new_short)
    else:
        longest = 1.0 if mode == "longest" else 0.0
        ratio_h, ratio_w = Hs / Ho, Ws / Wo
        ratio = max(ratio_h, ratio_w) * longest + min(ratio_h, ratio_w) * (1. - longest)
        Rh, Rw = (round(x * 1. / ratio) for x in (Hs, Ws))
    off = []
    for R, m in ((Rh, Ho), (Rw, Wo)):
        off.append(-((m - R) // 2) if R < m else int(round((R - m) / 2.0)))
    return Rh, Rw, off[0], off[1]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", TARGETS + [224, (224, 160)])
def test_eval_plan_restates_the_reference_transform(mode, size):
    rng = np.random.default_rng(7)
    sizes = U.SIZES + [(int(h), int(w)) for h, w in rng.integers(20, 700, (200, 2))] + [(375, 500), (500, 375), (333, 500), (1, 9), (224, 224)]
    plan = eval_resample_plan(torch.tensor(sizes), size, mode)
    assert plan.dtype == torch.int32 and tuple(plan.shape) == (len(sizes), 10) and not plan.is_cuda
    for (Hs, Ws), p in zip(sizes, plan.tolist()):
        assert p[:6] == [Hs, Ws, 0, 0, Hs, Ws]  # the filter sees the whole image
        assert tuple(p[6:]) == _reference_plan(Hs, Ws, size, mode), (Hs, Ws, size, mode)
    if mode == "shortest":  # CenterCrop of an image smaller than the target cannot arise
        Ho, Wo = _hw(size)
        assert bool((plan[:, 6] >= Ho).all()) and bool((plan[:, 7] >= Wo).all()) and bool((plan[:, 8:] >= 0).all())


def test_eval_plan_crops_with_an_odd_remainder_round_half_to_even():
    """(R - m) / 2 ends in .5: Python's round goes to the even neighbour, not up.  The twelve sizes give 2 such crops at 32 x 32 and 4 at (24, 40)"""
    for size, count in ((32, 2), ((24, 40), 4)):
        plan = eval_resample_plan(SIZES_T, size, "shortest").long()
        m = torch.tensor(_hw(size))
        odd = ((plan[:, 6:8] - m) % 2 == 1) & (plan[:, 6:8] > m)
        assert int(odd.sum()) == count
        d = (plan[:, 6:8] - m)[odd]
        o = plan[:, 8:10][odd]
        assert bool((o % 2 == 0).all()) and bool(((o - d.double() / 2).abs() == 0.5).all())  # the even one of the two neighbours
    assert eval_resample_plan(torch.tensor([(37, 32)]), 32, "shortest")[0, 6:].tolist() == [37, 32, 2, 0]  # 2.5 -> 2
    assert eval_resample_plan(torch.tensor([(39, 32)]), 32, "shortest")[0, 6:].tolist() == [39, 32, 4, 0]  # 3.5 -> 4
    with pytest.raises(ValueError, match="resize_mode"):
        eval_resample_plan(SIZES_T, 32, "fit")
    with pytest.raises(ValueError, match="empty side"):
        eval_resample_plan(torch.tensor([(4, 0)]), 32)


def test_longest_pads_on_both_sides():
    p = eval_resample_plan(torch.tensor([(75, 100), (128, 40)]), 32, "longest").tolist()
    assert p[0][6:] == [24, 32, -4, 0] and p[1][6:] == [32, 10, 0, -11]  # 8 rows of padding: 4 + 4; 22 columns: 11 + 11
    assert eval_resample_plan(torch.tensor([(31, 100)]), 32, "longest")[0, 6:].tolist() == [10, 32, -11, 0]


@pytest.mark.parametrize("scale,ratio", [((0.9, 1.0), (3 / 4, 4 / 3)), ((0.08, 1.0), (3 / 4, 4 / 3)), ((0.5, 0.6), (0.5, 1.0))])
def test_train_plan_respects_each_images_area_and_ratio(scale, ratio):
    rng = np.random.default_rng(11)
    sizes = torch.tensor(U.SIZES * 20 + [(int(h), int(w)) for h, w in rng.integers(30, 600, (272, 2))])
    B = sizes.shape[0]
    plan = train_resample_plan(sizes, (24, 40), scale, ratio, generator=torch.Generator().manual_seed(3))
    assert plan.dtype == torch.int32 and tuple(plan.shape) == (B, 10) and not plan.is_cuda
    assert torch.equal(plan[:, :2].long(), sizes) and plan[:, 6:].tolist() == [[24, 40, 0, 0]] * B
    Hs, Ws, top, left, h, w = (plan[:, i].double() for i in range(6))
    assert bool((top >= 0).all()) and bool((left >= 0).all()) and bool((top + h <= Hs).all()) and bool((left + w <= Ws).all())
    assert bool((h > 0).all()) and bool((w > 0).all())
    # as tests/test_resized_crop.py: the rounded sides lie within 1/2 of their real values; the requested ranges must meet that square
    area = Hs * Ws
    whole = (h == Hs) & (w == Ws)  # a fallback (no attempt fitted) may be the whole image
    ok_area = ((w - .5) * (h - .5) <= scale[1] * area) & ((w + .5) * (h + .5) >= scale[0] * area)
    ok_ratio = ((w - .5) / (h + .5) <= ratio[1]) & ((w + .5) / (h - .5) >= ratio[0])
    in_range = (Ws / Hs >= ratio[0]) & (Ws / Hs <= ratio[1])
    assert bool((ok_area | ~in_range | whole).all()) and bool((ok_ratio | whole).all())
    assert len({tuple(b) for b in plan[:, 2:6].tolist()}) > B // 4


def test_train_plan_is_reproducible_and_equals_the_box_sampler_on_one_size():
    sizes = torch.tensor(U.SIZES * 4)
    a = train_resample_plan(sizes, 32, generator=torch.Generator().manual_seed(11))
    b = train_resample_plan(sizes, 32, generator=torch.Generator().manual_seed(11))
    c = train_resample_plan(sizes, 32, generator=torch.Generator().manual_seed(12))
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert not torch.equal(train_resample_plan(sizes, 32), train_resample_plan(sizes, 32))  # the global generator moves on
    same = train_resample_plan(torch.tensor([(256, 256)] * 64), 224, generator=torch.Generator().manual_seed(5))
    assert torch.equal(same[:, 2:6], random_resized_crop_boxes(64, 256, 256, generator=torch.Generator().manual_seed(5)))


def test_train_plan_fallback_is_each_images_own_clamped_centre_crop():
    # square boxes of 90-100 % of the area never fit the first two images; the third takes an attempt
    sizes = torch.tensor([(10, 200), (200, 10), (100, 100), (10, 200)])
    plan = train_resample_plan(sizes, 8, scale=(0.9, 1.0), ratio=(1.0, 1.0), generator=torch.Generator().manual_seed(0))
    assert plan[0].tolist() == [10, 200, 0, 95, 10, 10, 8, 8, 0, 0] and plan[1].tolist() == [200, 10, 95, 0, 10, 10, 8, 8, 0, 0]
    assert plan[3].tolist() == plan[0].tolist()
    assert 94 <= int(plan[2, 4]) <= 100 and int(plan[2, 4]) == int(plan[2, 5])
    # in-range source ratios, an area no attempt can fit: each image's whole self
    plan = train_resample_plan(torch.tensor([(10, 12), (30, 27)]), 8, scale=(4.0, 5.0))
    assert plan[:, 2:6].tolist() == [[0, 0, 10, 12], [0, 0, 30, 27]]


def test_train_plan_and_box_sampler_agree_on_the_fallback():
    """scale = (4, 4): no attempt fits, every image takes the fallback -- narrow, wide and in range, the by-hand centre crops of
    tests/test_resized_crop.py (round(40 * 4 / 3) = 53 of the 200 rows, round(40 / (3 / 4)) = 53 of the 200 columns), from both entries of the one sampler"""
    by_hand = {(40, 200): [0, 73, 40, 53], (200, 40): [73, 0, 53, 40], (64, 64): [0, 0, 64, 64]}
    for (Hs, Ws), box in by_hand.items():
        boxes = random_resized_crop_boxes(3, Hs, Ws, scale=(4.0, 4.0), generator=torch.Generator().manual_seed(13))
        plan = train_resample_plan(torch.tensor([(Hs, Ws)] * 3), 32, scale=(4.0, 4.0), generator=torch.Generator().manual_seed(13))
        assert boxes.dtype == torch.int32 and boxes.tolist() == [box] * 3 and torch.equal(plan[:, 2:6], boxes)
    mixed = train_resample_plan(torch.tensor(list(by_hand)), 32, scale=(4.0, 4.0), generator=torch.Generator().manual_seed(13))
    assert mixed[:, 2:6].tolist() == list(by_hand.values())


GOOD = [40, 52, 2, 3, 32, 32, 8, 8, 0, 0]


@pytest.mark.parametrize("change,offset,what", [
    ({4: 0}, 16, "empty window"), ({5: -1}, 16, "empty window"), ({2: -1}, 16, "lies outside its source"), ({3: 21}, 16, "lies outside its source"),
    ({2: 9}, 16, "lies outside its source"), ({6: 0}, 16, "resized side outside"), ({7: 4097, 5: 8}, 16, "resized side outside"),
    ({4: 33}, 16, r"more than 4 x its resized side: the loader must reduce such an image first \(for instance with PIL's Image.draft"),
    ({0: 0, 4: 1, 2: 0}, 16, "source side outside"), ({1: 8193}, 16, "source side outside"), ({8: 5000}, 16, "output offset beyond"),
    ({}, 24, "no multiple of 16"), ({}, -16, "negative"), ({}, 10000 - 6240 + 16, "does not fit the arena of 10000 bytes")])
def test_check_resample_plan_raises_on_each_bad_form(change, offset, what):
    good = torch.tensor([GOOD, GOOD], dtype=torch.int32)
    check_resample_plan(good, torch.tensor([0, 6240]), 12480, 8)
    check_resample_plan(torch.tensor([[40, 52, 0, 0, 40, 52, 10, 13, -3, 2]], dtype=torch.int32), torch.tensor([3760]), 10000, (10, 13))  # exactly 4x, flush
    bad = good.clone()
    for k, v in change.items():
        bad[1, k] = v
    with pytest.raises(ValueError, match=r"check_resample_plan: image 1 \(plan .*" + what):
        check_resample_plan(bad, torch.tensor([0, offset]), 10000, 8)
    with pytest.raises(ValueError, match="expected an integer plan"):
        check_resample_plan(torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, dtype=torch.int64), 10000, 8)
    with pytest.raises(ValueError, match="expected an integer plan"):
        check_resample_plan(torch.zeros(2, 10), torch.zeros(2, dtype=torch.int64), 10000, 8)
    with pytest.raises(ValueError, match="expected integer offsets"):
        check_resample_plan(good, torch.zeros(3, dtype=torch.int64), 10000, 8)


def test_pack_images_aligns_and_refuses_an_overflow():
    images = U.noise_images(3)[:5]  # 22500, 22500, 13431, 15360, 2697 bytes
    want_arena, want_offsets = U.pack(images)
    arena, offsets = torch.full((want_arena.size + 64,), 9, dtype=torch.uint8), torch.zeros(5, dtype=torch.int64)
    used = pack_images([images[0], torch.from_numpy(images[1])] + images[2:], arena, offsets)  # arrays and tensors alike
    assert used == want_arena.size and used % 16 == 0 and offsets.tolist() == want_offsets.tolist() and all(o % 16 == 0 for o in offsets.tolist())
    for o, im in zip(offsets.tolist(), images):
        assert np.array_equal(arena[o:o + im.size].numpy().reshape(im.shape), im)
    assert bool((arena[used:] == 9).all())  # nothing behind the used prefix is touched
    assert offsets.tolist() == [0, 22512, 45024, 58464, 73824]  # 22500 bytes: the next image starts 12 bytes later; 13431: 9 bytes later
    exact = torch.zeros(want_offsets[-1] + images[-1].size, dtype=torch.uint8)  # the last image ends with the arena: used = the arena's size
    assert pack_images(images, exact, offsets) == exact.numel()
    with pytest.raises(ValueError, match=r"pack_images: image 4 \(31 x 29, 2697 bytes at offset 73824\) does not fit the arena of 76520 bytes"):
        pack_images(images, torch.zeros(exact.numel() - 1, dtype=torch.uint8), offsets)
    with pytest.raises(ValueError, match=r"pack_images: image 1 must be a host uint8 \[Hs, Ws, 3\]"):
        pack_images([images[0], images[1].astype(np.float32)], arena, offsets[:2])
    with pytest.raises(ValueError, match=r"pack_images: image 0 must be a host uint8 \[Hs, Ws, 3\]"):
        pack_images([images[0].transpose(2, 0, 1)], arena, offsets[:1])  # CHW
    with pytest.raises(ValueError, match="offsets_out must be host int64"):
        pack_images(images, arena, offsets[:4])


def test_op_refuses_what_it_cannot_run():
    arena = torch.zeros(1024, dtype=torch.uint8)
    offsets, plan = torch.tensor([0, 512]), torch.tensor([[8, 8, 0, 0, 8, 8, 4, 4, 0, 0]] * 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.resample_u8(arena, offsets, plan, 4)
    with pytest.raises(RuntimeError, match="'arena' must be uint8"):
        ops.resample_u8(arena.float(), offsets, plan, 4)
    with pytest.raises(RuntimeError, match="'arena' must be a flat byte buffer"):
        ops.resample_u8(arena.view(2, 512), offsets, plan, 4)
    with pytest.raises(RuntimeError, match="'arena' must be a flat byte buffer"):
        ops.resample_u8(arena[:1022], offsets, plan, 4)
    with pytest.raises(RuntimeError, match=r"'plan' must be int32 \[B = 2, 10\]"):
        ops.resample_u8(arena, offsets, plan[:1], 4)
    with pytest.raises(RuntimeError, match=r"'plan' must be int32 \[B = 2, 10\]"):
        ops.resample_u8(arena, offsets, plan[:, :4], 4)
    with pytest.raises(RuntimeError, match=r"'offsets' must be int64 \[B\]"):
        ops.resample_u8(arena, offsets.view(2, 1), plan, 4)
    for fill in (-1, 256, 1.5, True):
        with pytest.raises(RuntimeError, match="'fill' must be an int in"):
            ops.resample_u8(arena, offsets, plan, 4, fill=fill)


def test_ragged_pipeline_refuses_bilinear_by_name():
    # refused before anything touches a device
    with pytest.raises(NotImplementedError, match="interpolation='bilinear' is not implemented"):
        DeviceBatchPipeline.ragged("cuda:0", 4, (4, 16), 32, 1 << 20, interpolation="bilinear")
    with pytest.raises(ValueError, match="interpolation must be"):
        DeviceBatchPipeline.ragged("cuda:0", 4, (4, 16), 32, 1 << 20, interpolation="nearest")
    with pytest.raises(ValueError, match="resize_mode must be"):
        DeviceBatchPipeline.ragged("cuda:0", 4, (4, 16), 32, 1 << 20, resize_mode="fit")
    with pytest.raises(ValueError, match="arena_bytes must be a positive multiple of 16"):
        DeviceBatchPipeline.ragged("cuda:0", 4, (4, 16), 32, (1 << 20) + 4)
    with pytest.raises(ValueError, match="fill_color must be an int"):
        DeviceBatchPipeline.ragged("cuda:0", 4, (4, 16), 32, 1 << 20, fill_color=(0, 0, 0))


def test_library_refuses_sizes_outside_its_limits_before_any_launch():
    """host-side argument checks: safe without a GPU (fake, never dereferenced device pointers)"""
    from open_clip_amd import _lib, build
    build.build()
    p = 4096  # arena, arena_bytes, offsets, plan, B, out, Ho, Wo, fill, stream
    for args, msg in (((p, 64, p, p, 1, p, 0, 4, 0, 0), "bad output shape"), ((p, 64, p, p, 1, p, 4, 1025, 0, 0), "bad output shape"),
                      ((p, 64, p, p, 1, p, 1025, 4, 0, 0), "bad output shape"), ((p, 64, p, p, 0, p, 4, 4, 0, 0), "bad output shape"),
                      ((p, 64, p, p, 1, p, 4, 4, 256, 0), r"fill=256 must lie in \[0, 255\]"), ((p, 64, p, p, 1, p, 4, 4, -1, 0), r"fill=-1 must lie in"),
                      ((0, 64, p, p, 1, p, 4, 4, 0, 0), "null operand"), ((p, 64, 0, p, 1, p, 4, 4, 0, 0), "null operand"),
                      ((p, 64, p, 0, 1, p, 4, 4, 0, 0), "null operand"), ((p, 64, p, p, 1, 0, 4, 4, 0, 0), "null operand"),
                      ((p + 8, 64, p, p, 1, p, 4, 4, 0, 0), "the arena must be 16-byte aligned"), ((p, 62, p, p, 1, p, 4, 4, 0, 0), "arena_bytes=62 must be"),
                      ((p, 0, p, p, 1, p, 4, 4, 0, 0), "arena_bytes=0 must be"), ((p, 64, p + 4, p, 1, p, 4, 4, 0, 0), "offsets must be 8-byte aligned"),
                      ((p, 64, p, p + 2, 1, p, 4, 4, 0, 0), "plan must be 4-byte aligned")):
        with pytest.raises(RuntimeError, match=r"ocn_resample_u8 failed \(-1\): ocn_resample_u8: " + msg):
            _lib.call("ocn_resample_u8", *args)
