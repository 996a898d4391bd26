"""CPU: the float64 oracle of the device-side RandomResizedCrop is checked against torch before it judges the kernel; the host-side box sampler and
box check; the argument checks of ``ops.resized_crop_u8`` (which has no CPU path)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from open_clip_amd import ops
from open_clip_amd.input_pipeline import check_boxes, random_resized_crop_boxes
from tests import resized_crop_util as U


# (crop height, crop width, output): down, up, anisotropic (one axis up, one down), the 4x limit, identity
ORACLE_CASES = [(31, 37, (16, 16)), (9, 11, (16, 16)), (40, 13, (16, 24)), (64, 45, (23, 16)), (16, 16, (16, 16)), (243, 250, (224, 224))]


@pytest.mark.parametrize("h,w,size", ORACLE_CASES)
def test_oracle_is_torch_antialiased_bicubic_in_float64(h, w, size):
    rng = np.random.default_rng(h * 1000 + w)
    crop = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    mine = U.oracle_crop(crop, size)
    x = torch.from_numpy(crop).permute(2, 0, 1)[None].double()
    ref = F.interpolate(x, size=size, mode="bicubic", antialias=True, align_corners=False)[0].permute(1, 2, 0).numpy()
    err = float(np.abs(mine - ref).max())
    print(f"oracle vs F.interpolate float64, {h}x{w} -> {size}: max abs {err:.3e}")
    assert err <= 1e-9


def test_oracle_tap_counts_and_identity():
    assert max(U.tap_counts(64, 16)) == 16 and max(U.tap_counts(64, 23)) <= 17  # a side of 4x the output: the kernel's largest tap count
    assert max(U.tap_counts(40, 16)) == 10 and max(U.tap_counts(52, 16)) == 13
    assert np.array_equal(U.axis_matrix(16, 16), np.eye(16))  # scale 1: the cubic is exactly 0 at +-1 and +-2, 1 at 0
    assert np.array_equal(U.axis_matrix(1, 16), np.ones((16, 1)))


def test_acceptance_rule_rejects_a_wrong_level_and_a_useless_input():
    ref = np.array([[10.2, 11.5 + 2.0 ** -11, 300.0, -4.0]] * 50)
    ok = np.array([[10, 11, 255, 0]] * 50)
    with pytest.raises(AssertionError, match="lie in the band"):
        U.assert_matches(ok, ref)  # a quarter of the values in the band: refused whatever the output
    ref = np.concatenate([np.full((199, 4), 10.2), ref[:1]])  # now 1 of 800
    for v, good in ((11, True), (12, True), (10, False), (13, False)):
        out = np.concatenate([np.full((199, 4), 10), [[10, v, 255, 0]]])
        if good:
            U.assert_matches(out, ref)
        else:
            with pytest.raises(AssertionError, match="differ from the oracle"):
                U.assert_matches(out, ref)
    out = np.concatenate([np.full((199, 4), 10), [[11, 12, 255, 0]]])  # 10.2 -> 11 outside the band
    with pytest.raises(AssertionError, match="differ from the oracle"):
        U.assert_matches(out, ref)


@pytest.mark.parametrize("Hs,Ws,scale,ratio", [(256, 256, (0.9, 1.0), (3 / 4, 4 / 3)), (40, 52, (0.08, 1.0), (3 / 4, 4 / 3)), (300, 200, (0.5, 0.6), (0.5, 1.0))])
def test_random_boxes_respect_source_area_and_ratio(Hs, Ws, scale, ratio):
    B = 512
    boxes = random_resized_crop_boxes(B, Hs, Ws, scale, ratio, generator=torch.Generator().manual_seed(3))
    assert boxes.dtype == torch.int32 and tuple(boxes.shape) == (B, 4) and not boxes.is_cuda
    check_boxes(boxes, Hs, Ws, (max(1, -(-Hs // 4)), max(1, -(-Ws // 4))))  # inside the source, not empty (and within 4x of this output size)
    top, left, h, w = (boxes[:, i].double() for i in range(4))
    # w = round(sqrt(area * r)), h = round(sqrt(area / r)): each side is within 1/2 of its real value, so the real (w, h) lies in the square
    # [w - 1/2, w + 1/2] x [h - 1/2, h + 1/2]: the requested ranges must meet that square's range of w * h and of w / h
    area = Hs * Ws
    assert bool(((w - .5) * (h - .5) <= scale[1] * area).all()) and bool(((w + .5) * (h + .5) >= scale[0] * area).all())
    assert bool(((w - .5) / (h + .5) <= ratio[1]).all()) and bool(((w + .5) / (h - .5) >= ratio[0]).all())
    assert len({tuple(b) for b in boxes.tolist()}) > B // 4  # they do differ from image to image
    assert int(top.min()) >= 0 and int((top + h).max()) <= Hs and int(left.min()) >= 0 and int((left + w).max()) <= Ws


def test_random_boxes_reproducible_under_a_generator():
    a = random_resized_crop_boxes(64, 256, 256, generator=torch.Generator().manual_seed(11))
    b = random_resized_crop_boxes(64, 256, 256, generator=torch.Generator().manual_seed(11))
    c = random_resized_crop_boxes(64, 256, 256, generator=torch.Generator().manual_seed(12))
    assert torch.equal(a, b) and not torch.equal(a, c)
    d, e = random_resized_crop_boxes(64, 256, 256), random_resized_crop_boxes(64, 256, 256)  # the global generator moves on
    assert not torch.equal(d, e)


def test_random_boxes_fallback_is_the_clamped_centre_crop():
    # a 10 x 200 source, square boxes of 90-100 % of its area: a side of about 44 never fits the 10 rows
    boxes = random_resized_crop_boxes(5, 10, 200, scale=(0.9, 1.0), ratio=(1.0, 1.0), generator=torch.Generator().manual_seed(0))
    assert boxes.tolist() == [[0, 95, 10, 10]] * 5
    boxes = random_resized_crop_boxes(3, 200, 10, scale=(0.9, 1.0), ratio=(1.0, 1.0))
    assert boxes.tolist() == [[95, 0, 10, 10]] * 3
    # in-range source ratio: the whole image
    boxes = random_resized_crop_boxes(2, 10, 12, scale=(4.0, 5.0), ratio=(3 / 4, 4 / 3))
    assert boxes.tolist() == [[0, 0, 10, 12]] * 2


@pytest.mark.parametrize("box,what", [((0, 0, 0, 8), "is empty"), ((0, 0, 8, -1), "is empty"), ((-1, 0, 8, 8), "lies outside"), ((0, 45, 8, 8), "lies outside"),
                                      ((33, 0, 8, 8), "lies outside"), ((0, 0, 40, 52), "more than 4 x"), ((0, 0, 33, 8), "more than 4 x")])
def test_check_boxes_raises_on_each_bad_form(box, what):
    good = [2, 3, 32, 32]
    check_boxes(torch.tensor([good, good], dtype=torch.int32), 40, 52, 8)
    check_boxes(torch.tensor([[0, 0, 40, 52]], dtype=torch.int32), 40, 52, (10, 13))  # exactly 4x and flush with every edge
    with pytest.raises(ValueError, match=r"box 1 = .*" + what):
        check_boxes(torch.tensor([good, list(box)], dtype=torch.int32), 40, 52, 8)
    with pytest.raises(ValueError, match="expected integer boxes"):
        check_boxes(torch.zeros(2, 3, dtype=torch.int32), 40, 52, 8)
    with pytest.raises(ValueError, match="expected integer boxes"):
        check_boxes(torch.zeros(2, 4), 40, 52, 8)


def test_op_refuses_what_it_cannot_run():
    src = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    boxes = torch.tensor([[0, 0, 8, 8]] * 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.resized_crop_u8(src, boxes, 4)
    with pytest.raises(RuntimeError, match="'src' must be uint8"):
        ops.resized_crop_u8(src.float(), boxes, 4)
    with pytest.raises(RuntimeError, match=r"'src' must be \[B, Hs, Ws, 3\]"):
        ops.resized_crop_u8(src.permute(0, 3, 1, 2).contiguous(), boxes, 4)  # CHW
    with pytest.raises(RuntimeError, match=r"'src' must be \[B, Hs, Ws, 3\]"):
        ops.resized_crop_u8(src[0], boxes, 4)
    with pytest.raises(RuntimeError, match=r"'boxes' must be int32 \[B = 2, 4\]"):
        ops.resized_crop_u8(src, boxes[:1], 4)
    with pytest.raises(RuntimeError, match=r"'boxes' must be int32 \[B = 2, 4\]"):
        ops.resized_crop_u8(src, boxes.reshape(-1), 4)


def test_library_refuses_sizes_outside_its_limits_before_any_launch():
    """host-side argument checks: safe without a GPU (fake, never dereferenced device pointers)"""
    from open_clip_amd import _lib, build
    build.build()
    p = 4096
    for args, msg in (((p, 1, 8, 8, p, p, 0, 4, 0), "bad output shape"), ((p, 1, 8, 8, p, p, 4, 1025, 0), "bad output shape"),
                      ((p, 0, 8, 8, p, p, 4, 4, 0), "bad output shape"), ((p, 1, 8193, 8, p, p, 4, 4, 0), "bad source shape"),
                      ((p, 1, 8, 0, p, p, 4, 4, 0), "bad source shape"), ((0, 1, 8, 8, p, p, 4, 4, 0), "null operand"),
                      ((p, 1, 8, 8, 0, p, 4, 4, 0), "null operand"), ((p, 1, 8, 8, p, 0, 4, 4, 0), "null operand"),
                      ((p, 1, 8, 8, p + 2, p, 4, 4, 0), "boxes must be 4-byte aligned")):
        with pytest.raises(RuntimeError, match=r"ocn_resized_crop_u8 failed \(-1\): ocn_resized_crop_u8: " + msg):
            _lib.call("ocn_resized_crop_u8", *args)
