"""GPU: ``ocn_color_jitter_u8`` against the float64 oracle of tests/color_jitter_util.py (acceptance rule and its derivation there), at the smallest
shapes at which the kernel can still go wrong, and ``DeviceBatchPipeline(color_jitter_prob=..., gray_scale_prob=...)`` around it."""
import numpy as np
import pytest
import torch

from open_clip_amd import ops
from open_clip_amd.input_pipeline import JITTER_GRAY_BIT, DeviceBatchPipeline, color_jitter_plan, random_resized_crop_boxes
from tests import color_jitter_util as U

pytestmark = pytest.mark.gpu

CJ = (0.4, 0.4, 0.4, 0.1)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _run(img, factors, plan, dev, **kw):
    img = torch.as_tensor(img)
    out = ops.color_jitter_u8(img.to(dev), torch.as_tensor(np.asarray(factors, dtype=np.float32)).to(dev),
                              torch.as_tensor(np.asarray(plan, dtype=np.int32)).to(dev), **kw)
    assert out.dtype == torch.uint8 and out.shape == img.shape
    return out.cpu().numpy()


def test_all_24_orders_in_one_launch(dev):
    """48 images of 9 x 11 noise, 297 bytes each: the images start at all four byte alignments (single pixels in front of the 4-pixel groups) and their
    99 pixels leave a tail behind the groups.  Every order once without and once with grayscale, every image with factors of its own"""
    img, factors, plan = U.all_orders_case()
    assert len({int(p) for p in plan}) == 48 and len({tuple(f) for f in factors.tolist()}) == 48
    out = _run(img, factors, plan, dev)
    U.assert_matches(out, U.oracle(img, factors, plan), "24 orders x {colour, gray}")
    assert (out[24:, ..., 0] == out[24:, ..., 1]).all() and (out[24:, ..., 0] == out[24:, ..., 2]).all()  # grayscale: one rounding of one value


def test_absent_steps_and_untouched_images(dev):
    """plans with one, two and three steps, holes in front of and between the steps, codes above 4 (treated as nothing), grayscale alone, and plan 0:
    an untouched image is a bit-identical copy"""
    img = U.noise((10, 9, 11, 3), 2)
    plan = [0, U.make_plan([U.HUE]), U.make_plan([U.CONTRAST, U.BRIGHTNESS]), U.make_plan([U.SATURATION, U.HUE, U.CONTRAST]), U.make_plan([], True),
            U.make_plan([U.BRIGHTNESS]), U.make_plan([0, U.CONTRAST, 0, U.SATURATION]), U.make_plan([7, 5, 6]), U.make_plan([U.SATURATION], True), 0]
    factors = np.array([[1.3, 0.7, 1.2, 0.07]] * 10, dtype=np.float32) + 0.011 * np.arange(10, dtype=np.float32)[:, None]
    out = _run(img, factors, plan, dev)
    U.assert_matches(out, U.oracle(img, factors, plan), "partial plans")
    for b in (0, 7, 9):
        assert np.array_equal(out[b], img[b]), b
    assert not np.array_equal(out[4], img[4]) and (out[4][..., 0] == out[4][..., 2]).all()


def test_the_clamp_between_steps(dev):
    """brightness 1.9 then contrast 0.3 (on noise), saturation 1.8 then brightness 0.5 (on noise in 60..199: a channel that saturation clamps to 1 comes
    out at exactly 127.5, inside the band by construction, so the image is chosen to clamp few of them -- and still enough to be seen)"""
    img = U.noise((2, 12, 13, 3), 4)
    img[1] = np.random.default_rng(0).integers(60, 200, (12, 13, 3), dtype=np.uint8)
    plan = [U.make_plan([U.BRIGHTNESS, U.CONTRAST]), U.make_plan([U.SATURATION, U.BRIGHTNESS])]
    factors = np.array([[1.9, 0.3, 1.0, 0.0], [0.5, 1.0, 1.8, 0.0]], dtype=np.float32)
    ref = U.oracle(img, factors, plan)
    for b in range(2):  # the test does see the clamp
        unclamped = np.clip(255.0 * U.chain(img[b], factors[b], plan[b], clamp_steps=False), 0.0, 255.0)
        assert np.abs(unclamped - ref[b]).max() > 10, b
    U.assert_matches(_run(img, factors, plan, dev), ref, "clamps")


@pytest.fixture(scope="module")
def mean_case():
    """two 224 x 224 images (noise in 0..199, so that the means do not sit at 127.5) with contrast 0: alone, and as the last of four steps"""
    img = np.random.default_rng(5).integers(0, 200, (2, 224, 224, 3), dtype=np.uint8)
    plan = [U.make_plan([U.CONTRAST]), U.make_plan([U.BRIGHTNESS, U.SATURATION, U.HUE, U.CONTRAST])]
    factors = np.array([[1.0, 0.0, 1.0, 0.0], [1.2, 0.0, 0.8, 0.05]], dtype=np.float32)
    return img, factors, plan, U.oracle(img, factors, plan)


def test_the_contrast_mean(dev, mean_case):
    img, factors, plan, ref = mean_case
    out = _run(img, factors, plan, dev)
    for b in range(2):
        level = ref[b, 0, 0, 0]
        assert np.abs(ref[b] - level).max() < 1e-9  # contrast 0: the constant mean, of the transformed image for b = 1
        assert abs(level - np.floor(level) - 0.5) >= 0.05, level  # far from a rounding boundary: the mean may be off by 2e-4 of its value
        print(f"contrast mean of image {b}: oracle {level:.6f} levels, got {np.unique(out[b]).tolist()}")
        assert (out[b] == int(np.rint(level))).all(), (b, level, np.unique(out[b]))


def test_constant_image_stays_constant(dev):
    img = np.full((2, 9, 11, 3), 200, dtype=np.uint8)
    img[1, ..., 1] = 90  # one colour
    plan = [U.make_plan([U.CONTRAST, U.SATURATION]), U.make_plan([U.SATURATION, U.CONTRAST])]
    factors = np.array([[1.0, 1.37, 0.61, 0.0], [1.0, 0.77, 1.21, 0.0]], dtype=np.float32)
    out = _run(img, factors, plan, dev)
    assert (out[0] == 200).all()  # gray of (200, 200, 200) is 0.9999 * 200: off by 0.02 levels x |1 - f|, nowhere near a rounding boundary
    assert (out[1] == out[1][0, 0]).all()
    U.assert_matches(out, U.oracle(img, factors, plan), "constant images")


def test_workgroup_edge(dev):
    """17 x 241 = 4097 pixels: one pixel past the 1024 four-pixel groups a workgroup of the apply pass covers (the second workgroup of an image has a
    single item), and one past four rounds of the mean pass's 256 threads"""
    img = U.noise((3, 17, 241, 3), 6)
    plan = [U.make_plan(U.ORDERS[5]), U.make_plan(U.ORDERS[17], True), U.make_plan([U.CONTRAST])]
    factors = np.array([[1.23, 0.81, 1.31, -0.07], [0.77, 1.19, 0.69, 0.09], [1.0, 0.53, 1.0, 0.0]], dtype=np.float32)
    U.assert_matches(_run(img, factors, plan, dev), U.oracle(img, factors, plan), "17 x 241")


def test_bit_identity(dev):
    """two launches; in place against out of place; views that start 1 byte into their allocation (other single pixels, other groups, byte loads when
    source and destination are aligned differently) against aligned ones, and the byte in front is untouched"""
    img, factors, plan = U.all_orders_case(seed=7)
    first = _run(img, factors, plan, dev)
    assert np.array_equal(_run(img, factors, plan, dev), first)
    f, p = torch.from_numpy(factors).to(dev), torch.from_numpy(plan).to(dev)
    x = torch.from_numpy(img).to(dev)
    assert ops.color_jitter_u8(x, f, p, out=x) is x and np.array_equal(x.cpu().numpy(), first)
    n = img.size
    buf_i, buf_o = torch.zeros(n + 1, dtype=torch.uint8, device=dev), torch.full((n + 1,), 171, dtype=torch.uint8, device=dev)
    i1, o1 = buf_i[1:].view(img.shape), buf_o[1:].view(img.shape)
    i1.copy_(torch.from_numpy(img))
    assert ops.color_jitter_u8(i1, f, p, out=o1) is o1 and int(buf_o[0]) == 171 and np.array_equal(o1.cpu().numpy(), first)  # both 1 byte in
    assert np.array_equal(ops.color_jitter_u8(i1, f, p).cpu().numpy(), first)  # source 1 byte in, destination aligned: byte loads
    o1.zero_()
    ops.color_jitter_u8(torch.from_numpy(img).to(dev), f, p, out=o1)  # source aligned, destination 1 byte in
    assert int(buf_o[0]) == 171 and np.array_equal(o1.cpu().numpy(), first)
    ops.color_jitter_u8(i1, f, p, out=i1)  # in place, 1 byte in
    assert int(buf_i[0]) == 0 and np.array_equal(i1.cpu().numpy(), first)


def _batch(B, Hs, Ws, L, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.from_numpy(U.noise((B, Hs, Ws, 3), seed)), torch.randint(1, 500, (B, L), generator=g)


def test_pipeline_draws_seeded_parameters(dev):
    B, Hs, Ws, L = 8, 40, 52, 16
    pixels, text = _batch(B, Hs, Ws, L, 8)
    pipes = [DeviceBatchPipeline(dev, (B, Hs, Ws, 3), (B, L), crop_size=16, crop_generator=torch.Generator().manual_seed(21), color_jitter=CJ,
                                 color_jitter_prob=0.8, gray_scale_prob=0.2, jitter_generator=torch.Generator().manual_seed(22)) for _ in range(2)]
    got = []
    for pipe in pipes:
        pipe.submit(pixels, text)
        batch = pipe.next()
        factors, plan = batch["jitter"]
        assert sorted(batch) == ["_slot", "boxes", "image", "jitter", "text"]
        assert batch["image"].dtype == torch.uint8 and tuple(batch["image"].shape) == (B, 16, 16, 3)
        assert factors.is_cuda and factors.dtype == torch.float32 and tuple(factors.shape) == (B, 4)
        assert plan.is_cuda and plan.dtype == torch.int32 and tuple(plan.shape) == (B,)
        by_hand = ops.color_jitter_u8(ops.resized_crop_u8(pixels.to(dev), batch["boxes"], 16), factors, plan)  # crop, then jitter, then grayscale
        assert torch.equal(batch["image"], by_hand)
        pipe.release(batch)
        got.append((batch["image"].cpu(), factors.cpu(), plan.cpu(), batch["boxes"].cpu()))
    assert all(torch.equal(a, b) for a, b in zip(got[0], got[1]))  # the same seeds: the same parameters, the same pixels
    want = color_jitter_plan(B, CJ, 0.8, 0.2, generator=torch.Generator().manual_seed(22))
    assert torch.equal(got[0][1], want[0]) and torch.equal(got[0][2], want[1])
    assert torch.equal(got[0][3], random_resized_crop_boxes(B, Hs, Ws, generator=torch.Generator().manual_seed(21)))
    cropped = ops.resized_crop_u8(pixels.to(dev), got[0][3].to(dev), 16).cpu().numpy()
    U.assert_matches(got[0][0].numpy(), U.oracle(cropped, got[0][1].numpy(), got[0][2].numpy()), "pipeline batch")


def test_pipeline_takes_the_callers_parameters(dev):
    B, Hs, Ws, L = 4, 20, 24, 16
    pixels, text = _batch(B, Hs, Ws, L, 9)
    pipe = DeviceBatchPipeline.from_aug_cfg(dev, (B, Hs, Ws, 3), (B, L), 16, {"scale": (0.5, 1.0), "ratio": (0.9, 1.1), "color_jitter": CJ,
                                                                            "color_jitter_prob": 0.8, "gray_scale_prob": 0.2})
    assert pipe.crop_size == 16 and pipe.crop_scale == (0.5, 1.0) and pipe.crop_ratio == (0.9, 1.1) and pipe.jitter
    factors = torch.tensor([[1.0, 1.0, 1.0, 0.0], [1.3137, 1.0, 1.0, 0.0], [1.0, 0.7, 1.2, 0.1], [1.0, 1.0, 1.0, 0.0]])  # (1.3 k has a tie at every k = 5 mod 10)
    plan = torch.tensor([0, U.make_plan([U.BRIGHTNESS]), U.make_plan([U.HUE, U.CONTRAST, U.SATURATION]), JITTER_GRAY_BIT], dtype=torch.int32)
    boxes = torch.tensor([(2, 2, 16, 16)] * B, dtype=torch.int32)  # identity crops
    pipe.submit(pixels, text, boxes=boxes, jitter=(factors, plan))
    batch = pipe.next()
    assert torch.equal(batch["jitter"][0].cpu(), factors) and torch.equal(batch["jitter"][1].cpu(), plan)
    crop = pixels[:, 2:18, 2:18].numpy()
    assert np.array_equal(batch["image"][0].cpu().numpy(), crop[0])  # plan 0: the crop as it is
    U.assert_matches(batch["image"].cpu().numpy(), U.oracle(crop, factors.numpy(), plan.numpy()), "explicit jitter")
    pipe.release(batch)
    bad = factors.clone()
    bad[2, 3] = 0.7
    with pytest.raises(ValueError, match=r"check_jitter: image 2 .* hue shift outside"):
        pipe.submit(pixels, text, jitter=(bad, plan))
    with pytest.raises(ValueError, match="jitter must be"):
        pipe.submit(pixels, text, jitter=(factors[:2], plan[:2]))


def test_pipeline_without_the_new_options(dev):
    B, Hs, Ws, L = 4, 20, 24, 16
    pixels, text = _batch(B, Hs, Ws, L, 10)
    plain = DeviceBatchPipeline(dev, (B, Hs, Ws, 3), (B, L), color_jitter=CJ)  # color_jitter without a probability: ignored, as in the reference
    plain.submit(pixels, text)
    batch = plain.next()
    assert sorted(batch) == ["_slot", "image", "text"] and batch["image"] is batch["_slot"]["image"] and torch.equal(batch["image"].cpu(), pixels)
    plain.release(batch)
    with pytest.raises(ValueError, match="needs a pipeline built with color_jitter_prob or gray_scale_prob"):
        plain.submit(pixels, text, jitter=(torch.ones(B, 4), torch.zeros(B, dtype=torch.int32)))
    # jitter without crop_size: a new tensor, the slot's pixels stay as they were copied
    pipe = DeviceBatchPipeline(dev, (B, Hs, Ws, 3), (B, L), gray_scale_prob=1.0)
    pipe.submit(pixels, text)
    batch = pipe.next()
    assert sorted(batch) == ["_slot", "image", "jitter", "text"] and batch["image"] is not batch["_slot"]["image"]
    assert torch.equal(batch["_slot"]["image"].cpu(), pixels) and (batch["jitter"][1].cpu() == JITTER_GRAY_BIT).all()
    out = batch["image"].cpu().numpy()
    assert (out[..., 0] == out[..., 1]).all() and not np.array_equal(out, pixels.numpy())
    pipe.release(batch)
    with pytest.raises(ValueError, match="need uint8 images"):
        DeviceBatchPipeline(dev, (B, 3, Hs, Ws), (B, L), gray_scale_prob=0.2)
    with pytest.raises(ValueError, match="color_jitter must have 4 entries"):
        DeviceBatchPipeline(dev, (B, Hs, Ws, 3), (B, L), color_jitter_prob=0.8)


def test_jitter_survives_release_and_the_next_submit(dev):
    """the stream contract at depth 1, with and without the crop: what next() enqueued reads the slot (pixels and parameters) before release() records
    'free', and the copy stream waits for 'free' before the second submit overwrites the slot"""
    B, Hs, Ws, L = 4, 64, 64, 16
    first, text = _batch(B, Hs, Ws, L, 11)
    second = 255 - first
    jit = color_jitter_plan(B, CJ, 1.0, 0.5, generator=torch.Generator().manual_seed(6))
    jit2 = (jit[0].flip(0).contiguous(), jit[1].flip(0).contiguous())
    for crop in (None, 48):
        boxes = random_resized_crop_boxes(B, Hs, Ws, generator=torch.Generator().manual_seed(7)) if crop else None

        def by_hand(pixels, j):
            x = pixels.to(dev)
            x = ops.resized_crop_u8(x, boxes.to(dev), crop) if crop else x
            return ops.color_jitter_u8(x, j[0].to(dev), j[1].to(dev)).cpu()

        expect = by_hand(first, jit)
        pipe = DeviceBatchPipeline(dev, (B, Hs, Ws, 3), (B, L), depth=1, crop_size=crop, color_jitter=CJ, color_jitter_prob=1.0)
        kw = {"boxes": boxes} if crop else {}
        pipe.submit(first.pin_memory(), text.pin_memory(), jitter=jit, **kw)
        batch = pipe.next()
        pipe.release(batch)
        pipe.submit(second.pin_memory(), text.pin_memory(), jitter=jit2, **kw)
        assert torch.equal(batch["image"].cpu(), expect) and torch.equal(batch["jitter"][0].cpu(), jit[0]) and torch.equal(batch["jitter"][1].cpu(), jit[1])
        nxt = pipe.next()
        assert torch.equal(nxt["image"].cpu(), by_hand(second, jit2)) and torch.equal(nxt["jitter"][1].cpu(), jit2[1])
        pipe.release(nxt)
