"""GPU: ``ocn_resized_crop_u8`` against the float64 oracle of tests/resized_crop_util.py (acceptance rule and its derivation there), at the smallest
shapes at which the kernel can still go wrong, and ``DeviceBatchPipeline(crop_size=...)`` around it."""
import numpy as np
import pytest
import torch

from open_clip_amd import ops
from open_clip_amd.input_pipeline import DeviceBatchPipeline, random_resized_crop_boxes
from tests import resized_crop_util as U
from tests.resample_util import SIX_BOXES  # also a case of its golden_cases()

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _noise(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8))


def _run(src, boxes, size, dev):
    out = ops.resized_crop_u8(src.to(dev), torch.as_tensor(boxes, dtype=torch.int32).to(dev), size)
    Ho, Wo = (size, size) if isinstance(size, int) else size
    assert out.dtype == torch.uint8 and tuple(out.shape) == (src.shape[0], Ho, Wo, 3)
    return out.cpu().numpy()


def test_six_boxes_in_one_launch(dev):
    """identity (bit-exact copy), the whole image (10 and 13 taps), a plain downscale, an upscale of noise (the oracle overshoots [0, 255]: the
    clamp), a box flush with the bottom-right corner, a single pixel"""
    src = _noise((6, 40, 52, 3), 1)
    ref = U.oracle(src.numpy(), SIX_BOXES, 16)
    assert ref[3].min() < -10 and ref[3].max() > 260  # the upscale does test the clamp
    out = _run(src, SIX_BOXES, 16, dev)
    for b, box in enumerate(SIX_BOXES):
        U.assert_matches(out[b], ref[b], f"box {box}")
    assert np.array_equal(out[0], src[0, 2:18, 2:18].numpy())  # scale 1: the weights are the unit matrix
    assert np.array_equal(out[4], src[4, 24:40, 36:52].numpy())
    assert np.array_equal(out[5], np.broadcast_to(src[5, 7, 9].numpy(), (16, 16, 3)))


def test_constant_image_stays_constant(dev):
    src = torch.full((3, 40, 52, 3), 200, dtype=torch.uint8)
    out = _run(src, [(0, 0, 40, 52), (3, 5, 31, 37), (1, 7, 9, 11)], (16, 24), dev)
    assert (out == 200).all()  # normalised weights: the sum is 200 (1 + O(2**-22)), nowhere near a rounding boundary


def test_largest_tap_count_non_square_output(dev):
    """a 64 x 64 box of a 70 x 70 source (rows of 210 bytes: no row but the first starts on a dword) -> 23 x 16: side ratios 2.8 and 4.0, the limit"""
    src = _noise((2, 70, 70, 3), 2)
    boxes = [(3, 5, 64, 64), (6, 0, 64, 64)]
    assert max(U.tap_counts(64, 16)) == 16 and max(U.tap_counts(64, 23)) == 12
    U.assert_matches(_run(src, boxes, (23, 16), dev), U.oracle(src.numpy(), boxes, (23, 16)), "64x64 -> 23x16")


def test_tile_edge_output(dev):
    """17 x 33: one row and one column past the 16 x 32 output tile, an output row of 99 bytes (dword and byte stores mixed)"""
    src = _noise((2, 40, 52, 3), 3)
    boxes = [(0, 0, 40, 52), (5, 4, 30, 41)]
    U.assert_matches(_run(src, boxes, (17, 33), dev), U.oracle(src.numpy(), boxes, (17, 33)), "-> 17x33")


def test_training_shape_with_sampled_boxes(dev):
    src = _noise((2, 256, 256, 3), 4)
    boxes = random_resized_crop_boxes(2, 256, 256, generator=torch.Generator().manual_seed(5))
    U.assert_matches(_run(src, boxes, 224, dev), U.oracle(src.numpy(), boxes.numpy(), 224), f"256x256 {boxes.tolist()} -> 224x224")


def test_bad_boxes_are_clamped_and_never_read_outside_src(dev):
    """boxes the host-side check refuses, handed straight to the op: one that starts above and left of the source (first image: the guard rows lie
    above it), one with a side of more than 5x the output, one that reaches 8 rows and 3 columns past the source (last image: guard rows below).
    The call returns, the output is the oracle on the clamped box (sides into [1, 4 m], source coordinates into the image), and it does not depend
    on the guard rows that surround src inside a larger allocation."""
    Hs, Ws, G = 40, 52, 12
    src = _noise((3, Hs, Ws, 3), 6)
    boxes = [(-5, -4, 20, 24), (2, 1, 30, 45), (20, 30, 28, 25)]  # 45 > 4 * 8: processed as (2, 1, 30, 32)
    size = (12, 8)
    ref = U.oracle_clamped(src.numpy(), boxes, size)
    assert np.abs(ref[1] - U.oracle(src.numpy()[1:2], [(2, 1, 30, 32)], size)[0]).max() < 1e-9
    outs = []
    for fill in (0, 255):
        big = torch.full((G + 3 * Hs + G, Ws, 3), fill, dtype=torch.uint8, device=dev)  # guard rows | the 3 images | guard rows
        inner = big[G:G + 3 * Hs].view(3, Hs, Ws, 3)
        inner.copy_(src)
        outs.append(ops.resized_crop_u8(inner, torch.tensor(boxes, dtype=torch.int32, device=dev), size).cpu().numpy())
    assert np.array_equal(outs[0], outs[1])
    for b, box in enumerate(boxes):
        U.assert_matches(outs[0][b], ref[b], f"bad box {box}")


def test_out_argument_and_unaligned_views(dev):
    """``out=`` is written in place; a src / out that starts 1 byte into its allocation takes the byte-load and byte-store paths"""
    src = _noise((2, 40, 52, 3), 7)
    boxes = [(0, 0, 40, 52), (3, 5, 31, 37)]
    ref = U.oracle(src.numpy(), boxes, (16, 20))
    buf_s = torch.zeros(src.numel() + 1, dtype=torch.uint8, device=dev)
    buf_o = torch.zeros(2 * 16 * 20 * 3 + 1, dtype=torch.uint8, device=dev)
    s1, o1 = buf_s[1:].view(2, 40, 52, 3), buf_o[1:].view(2, 16, 20, 3)
    s1.copy_(src)
    res = ops.resized_crop_u8(s1, torch.tensor(boxes, dtype=torch.int32, device=dev), (16, 20), out=o1)
    assert res is o1 and int(buf_o[0]) == 0
    U.assert_matches(o1.cpu().numpy(), ref, "unaligned src / out")
    assert np.array_equal(_run(src, boxes, (16, 20), dev), o1.cpu().numpy())  # aligned and unaligned paths: the same arithmetic


def _batch(B, Hs, Ws, L, seed):
    g = torch.Generator().manual_seed(seed)
    return _noise((B, Hs, Ws, 3), seed), torch.randint(1, 500, (B, L), generator=g)


def test_pipeline_crops_on_the_device(dev):
    B, Hs, Ws, L = 4, 40, 52, 16
    pixels, text = _batch(B, Hs, Ws, L, 8)
    pipes = [DeviceBatchPipeline(dev, (B, Hs, Ws, 3), (B, L), crop_size=16, crop_generator=torch.Generator().manual_seed(21)) for _ in range(2)]
    got = []
    for pipe in pipes:
        pipe.submit(pixels, text)
        batch = pipe.next()
        assert batch["image"].dtype == torch.uint8 and tuple(batch["image"].shape) == (B, 16, 16, 3)
        assert batch["boxes"].dtype == torch.int32 and tuple(batch["boxes"].shape) == (B, 4) and batch["boxes"].is_cuda
        assert torch.equal(batch["image"], ops.resized_crop_u8(pixels.to(dev), batch["boxes"], 16))
        assert torch.equal(batch["text"].cpu(), text)
        pipe.release(batch)
        got.append((batch["image"].cpu(), batch["boxes"].cpu()))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])  # the same seed, the same boxes, the same pixels
    assert torch.equal(got[0][1], random_resized_crop_boxes(B, Hs, Ws, generator=torch.Generator().manual_seed(21)))
    U.assert_matches(got[0][0].numpy(), U.oracle(pixels.numpy(), got[0][1].numpy(), 16), "pipeline batch")
    # explicit boxes (evaluation) are honoured, and checked on the host
    mine = torch.tensor([(2, 2, 16, 16), (0, 0, 40, 52), (3, 5, 31, 37), (24, 36, 16, 16)], dtype=torch.int32)
    pipes[0].submit(pixels, text, boxes=mine)
    batch = pipes[0].next()
    assert torch.equal(batch["boxes"].cpu(), mine) and torch.equal(batch["image"][0].cpu(), pixels[0, 2:18, 2:18])
    pipes[0].release(batch)
    with pytest.raises(ValueError, match="lies outside"):
        pipes[0].submit(pixels, text, boxes=mine + torch.tensor([30, 0, 0, 0], dtype=torch.int32))
    # without crop_size the batch is what it has always been: the slot's own pixels, no boxes
    plain = DeviceBatchPipeline(dev, (B, Hs, Ws, 3), (B, L))
    plain.submit(pixels, text)
    batch = plain.next()
    assert sorted(batch) == ["_slot", "image", "text"] and batch["image"] is batch["_slot"]["image"] and torch.equal(batch["image"].cpu(), pixels)
    plain.release(batch)
    with pytest.raises(ValueError, match="needs a pipeline built with crop_size"):
        plain.submit(pixels, text, boxes=mine)


def test_model_takes_the_cropped_batch(dev):
    """``tiny-test`` reads 64 x 64 images, so this pipeline crops 72 x 80 sources to 64: the model's output on the pipeline's batch is bit for bit its
    output on the same crop made by hand"""
    from open_clip_amd.configs import get_model_config
    from open_clip_amd.synth import init_state_dict
    from tests.test_model_gpu import _build
    cfg = get_model_config("tiny-test")
    S, L, B = cfg["vision_cfg"]["image_size"], cfg["text_cfg"]["context_length"], 4
    model = _build(cfg, init_state_dict(cfg, seed=3, perturb=True)).eval()
    pixels, text = _batch(B, 72, 80, L, 9)
    pipe = DeviceBatchPipeline(dev, (B, 72, 80, 3), (B, L), crop_size=S, crop_generator=torch.Generator().manual_seed(4))
    pipe.submit(pixels, text)
    batch = pipe.next()
    with torch.no_grad():
        a = model(image=batch["image"], text=batch["text"])
        pipe.release(batch)
        cropped = ops.resized_crop_u8(pixels.to(dev), batch["boxes"], S)
        b = model(image=cropped, text=text.to(dev))
    a, b = (x if isinstance(x, dict) else dict(zip(("image_features", "text_features", "logit_scale"), x)) for x in (a, b))
    assert torch.isfinite(a["image_features"]).all()
    assert torch.equal(a["image_features"], b["image_features"]) and torch.equal(a["text_features"], b["text_features"])


def test_crop_survives_release_and_the_next_submit(dev):
    """the stream contract at depth 1: the crop that next() enqueued reads the slot before release() records 'free', and the copy stream waits for
    'free' before the second submit overwrites the slot -- so the first batch's crop is the first batch's, by value"""
    B, Hs, Ws, L = 4, 256, 256, 16
    first, text = _batch(B, Hs, Ws, L, 10)
    second = 255 - first
    boxes = random_resized_crop_boxes(B, Hs, Ws, generator=torch.Generator().manual_seed(6))
    expect = ops.resized_crop_u8(first.to(dev), boxes.to(dev), 224).cpu()
    pipe = DeviceBatchPipeline(dev, (B, Hs, Ws, 3), (B, L), depth=1, crop_size=224)
    pipe.submit(first.pin_memory(), text.pin_memory(), boxes=boxes)
    batch = pipe.next()
    pipe.release(batch)
    pipe.submit(second.pin_memory(), text.pin_memory(), boxes=boxes.flip(0))
    assert torch.equal(batch["image"].cpu(), expect) and torch.equal(batch["boxes"].cpu(), boxes)
    nxt = pipe.next()
    assert torch.equal(nxt["image"].cpu(), ops.resized_crop_u8(second.to(dev), boxes.flip(0).to(dev), 224).cpu())
    pipe.release(nxt)
