"""GPU: ``ocn_resample_u8`` against the float64 oracle of tests/resample_util.py (acceptance rule and its derivation in tests/resized_crop_util.py) on
twelve ragged noise images whose row bytes cover all four residues mod 4, and ``DeviceBatchPipeline.ragged`` around it."""
import numpy as np
import pytest
import torch

from open_clip_amd import ops
from open_clip_amd.input_pipeline import DeviceBatchPipeline, check_resample_plan, color_jitter_plan, eval_resample_plan, train_resample_plan
from tests import resample_util as U

pytestmark = pytest.mark.gpu

SIZES_T = torch.tensor(U.SIZES)
MODES = ("shortest", "longest", "squash")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ragged():
    """the twelve noise images (seed 1234), packed once: (images, arena uint8 numpy, offsets int64 numpy); nobody modifies them"""
    images = U.noise_images(1234)
    assert sorted({(w * 3) % 4 for _, w in U.SIZES}) == [0, 1, 2, 3]
    arena, offsets = U.pack(images)
    return images, arena, offsets


def _run(arena, offsets, plan, size, dev, fill=0):
    plan = torch.as_tensor(np.asarray(plan), dtype=torch.int32)
    out = ops.resample_u8(torch.from_numpy(arena).to(dev), torch.from_numpy(np.asarray(offsets, dtype=np.int64)).to(dev), plan.to(dev), size, fill=fill)
    Ho, Wo = (size, size) if isinstance(size, int) else size
    assert out.dtype == torch.uint8 and tuple(out.shape) == (plan.shape[0], Ho, Wo, 3)
    return out.cpu().numpy()


def _judge(out, ref, plan, what):
    for b in range(out.shape[0]):
        U.assert_matches(out[b], ref[b], f"{what}, image {b} {U.SIZES[b] if out.shape[0] == len(U.SIZES) else ''} plan {tuple(int(v) for v in plan[b])}")


@pytest.mark.parametrize("mode", MODES)
def test_three_modes_to_32(dev, ragged, mode):
    """the validation transform of all twelve images in one launch; 'squash' and 'longest' reach a side ratio of exactly 4.0 (128 -> 32), the limit;
    'longest' pads with 7 on both sides"""
    _, arena, offsets = ragged
    plan = eval_resample_plan(SIZES_T, 32, mode)
    check_resample_plan(plan, torch.from_numpy(offsets), arena.size, 32)
    assert mode == "shortest" or float((plan[:, 4:6].double() / plan[:, 6:8].double()).max()) == 4.0
    ref = U.oracle(arena, offsets, plan.numpy(), 32, fill=7)
    out = _run(arena, offsets, plan, 32, dev, fill=7)
    _judge(out, ref, plan.numpy(), mode)
    if mode == "longest":  # (75, 100) -> 24 x 32: four rows of 7 above and below; (128, 40) -> 32 x 10: eleven columns left and right
        assert (out[0, :4] == 7).all() and (out[0, 28:] == 7).all() and (out[3, :, :11] == 7).all() and (out[3, :, 21:] == 7).all()
        assert not (out[0, 4:28] == 7).all(axis=-1).any() and not (out[3, :, 11:21] == 7).all(axis=-1).any()


def test_non_square_target_shortest(dev, ragged):
    _, arena, offsets = ragged
    plan = eval_resample_plan(SIZES_T, (24, 40), "shortest")
    check_resample_plan(plan, torch.from_numpy(offsets), arena.size, (24, 40))
    _judge(_run(arena, offsets, plan, (24, 40), dev), U.oracle(arena, offsets, plan.numpy(), (24, 40)), plan.numpy(), "shortest -> (24, 40)")


@pytest.mark.parametrize("mode", ["squash", "longest"])
def test_non_square_target_on_the_images_within_ratio_4(dev, ragged, mode):
    """(24, 40) squashes some of the twelve by more than 4 on an axis: those the host-side check refuses are left out, by its rule"""
    _, arena, offsets = ragged
    plan = eval_resample_plan(SIZES_T, (24, 40), mode)
    keep = []
    for b in range(len(U.SIZES)):
        try:
            check_resample_plan(plan[b:b + 1], torch.from_numpy(offsets[b:b + 1]), arena.size, (24, 40))
            keep.append(b)
        except ValueError as e:
            assert "more than 4 x its resized side" in str(e)
    assert 6 <= len(keep) < len(U.SIZES)
    plan, offs = plan[keep], offsets[keep]
    out, ref = _run(arena, offs, plan, (24, 40), dev, fill=7), U.oracle(arena, offs, plan.numpy(), (24, 40), fill=7)
    for i, b in enumerate(keep):
        U.assert_matches(out[i], ref[i], f"{mode} -> (24, 40), image {b} {U.SIZES[b]}")


def test_partial_tiles_on_both_axes(dev, ragged):
    """(20, 45): one full and one partial 16 x 32 tile on either axis, an output row of 135 bytes (dword and byte stores mixed)"""
    _, arena, offsets = ragged
    plan = eval_resample_plan(SIZES_T, (20, 45), "shortest")
    check_resample_plan(plan, torch.from_numpy(offsets), arena.size, (20, 45))
    _judge(_run(arena, offsets, plan, (20, 45), dev), U.oracle(arena, offsets, plan.numpy(), (20, 45)), plan.numpy(), "shortest -> (20, 45)")


def test_train_plans_on_the_ragged_set(dev, ragged):
    """an identity window (bit-exact copy), a single-pixel window, a window flush with the bottom-right corner, an upscale of noise (the oracle
    overshoots [0, 255]: the clamp), and one sampled box per image"""
    images, arena, offsets = ragged
    size = 32
    by_hand = {0: (3, 5, 32, 32), 1: (7, 9, 1, 1), 2: (37 - 32, 121 - 32, 32, 32), 3: (128 - 56, 40 - 36, 56, 36), 4: (1, 7, 9, 11)}
    plan = train_resample_plan(SIZES_T, size, scale=(0.3, 1.0), generator=torch.Generator().manual_seed(2))
    for b, box in by_hand.items():
        plan[b, 2:6] = torch.tensor(box, dtype=torch.int32)
    check_resample_plan(plan, torch.from_numpy(offsets), arena.size, size)
    ref = U.oracle(arena, offsets, plan.numpy(), size)
    assert ref[4].min() < -10 and ref[4].max() > 260  # the upscale does test the clamp
    out = _run(arena, offsets, plan, size, dev)
    _judge(out, ref, plan.numpy(), "train plans")
    assert np.array_equal(out[0], images[0][3:35, 5:37])  # scale 1: the weights are the unit matrix
    assert np.array_equal(out[1], np.broadcast_to(images[1][7, 9], (size, size, 3)))
    assert np.array_equal(out[2], images[2][5:37, 89:121])


def test_fixed_size_sources_match_the_crop_kernel_bit_for_bit(dev):
    """on sources of one size with dword-aligned rows, a train plan is a box: ocn_resample_u8 and ocn_resized_crop_u8 do the same arithmetic.  Both
    are now csrc/resample.hip's resample_tile, so this compares a routine with itself (the two kernels still fill their descriptions and choose
    their load modes separately); what holds the arithmetic to that of the two kernels it came from is test_outputs_are_the_bytes_of_the_parent_commit"""
    src = torch.from_numpy(np.random.default_rng(9).integers(0, 256, (4, 64, 64, 3), dtype=np.uint8))
    plan = train_resample_plan(torch.tensor([(64, 64)] * 4), 48, scale=(0.5, 1.0), generator=torch.Generator().manual_seed(4))
    offsets = torch.arange(4, dtype=torch.int64) * (64 * 64 * 3)
    a = ops.resample_u8(src.to(dev).view(-1), offsets.to(dev), plan.to(dev), 48)
    b = ops.resized_crop_u8(src.to(dev), plan[:, 2:6].contiguous().to(dev), 48)
    assert torch.equal(a, b)


@pytest.mark.parametrize("mode", MODES)
def test_constant_image_stays_constant(dev, mode):
    images = [np.full((h, w, 3), 200, dtype=np.uint8) for h, w in U.SIZES]
    arena, offsets = U.pack(images)
    plan = eval_resample_plan(SIZES_T, 32, mode)
    out = _run(arena, offsets, plan, 32, dev, fill=7)
    inside = ~np.isclose(U.oracle(arena, offsets, plan.numpy(), 32, fill=-1.0), -1.0)  # the oracle of a constant image is 200 or the fill
    assert (out[inside] == 200).all() and (out[~inside] == 7).all()  # normalised weights: 200 (1 + O(2**-22)), nowhere near a rounding boundary
    assert inside.all() == (mode != "longest")


def test_bad_plans_give_the_documented_clamped_result(dev, ragged):
    """plans and offsets the host-side check refuses, handed straight to the op.  The arena under test is the middle of a larger allocation with 1 MiB
    of a sentinel byte on each side; every deviation is small enough that a read the kernel failed to clamp would land in the sentinels and change
    the output with them.  The output is the oracle on the clamped plan (semantics in include/openclip_hip.h) and does not depend on the sentinels."""
    images, arena, offsets = ragged
    G = 1 << 20
    size = 32
    plan, offs = U.bad_plans(offsets)  # top = -3; two rows too many in the last image and in one in the middle; an offset beyond the arena; R = 0; n = 5 R
    bad = 0
    for b in range(len(U.SIZES)):  # five are refused by the host-side check (image 5's plan is consistent in itself: only the packer knows better)
        try:
            check_resample_plan(torch.from_numpy(plan[b:b + 1]), torch.from_numpy(offs[b:b + 1]), arena.size, size)
        except ValueError:
            bad += 1
    assert bad == 5
    ref = U.oracle_clamped(arena, offs, plan, size, fill=7)
    outs = []
    for sentinel in (0x5A, 0xA5):
        big = torch.full((G + arena.size + G,), sentinel, dtype=torch.uint8, device=dev)
        inner = big[G:G + arena.size]
        inner.copy_(torch.from_numpy(arena))
        outs.append(ops.resample_u8(inner, torch.from_numpy(offs).to(dev), torch.from_numpy(plan).to(dev), size, fill=7).cpu().numpy())
        assert bool((big[:G] == sentinel).all()) and bool((big[G + arena.size:] == sentinel).all())
    assert np.array_equal(outs[0], outs[1])
    _judge(outs[0], ref, plan, "bad plans")


def test_aligned_rows_last_in_the_arena(dev):
    """ragged + dword-aligned rows + a span that starts at byte 9 of a row (shifted down by 1) + the arena-end clamp: one dword per tap where the
    kernel used to take the aligned pair.  Two tile rows and two tile columns per image; the second image ends with the arena, which lies between
    1 MiB of a sentinel byte on each side, so a dword read past its end would change the output with the sentinel"""
    arena, offsets, plan, size = U.last_in_the_arena_case()
    assert plan[1, 3] * 3 == 9 and (plan[1, 1] * 3) % 4 == 0 and offsets[1] % 4 == 0
    check_resample_plan(torch.from_numpy(plan), torch.from_numpy(offsets), arena.size, size)
    ref = U.oracle(arena, offsets, plan, size)
    G, outs = 1 << 20, []
    for sentinel in (0x5A, 0xA5):
        big = torch.full((G + arena.size + G,), sentinel, dtype=torch.uint8, device=dev)
        inner = big[G:G + arena.size]
        inner.copy_(torch.from_numpy(arena))
        outs.append(ops.resample_u8(inner, torch.from_numpy(offsets).to(dev), torch.from_numpy(plan).to(dev), size).cpu().numpy())
        assert bool((big[:G] == sentinel).all()) and bool((big[G + arena.size:] == sentinel).all())
    assert np.array_equal(outs[0], outs[1])
    for b in range(2):
        U.assert_matches(outs[0][b], ref[b], f"last in the arena, image {b} plan {tuple(int(v) for v in plan[b])}")


def test_outputs_are_the_bytes_of_the_parent_commit(dev):
    """tests/golden/resample_parent.npz: what the two separate kernels (csrc/resized_crop.hip and csrc/resample.hip of the commit before they became
    one tile routine) wrote for ``U.golden_cases()`` -- the inputs of this file's and tests/test_resized_crop_gpu.py's tests.  Every byte must still
    be the same: the same taps, the same weights, the same order of summation, whichever load mode brings the bytes in"""
    golden = np.load(U.GOLDEN)
    cases = U.golden_cases()
    assert sorted(golden.files) == sorted(c["name"] for c in cases) and len(cases) == 11
    for case in cases:
        out = U.run_golden_case(case, dev)
        want = golden[case["name"]]
        assert out.dtype == np.uint8 and out.shape == want.shape, (case["name"], out.shape, want.shape)
        assert np.array_equal(out, want), f"{case['name']}: {int((out != want).sum())} of {out.size} bytes differ from the parent commit's"


def _text(B, L, seed):
    return torch.randint(1, 500, (B, L), generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("train", [False, True])
def test_ragged_pipeline_two_batches_in_flight(dev, ragged, train):
    images, arena, offsets = ragged
    B, L, size, cap = len(images), 16, 32, 1 << 18
    second = [np.ascontiguousarray(255 - im[: im.shape[0] // 2]) for im in images[::-1]]  # other sizes, fewer bytes: a shorter used prefix
    texts = [_text(B, L, 3), _text(B, L, 4)]
    kw = dict(train=True, crop_scale=(0.3, 1.0), crop_generator=torch.Generator().manual_seed(21)) if train else dict(resize_mode="longest", fill_color=7)
    pipe = DeviceBatchPipeline.ragged(dev, B, (B, L), size, cap, **kw)
    for s in pipe.slots:
        s["arena"].fill_(0xEE)  # the marker: what a submit does not bring stays
    torch.cuda.synchronize()
    pipe.submit(images, texts[0])
    pipe.submit(second, texts[1], sizes=torch.tensor([im.shape[:2] for im in second]))
    with pytest.raises(RuntimeError, match="all slots are in flight"):
        pipe.submit(images, texts[0])
    if train:
        g = torch.Generator().manual_seed(21)
        want = [train_resample_plan(torch.tensor([im.shape[:2] for im in ims]), size, (0.3, 1.0), generator=g) for ims in (images, second)]
    else:
        want = [eval_resample_plan(torch.tensor([im.shape[:2] for im in ims]), size, "longest") for ims in (images, second)]
    seen = []
    for i, ims in enumerate((images, second)):
        host_arena, host_offsets = U.pack(ims)
        batch = pipe.next()
        assert sorted(batch) == ["_slot", "image", "offsets", "plan", "text"]
        assert batch["image"].dtype == torch.uint8 and tuple(batch["image"].shape) == (B, size, size, 3)
        assert batch["plan"].dtype == torch.int32 and batch["plan"].is_cuda and torch.equal(batch["plan"].cpu(), want[i])
        assert batch["offsets"].dtype == torch.int64 and batch["offsets"].is_cuda and batch["offsets"].cpu().tolist() == host_offsets.tolist()
        direct = ops.resample_u8(torch.from_numpy(host_arena).to(dev), batch["offsets"], batch["plan"], size, fill=0 if train else 7)
        assert torch.equal(batch["image"], direct) and torch.equal(batch["text"].cpu(), texts[i])
        U.assert_matches(batch["image"].cpu().numpy(), U.oracle(host_arena, host_offsets, want[i].numpy(), size, fill=0 if train else 7), f"pipeline batch {i}")
        seen.append(batch["_slot"]["arena"].cpu().numpy())
        assert (seen[i][host_arena.size:] == 0xEE).all() and not (seen[i][:host_arena.size] == 0xEE).all()  # only the used prefix travelled
        pipe.release(batch)
    # the next submit into slot 0 brings fewer bytes than the first did: what lies behind its prefix is still the FIRST batch's, byte for byte
    used0, used1 = U.pack(images)[0].size, U.pack(second)[0].size
    assert used1 < used0
    pipe.submit(second, texts[1])
    batch = pipe.next()
    now = batch["_slot"]["arena"].cpu().numpy()
    assert batch["_slot"] is pipe.slots[0] and np.array_equal(now[used1:], seen[0][used1:]) and not np.array_equal(now[:used1], seen[0][:used1])
    pipe.release(batch)
    # the caller's plan is honoured and checked on the host
    mine = eval_resample_plan(SIZES_T, size, "squash")
    pipe.submit(images, texts[0], plan=mine)
    batch = pipe.next()
    assert torch.equal(batch["plan"].cpu(), mine)
    pipe.release(batch)
    bad = mine.clone()
    bad[2, 2] = 30
    with pytest.raises(ValueError, match=r"image 2 .*lies outside its source"):
        pipe.submit(images, texts[0], plan=bad)
    with pytest.raises(ValueError, match=r"pack_images: image 3 .*does not fit the arena of 65536 bytes"):
        DeviceBatchPipeline.ragged(dev, B, (B, L), size, 1 << 16).submit(images, texts[0])
    with pytest.raises(ValueError, match="need a pipeline built with DeviceBatchPipeline.ragged"):
        DeviceBatchPipeline(dev, (B, 8, 8, 3), (B, L)).submit(torch.zeros(B, 8, 8, 3, dtype=torch.uint8), texts[0], plan=mine)


def test_ragged_pipeline_with_jitter_behind_it(dev, ragged):
    """the colour jitter and grayscale run in place on the resampler's fresh output, with the parameters of the batch: bit for bit ops.color_jitter_u8"""
    images, arena, offsets = ragged
    B, L, size = len(images), 16, 32
    cj = dict(color_jitter=(0.4, 0.4, 0.4, 0.1), color_jitter_prob=0.8, gray_scale_prob=0.2)
    pipe = DeviceBatchPipeline.ragged(dev, B, (B, L), size, 1 << 18, train=True, crop_generator=torch.Generator().manual_seed(5),
                                      jitter_generator=torch.Generator().manual_seed(6), **cj)
    pipe.submit(images, _text(B, L, 7))
    batch = pipe.next()
    factors, jplan = color_jitter_plan(B, cj["color_jitter"], 0.8, 0.2, torch.Generator().manual_seed(6))
    assert torch.equal(batch["jitter"][0].cpu(), factors) and torch.equal(batch["jitter"][1].cpu(), jplan)
    plain = ops.resample_u8(torch.from_numpy(arena).to(dev), batch["offsets"], batch["plan"], size)
    assert torch.equal(batch["image"], ops.color_jitter_u8(plain, factors.to(dev), jplan.to(dev)))
    assert not torch.equal(batch["image"], plain)
    pipe.release(batch)
