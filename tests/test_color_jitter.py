"""CPU: the float64 oracle of the colour jitter (tests/color_jitter_util.py) on cases whose answer is known, the fp32 restatement behind DELTA, the
parameter sampler, the host-side parameter check, ``from_aug_cfg``'s refusals and the argument checks of ``ops.color_jitter_u8`` (which has no
CPU path)."""
import itertools
import types

import numpy as np
import pytest
import torch

from open_clip_amd import ops
from open_clip_amd.input_pipeline import JITTER_GRAY_BIT, DeviceBatchPipeline, check_jitter, color_jitter_plan
from tests import color_jitter_util as U

F1 = (1.0, 1.0, 1.0, 0.0)


def _with(k, v):
    f = list(F1)
    f[k] = v
    return f


# ---- the oracle ----
def test_oracle_brightness_alone_is_a_clamped_product():
    img = U.noise((5, 7, 3), 1)
    got = U.chain(img, _with(0, 1.7), U.make_plan([U.BRIGHTNESS]))
    assert np.array_equal(got, np.clip(np.float64(np.float32(1.7)) * (img / 255.0), 0.0, 1.0)) and got.max() == 1.0


def test_oracle_saturation_zero_is_grayscale_and_contrast_zero_the_mean():
    img = U.noise((5, 7, 3), 2)
    x = img / 255.0
    gray = 0.2989 * x[..., 0] + 0.587 * x[..., 1] + 0.114 * x[..., 2]
    sat0 = U.chain(img, _with(2, 0.0), U.make_plan([U.SATURATION]))
    assert np.allclose(sat0, U.chain(img, F1, U.make_plan([], gray=True)), rtol=0, atol=1e-15)
    assert np.allclose(sat0, np.repeat(gray[..., None], 3, axis=-1), rtol=0, atol=1e-15)
    con0 = U.chain(img, _with(1, 0.0), U.make_plan([U.CONTRAST]))
    assert np.allclose(con0, gray.mean(), rtol=0, atol=1e-15)
    # the mean is taken of the image as it stands when the contrast step is reached
    after = U.chain(img, (1.6, 0.0, 1.0, 0.0), U.make_plan([U.BRIGHTNESS, U.CONTRAST]))
    y = np.clip(np.float64(np.float32(1.6)) * x, 0, 1)
    assert np.allclose(after, (0.2989 * y[..., 0] + 0.587 * y[..., 1] + 0.114 * y[..., 2]).mean(), rtol=0, atol=1e-15)


def test_oracle_hue():
    gray = np.array([[[0, 0, 0], [255, 255, 255], [10, 10, 10], [200, 200, 200]]], dtype=np.uint8)
    for h in (-0.5, -0.13, 0.0, 0.3, 0.5):
        assert np.array_equal(255.0 * U.chain(gray, _with(3, h), U.make_plan([U.HUE])), gray.astype(np.float64)), h  # no chroma: nothing to turn
    img = U.noise((6, 6, 3), 3)
    plus, minus = (255.0 * U.chain(img, _with(3, h), U.make_plan([U.HUE])) for h in (0.5, -0.5))
    assert np.abs(plus - minus).max() < 1e-9  # half a turn either way
    red = np.array([[[255, 0, 0]]], dtype=np.uint8)
    assert np.rint(255.0 * U.chain(red, _with(3, 0.3), U.make_plan([U.HUE]))).tolist() == [[[51, 255, 0]]]
    back = 255.0 * U.chain(img, _with(3, 0.0), U.make_plan([U.HUE]))
    assert np.abs(back - img).max() < 1e-9  # the round trip in float64


def test_oracle_skips_absent_steps_and_unknown_codes():
    img = U.noise((4, 5, 3), 4)
    f = (1.3, 0.7, 1.2, 0.07)
    assert np.array_equal(U.chain(img, f, U.make_plan([0, U.CONTRAST, 0, U.SATURATION])), U.chain(img, f, U.make_plan([U.CONTRAST, U.SATURATION])))
    assert np.array_equal(U.chain(img, f, U.make_plan([7, 5, 6])), img / 255.0)


def test_fp32_restatement_stays_within_a_quarter_of_delta():
    """what DELTA rests on (tests/color_jitter_util.py): the chain in numpy fp32 against float64 over all 24 orders, with and without grayscale, on
    noise and on low-contrast images; and how much of the oracle lies in the band"""
    worst, fractions = 0.0, []
    for seed, low in itertools.product(range(3), (False, True)):
        img, fac, plan = U.all_orders_case(seed=seed, H=16, W=16)
        if low:
            img = (100 + img % 24).astype(np.uint8)
        ref = U.oracle(img, fac, plan)
        f32 = np.stack([255.0 * U.chain(img[b], fac[b], plan[b], dtype=np.float32).astype(np.float64) for b in range(len(plan))])
        worst = max(worst, float(np.abs(ref - f32).max()))
        fractions.append(float((np.abs(ref - np.floor(ref) - 0.5) < U.DELTA).mean()))
    print(f"fp32 against float64: at most {worst:.3e} levels; in the band: {np.mean(fractions):.3%} on average, {np.max(fractions):.3%} at most")
    assert worst <= U.DELTA / 4
    assert np.max(fractions) <= U.MAX_BAND_FRACTION / 2


# ---- the sampler ----
def _codes(plan):
    return torch.stack([(plan.long() >> (3 * k)) & 7 for k in range(4)], dim=1)


def test_plan_ranges_float_and_pair_forms():
    B = 4000
    fac, plan = color_jitter_plan(B, (0.4, 1.5, (0.5, 0.75), 0.1), 1.0, None, generator=torch.Generator().manual_seed(1))
    assert fac.dtype == torch.float32 and tuple(fac.shape) == (B, 4) and plan.dtype == torch.int32 and tuple(plan.shape) == (B,)
    for k, (lo, hi) in enumerate(((0.6, 1.4), (0.0, 2.5), (0.5, 0.75), (-0.1, 0.1))):  # 1 - 1.5 < 0: clipped to 0
        col = fac[:, k].double()
        assert lo - 1e-6 <= float(col.min()) and float(col.max()) <= hi + 1e-6, (k, float(col.min()), float(col.max()))
        assert float(col.min()) < lo + 0.02 * (hi - lo) and float(col.max()) > hi - 0.02 * (hi - lo)  # and the range is used up
        assert abs(float(col.mean()) - (lo + hi) / 2) < 0.03 * (hi - lo)
    assert (_codes(plan).sort(dim=1).values == torch.tensor([1, 2, 3, 4])).all() and not (plan & JITTER_GRAY_BIT).any()
    check_jitter(fac, plan)
    fac, plan = color_jitter_plan(100, (0.4, 0.4, 0.4, (-0.5, 0.5)), 1.0, 1.0)
    assert float(fac[:, 3].abs().max()) <= 0.5 and (plan & JITTER_GRAY_BIT).all()


def test_plan_drops_a_degenerate_step():
    fac, plan = color_jitter_plan(500, (0.4, 0, (1.0, 1.0), 0.1), 1.0, 0.0, generator=torch.Generator().manual_seed(2))
    codes = _codes(plan)
    assert (codes[:, :2].sort(dim=1).values == torch.tensor([1, 4])).all() and (codes[:, 2:] == 0).all()  # two steps, then nothing
    assert (fac[:, 1] == 1).all() and (fac[:, 2] == 1).all()
    both = {tuple(c) for c in codes[:, :2].tolist()}
    assert both == {(1, 4), (4, 1)}
    fac, plan = color_jitter_plan(50, (0, 0, 0, 0), 1.0, None)
    assert (plan == 0).all() and (fac == torch.tensor(F1)).all()


def test_plan_probabilities_zero_and_one():
    cj = (0.4, 0.4, 0.4, 0.1)
    fac, plan = color_jitter_plan(300, cj, 0.0, 0.0)
    assert (plan == 0).all() and (fac == torch.tensor(F1)).all()
    fac, plan = color_jitter_plan(300, None, None, None)  # as the reference: nothing asked, nothing needed
    assert (plan == 0).all()
    fac, plan = color_jitter_plan(300, cj, None, 1.0)  # no jitter probability: color_jitter is ignored (transform.py:442)
    assert (plan == JITTER_GRAY_BIT).all()
    fac, plan = color_jitter_plan(300, cj, 1.0, 1.0)
    assert ((plan & 0xfff) != 0).all() and (plan & JITTER_GRAY_BIT).all()
    fac, plan = color_jitter_plan(20000, cj, 0.8, 0.2, generator=torch.Generator().manual_seed(3))
    on, gray = ((plan & 0xfff) != 0).double().mean(), ((plan & JITTER_GRAY_BIT) != 0).double().mean()
    assert abs(float(on) - 0.8) < 0.02 and abs(float(gray) - 0.2) < 0.02  # 6 standard deviations = 0.017
    off = (plan & 0xfff) == 0
    assert (fac[off] == torch.tensor(F1)).all()  # an image without the jitter: four zero codes, identity factors
    with pytest.raises(ValueError, match="color_jitter must have 4 entries"):
        color_jitter_plan(4, None, 0.8, None)
    with pytest.raises(ValueError, match="color_jitter must have 4 entries"):
        color_jitter_plan(4, (0.4, 0.4, 0.4), 0.8, None)
    with pytest.raises(ValueError, match="hue range"):
        color_jitter_plan(4, (0.4, 0.4, 0.4, 0.6), 0.8, None)
    with pytest.raises(ValueError, match="must not be negative"):
        color_jitter_plan(4, (-0.4, 0.4, 0.4, 0.1), 0.8, None)


def test_plan_is_reproducible_under_a_generator():
    cj = (0.4, 0.4, 0.4, 0.1)
    a = color_jitter_plan(64, cj, 0.8, 0.2, generator=torch.Generator().manual_seed(11))
    b = color_jitter_plan(64, cj, 0.8, 0.2, generator=torch.Generator().manual_seed(11))
    c = color_jitter_plan(64, cj, 0.8, 0.2, generator=torch.Generator().manual_seed(12))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], c[0])
    d, e = color_jitter_plan(64, cj, 0.8, 0.2), color_jitter_plan(64, cj, 0.8, 0.2)  # the global generator moves on
    assert not torch.equal(d[0], e[0])


def test_plan_orders_are_uniform():
    """B = 24000, all four steps present: each of the 24 orders 1000 +- 200 times (a count has a standard deviation of 31: about 6 of them)"""
    _, plan = color_jitter_plan(24000, (0.4, 0.4, 0.4, 0.1), 1.0, None, generator=torch.Generator().manual_seed(5))
    values, counts = torch.unique(plan, return_counts=True)
    assert sorted(values.tolist()) == sorted(U.make_plan(o) for o in U.ORDERS)
    assert int(counts.min()) >= 800 and int(counts.max()) <= 1200, counts.tolist()


# ---- the host-side check ----
def test_check_jitter_names_what_is_wrong():
    fac = torch.tensor([F1, (1.2, 0.8, 1.1, 0.05), F1])
    plan = torch.tensor([0, U.make_plan([2, 4, 1, 3], True), U.make_plan([3])], dtype=torch.int32)
    check_jitter(fac, plan)

    def bad_factor(k, v):
        f = fac.clone()
        f[1, k] = v
        return f

    def bad_plan(v):
        p = plan.clone()
        p[2] = v
        return p

    for f, p, msg in ((bad_factor(0, float("nan")), plan, r"image 1 .* not finite"), (bad_factor(3, float("inf")), plan, r"image 1 .* not finite"),
                      (bad_factor(2, -0.1), plan, r"image 1 .* negative brightness, contrast or saturation"),
                      (bad_factor(3, 0.51), plan, r"image 1 .* hue shift outside"), (bad_factor(3, -0.6), plan, r"image 1 .* hue shift outside"),
                      (fac, bad_plan(U.make_plan([1, 5])), r"image 2 .* step code above 4"),
                      (fac, bad_plan(U.make_plan([1, 3, 1])), r"image 2 .* step twice"),
                      (fac, bad_plan(1 << 13), r"image 2 .* bits above the grayscale bit"), (fac, bad_plan(-1), r"image 2 ")):
        with pytest.raises(ValueError, match="check_jitter: " + msg):
            check_jitter(f, p)
    for f, p, msg in ((fac.double(), plan, "expected float32 factors"), (fac[:, :3], plan, "expected float32 factors"),
                      (fac, plan.long(), "expected an int32 plan"), (fac, plan[:2], "expected an int32 plan")):
        with pytest.raises(ValueError, match="check_jitter: " + msg):
            check_jitter(f, p)
    with pytest.raises(ValueError, match="host-side check"):
        check_jitter(types.SimpleNamespace(is_cuda=True), plan)  # stands in for a device tensor: refused before anything of it is read


# ---- from_aug_cfg ----
def test_from_aug_cfg_refuses_what_is_not_implemented():
    shapes = ("cuda:0", (4, 40, 52, 3), (4, 16), 16)
    for cfg, name in (({"use_timm": True}, "use_timm"), ({"re_prob": 0.25}, "re_prob"), ({"naflex": True}, "naflex"), ({"re_count": 2}, "re_count"),
                      (types.SimpleNamespace(scale=(0.9, 1.0), use_timm=True), "use_timm")):
        with pytest.raises(NotImplementedError, match="aug_cfg." + name):
            DeviceBatchPipeline.from_aug_cfg(*shapes, cfg)
    with pytest.raises(TypeError, match="unknown aug_cfg field"):
        DeviceBatchPipeline.from_aug_cfg(*shapes, {"colour_jitter": (0.4, 0.4, 0.4, 0.1)})


# ---- the op's argument checks ----
def test_op_refuses_bad_arguments_before_any_launch():
    img = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    fac, plan = torch.ones((2, 4)), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="must live on the MI355X"):
        ops.color_jitter_u8(img, fac, plan)
    with pytest.raises(RuntimeError, match="'img' must be uint8"):
        ops.color_jitter_u8(img.float(), fac, plan)
    with pytest.raises(RuntimeError, match=r"'img' must be \[B, H, W, 3\]"):
        ops.color_jitter_u8(img.permute(0, 3, 1, 2).contiguous(), fac, plan)  # CHW
    with pytest.raises(RuntimeError, match=r"'factors' must be float32 \[B = 2, 4\]"):
        ops.color_jitter_u8(img, fac[:1], plan)
    with pytest.raises(RuntimeError, match=r"'plan' must be int32 \[B = 2\]"):
        ops.color_jitter_u8(img, fac, plan[:, None])


def test_abi_refuses_bad_shapes_before_any_launch():
    from open_clip_amd import _lib, build
    build.build()
    p = 4096  # a fake aligned device pointer: never dereferenced
    for args, msg in (((0, 2, 8, 8, p, p, p, p, 0), "null operand"), ((p, 2, 8, 8, p, p, 0, p, 0), "null operand"),
                      ((p, 2, 8, 8, p + 2, p, p, p, 0), "factors, plan and mean_ws must be 4-byte aligned"), ((p, 0, 8, 8, p, p, p, p, 0), r"bad shape B=0 H=8 W=8"),
                      ((p, 2, 8193, 8, p, p, p, p, 0), r"bad shape B=2 H=8193 W=8"), ((p, 2, 8, 0, p, p, p, p, 0), r"bad shape B=2 H=8 W=0")):
        with pytest.raises(RuntimeError, match=r"ocn_color_jitter_u8 failed \(-1\): ocn_color_jitter_u8: " + msg):
            _lib.call("ocn_color_jitter_u8", *args)
