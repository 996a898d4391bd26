"""The hand-scheduled wgrad kernel and its 16x16x32 MFMA main loop (forced with ``ocn_set_gemm_variant`` TN field 3) on integer
operands (tests/gemm_exact.py): every reduction order is exact, so dW and dbias are bit-equal to the integer result, the atomic and the
deterministic form bit-equal to each other, and the sentinels around dW and dbias untouched.  The operands are random and asymmetric: a store map
with rows and columns swapped, a fragment read that takes another lane group's reduction rows, a bias strip summed twice or not at all each change
a bit.  Cases: the smallest 'big' shape and a shape with ragged N and K tiles on three layouts; a zero-filled tail of every length that ends on
another side of a lane group's 8 reduction rows or of a transposing read's 4; bias slices over 2 and 3 k-tiles; the paired launch; the rescue form."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from open_clip_amd import _lib, ops  # noqa: E402
from tests import gemm_exact as X  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")
P = X.PAD_ROWS
HAND = 3  # TN field of ocn_set_gemm_variant: the hand-scheduled kernel whatever the size of the product
MODES = (HAND, "det")


@pytest.fixture(autouse=True)
def _defaults_afterwards():
    yield
    ops.set_tile_rescue(False)
    _lib.call("ocn_set_gemm_variant", 0)


def _sid(shape):
    return "x".join(str(v) for v in shape)


_OPS = {}


def _operands(shape):
    """integer operands and the float64-exact references of one shape, once (consecutive cases share them)"""
    if shape not in _OPS:
        _OPS.clear()
        o = X.tn_operands(*shape, device=DEV)
        o["ref"] = {}
        for alpha in (1.0, 0.25):
            assert (alpha * X.R_TN * shape[0] + X.BIAS_R) / alpha < X.LIMIT  # the bias gradient's partial sums
            o["ref"][alpha] = (X.f32_exact(X.exact_ref(o["a"], o["b"], "tn", alpha, o["dw0"])),
                               X.f32_exact(alpha * o["a"].double().sum(0) + o["db0"].double()))
        _OPS[shape] = o
    return _OPS[shape]


def _outputs(o, layout, N, K):
    """(dW parent, dW, dbias parent, dbias): pre-loaded with integers, the sentinel around them"""
    if layout == "dW_rows":  # the upper two thirds of a larger weight / bias pair
        dwp, dw = X.embed(o["dw0"], N // 2, 0, K, X.SENTINEL, pad_after=0)
        dbp, db = X.embed(o["db0"][:, None], N // 2, 0, 1, X.SENTINEL, pad_after=0)
    else:
        dwp, dw = X.embed(o["dw0"], P, 0, K, X.SENTINEL)
        dbp, db = X.embed(o["db0"][:, None], P, 0, 1, X.SENTINEL)
    return dwp, dw, dbp, db


def _run(o, shape, layout, mode, bias, alpha, tag):
    """one wgrad under ``mode``; checks it against the integer result and the surroundings; returns (dW, dbias)"""
    M, N, K = shape
    a = X.embed(o["a"], P, 0, (N + 63) // 64 * 64 + 64, NAN)[1] if layout == "A_cols" else o["a"]
    dwp, dw, dbp, db = _outputs(o, layout, N, K)
    try:
        _lib.call("ocn_set_gemm_variant", (0 if mode == "det" else mode) << 4)
        ops.gemm_tn_accum(a, o["b"], dw, db[:, 0] if bias else None, alpha=alpha, deterministic=mode == "det")
    finally:
        _lib.call("ocn_set_gemm_variant", 0)
    ref_w, ref_b = o["ref"][alpha]
    X.assert_bit_equal(tag + " dW", dw, ref_w)
    X.assert_bit_equal(tag + " dbias", db[:, 0], ref_b if bias else o["db0"])
    X.assert_outside_untouched(dwp, dw, X.SENTINEL, tag + " dW")
    X.assert_outside_untouched(dbp, db, X.SENTINEL, tag + " dbias")
    return dw.clone(), db.clone()


def _case(shape, layout, settings=((True, 1.0), (False, 0.25))):
    o = _operands(shape)
    for bias, alpha in settings:
        got = {}
        for mode in MODES:
            tag = f"wgrad MFMA shape [{_sid(shape)}] {layout} mode {mode} alpha={alpha}{' +dbias' if bias else ''}{' rescue' if ops.tile_rescue() else ''}"
            got[mode] = _run(o, shape, layout, mode, bias, alpha, tag)
        assert torch.equal(got[HAND][0], got["det"][0]) and torch.equal(got[HAND][1], got["det"][1]), \
            f"[{_sid(shape)}] {layout}: variant {HAND} != deterministic form"


@pytest.mark.parametrize("layout", ["contig", "A_cols", "dW_rows"])
@pytest.mark.parametrize("shape", [(8203, 512, 512), (3000, 640, 328)], ids=_sid)
def test_smallest_and_ragged_shapes(shape, layout):
    """(8203, 512, 512): the smallest shape that is 'big', ragged M; (3000, 640, 328): ragged N and K tiles, reached through the forced variant"""
    _case(shape, layout)


@pytest.mark.parametrize("r", [1, 7, 8, 9, 16, 17, 24, 31])
def test_zero_filled_tail_against_the_lane_group_map(r):
    """M = 8192 + r: the last M-split's last 32-row step holds r rows, the rest reads as zero; each r ends on another side of a lane group's 8
    rows or of a read's 4"""
    _case((8192 + r, 512, 512), "contig", settings=((True, 1.0),))


@pytest.mark.parametrize("shape", [(8203, 512, 512), (3000, 264, 520)], ids=_sid)
def test_bias_slices(shape):
    """tiles_k = 2, and 3 with a ragged last k-tile (N = 264: a ragged n-tile too; forced through the variant): every step's column sums are
    taken by exactly one of the workgroups that share the strip, each of its 16-wide blocks by exactly one wave"""
    assert (shape[2] + 255) // 256 == (2 if shape[2] == 512 else 3)
    _case(shape, "contig", settings=((True, 1.0),))


@pytest.mark.parametrize("bias", [True, False], ids=["dbias", "nodbias"])
def test_paired_launch(bias):
    """ocn_gemm_tn_accum2 under variant 3: both problems bit-equal to the integer result and to two single launches"""
    M, C = 8203, 256
    assert M * 4 * C * C >= 2 ** 31 and C >= 256  # what sends the pair to the one-launch kernel
    g = torch.Generator(device=DEV).manual_seed(M + C)
    a1, a2 = X.int_operand((M, C), X.R_TN, g, DEV), X.int_operand((M, 3 * C), X.R_TN, g, DEV)
    b1, b2 = X.int_operand((M, C), X.R_TN, g, DEV), X.int_operand((M, C), X.R_TN, g, DEV)
    w1, w2 = X.int_operand((C, C), X.BIAS_R, g, DEV, torch.float32), X.int_operand((3 * C, C), X.BIAS_R, g, DEV, torch.float32)
    d1, d2 = X.int_operand((C,), X.BIAS_R, g, DEV, torch.float32), X.int_operand((3 * C,), X.BIAS_R, g, DEV, torch.float32)
    r1, r2 = X.exact_ref(a1, b1, "tn", 1.0, w1), X.exact_ref(a2, b2, "tn", 1.0, w2)
    rb1, rb2 = a1.double().sum(0) + d1.double(), a2.double().sum(0) + d2.double()
    p1, o1 = X.embed(w1, P, 0, C, X.SENTINEL)
    p2, o2 = X.embed(w2, P, C, 2 * C, X.SENTINEL)
    q1, e1 = X.embed(d1[:, None], P, 0, 1, X.SENTINEL)
    q2, e2 = X.embed(d2[:, None], P, 0, 1, X.SENTINEL)
    s1, s2, f1, f2 = w1.clone(), w2.clone(), d1.clone(), d2.clone()
    try:
        _lib.call("ocn_set_gemm_variant", HAND << 4)
        ops.gemm_tn_accum2(a1, b1, o1, e1[:, 0] if bias else None, a2, b2, o2, e2[:, 0] if bias else None)
        ops.gemm_tn_accum(a1, b1, s1, f1 if bias else None)
        ops.gemm_tn_accum(a2, b2, s2, f2 if bias else None)
    finally:
        _lib.call("ocn_set_gemm_variant", 0)
    tag = f"wgrad MFMA shape pair [M={M} C={C}]{' +dbias' if bias else ''}"
    X.assert_bit_equal(tag + " dW1", o1, r1)
    X.assert_bit_equal(tag + " dW2", o2, r2)
    X.assert_bit_equal(tag + " dbias1", e1[:, 0], X.f32_exact(rb1) if bias else d1)
    X.assert_bit_equal(tag + " dbias2", e2[:, 0], X.f32_exact(rb2) if bias else d2)
    assert torch.equal(o1, s1) and torch.equal(o2, s2) and torch.equal(e1[:, 0], f1) and torch.equal(e2[:, 0], f2), tag + ": pair != two single launches"
    for parent, view, name in ((p1, o1, "dW1"), (p2, o2, "dW2"), (q1, e1, "dbias1"), (q2, e2, "dbias2")):
        X.assert_outside_untouched(parent, view, X.SENTINEL, f"{tag} {name}")


def test_rescue_form_nothing_held():
    """ops.set_tile_rescue(True) with no workgroup held back: the rescue instantiations (the fixture restores the defaults)"""
    ops.set_tile_rescue(True)
    assert ops.tile_rescue()
    _case((8203, 512, 512), "contig")
