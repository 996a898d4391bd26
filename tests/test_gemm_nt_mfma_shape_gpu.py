"""The persistent NT kernel's plain bf16-output launches under both MFMA shapes of its main loop (``ocn_set_gemm_variant`` NT value 6 = 32x32x16,
7 = 16x16x32; both force the persistent kernel as 5 does).

Integer operands (tests/gemm_exact.py): every partial sum is an exact fp32 integer in any order, alpha is a power of two and the bias an integer, so
the value in front of the bf16 rounding is exact and the output has to be bit-equal to its round-to-nearest-even value under either loop -- a
fragment read that takes another lane group's k, an accumulator block stored to another block's rows or columns, a bias quad added to the wrong
columns each change a bit (the operands are random and asymmetric).  Outputs sit inside a sentinel parent: a store outside the view shows.
Cases: the smallest paths (one whole / one partial row tile, a whole / a masked column tile, the two peeled K-tiles alone / one trip of the K loop),
the non-temporal store instantiation (N >= 1024), the half-tile tail, an output view with ldc > N.  Then Gaussian operands against float64."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from open_clip_amd import _lib, ops  # noqa: E402
from tests import gemm_exact as X  # noqa: E402

DEV = "cuda:0"
P = X.PAD_ROWS
LOOP_32, LOOP_16 = 6, 7  # NT value of ocn_set_gemm_variant
R = 4  # operands in [-4, 4]
SETTINGS = ((True, 1.0), (False, 1.0), (True, 0.5), (False, 0.5))  # (bias, alpha)


@pytest.fixture(autouse=True)
def _defaults_afterwards():
    yield
    _lib.call("ocn_set_gemm_variant", 0)


def _sid(shape):
    return "x".join(str(v) for v in shape)


def _case(shape, ld=None, col_off=0):
    """one shape through both loops, with and without bias, alpha 1 and 0.5: bit-equal to the integer result, nothing outside the view written"""
    M, N, K = shape
    assert K % 128 == 0 and N % 8 == 0  # what the persistent kernel takes
    o = X.nt_operands(M, N, K, r=R, device=DEV)
    acc = X.exact_ref(o["a"], o["b"], "nt")
    for bias, alpha in SETTINGS:
        want, _ = X.nt_reference(acc, o, "bf16", alpha, bias)
        got = {}
        for loop in (LOOP_32, LOOP_16):
            parent, out = X.embed_out((M, N), torch.bfloat16, DEV, P, col_off, ld or N)
            try:
                _lib.call("ocn_set_gemm_variant", loop)
                ops.gemm_nt(ops.EPI_BF16, o["a"], o["b"], out, bias=o["bias"] if bias else None, alpha=alpha)
            finally:
                _lib.call("ocn_set_gemm_variant", 0)
            tag = f"NT MFMA shape [{_sid(shape)}] ldc={ld or N} loop {loop} alpha={alpha}{' +bias' if bias else ''}"
            X.assert_bit_equal(tag, out, want)
            X.assert_outside_untouched(parent, out, X.SENTINEL, tag)
            got[loop] = out.clone()
        assert torch.equal(got[LOOP_32], got[LOOP_16])


@pytest.mark.parametrize("K", [128, 256])
@pytest.mark.parametrize("N", [256, 264])
@pytest.mark.parametrize("M", [256, 320])
def test_smallest_paths(M, N, K):
    """M = 320: a partial row tile; N = 264: a masked column tile with N % 8 == 0; K = 128: the two peeled K-tiles only; K = 256: one trip of the loop
    plus the peel"""
    _case((M, N, K))


def test_non_temporal_store_instantiation():
    """N = 1024: the wide-output store policy (AUX = 2)"""
    _case((320, 1024, 128))


def test_half_tile_tail():
    """280 tiles: on 256 CUs the last 24 are computed as 48 halves; (K / 64) % 4 == 0 as the tail requires"""
    M, N, K = 2560, 7168, 256
    assert (M // 256) * (N // 256) == 280 and (K // 64) % 4 == 0
    _case((M, N, K))


def test_strided_output_view():
    """ldc > N: the view starts 16 columns into a parent of N + 40 columns"""
    _case((320, 264, 256), ld=264 + 40, col_off=16)


def _rel_l2(got, ref64):
    return float((got.double() - ref64).norm() / ref64.norm())


def test_gaussian_operands_error_against_float64():
    """[512 x 768 x 768], unit Gaussian operands, four seeds: the relative L2 error of the bf16 result against the float64 product of the same bf16
    operands.  Both loops add exact bf16 products in fp32 and round once to bf16; the final rounding (2^-9 relative at most) dominates both errors,
    the summation order moves a few roundings.  The 16x16x32 loop's error must not exceed the 32x32x16 loop's on the same operands by more than the
    relative spread of the 32x32x16 loop's own error over the seeds -- a margin taken from the reference loop alone."""
    M, N, K = 512, 768, 768
    e32, e16 = [], []
    for seed in range(4):
        g = torch.Generator(device=DEV).manual_seed(1000 + seed)
        a = torch.randn(M, K, generator=g, device=DEV).bfloat16()
        b = torch.randn(N, K, generator=g, device=DEV).bfloat16()
        ref = a.double() @ b.double().t()
        err = {}
        for loop in (LOOP_32, LOOP_16):
            out = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
            try:
                _lib.call("ocn_set_gemm_variant", loop)
                ops.gemm_nt(ops.EPI_BF16, a, b, out)
            finally:
                _lib.call("ocn_set_gemm_variant", 0)
            err[loop] = _rel_l2(out, ref)
        e32.append(err[LOOP_32])
        e16.append(err[LOOP_16])
    spread = (max(e32) - min(e32)) / (sum(e32) / len(e32))
    margin = 1.0 + spread
    X.report(f"NT MFMA shape gaussian [{M}x{N}x{K}] rel-L2 vs float64: 32x32x16 {['%.6e' % e for e in e32]}  16x16x32 {['%.6e' % e for e in e16]}  "
             f"margin {margin:.6f}")
    for s, (x32, x16) in enumerate(zip(e32, e16)):
        assert x16 <= x32 * margin, f"seed {s}: 16x16x32 error {x16:.6e} > 32x32x16 error {x32:.6e} x {margin:.6f}"
