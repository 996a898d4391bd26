"""CPU: the references of the exact-arithmetic GEMM tests (tests/gemm_exact.py, run on the MI355X by tests/test_gemm_exact_gpu.py and
tests/test_tile_rescue_gpu.py), checked alone.  For every case table: the operands are integers that survive bf16, the fp32 CPU product equals
the int64 product (fp32 sums of these integers are exact in any order), the 2^24 guard holds for the FULL shape, and at least 5 % of every bf16
output's values are exact ties (the rounding mode is exercised; measured 13 .. 22 %).  Large shapes are checked on a sample of output rows (NT) or
output columns (TN: the reduction runs over all M rows) -- the guard is evaluated for the whole reduction length either way."""
import pytest
import torch

from tests import gemm_exact as X


def _is_integer_bf16(t, r):
    assert t.dtype == torch.bfloat16
    i = t.to(torch.int64)
    assert int(i.abs().max()) <= r
    assert torch.equal(i.to(torch.bfloat16), t) and torch.equal(t.float().to(torch.bfloat16), t)
    return i


def _sample(n, k=384):
    """k indices spread over 0..n-1, the last one (a ragged tile's last row) among them"""
    if n <= k:
        return torch.arange(n)
    return torch.unique(torch.cat([torch.arange(0, n, n // (k - 1))[:k - 1], torch.tensor([n - 1])]))


@pytest.mark.parametrize("M,N,K", list(X.NT_SHAPES))
def test_nt_references_are_exact_and_tie_rich(M, N, K):
    o = X.nt_operands(M, N, K)
    assert X.R_NT * X.R_NT * K + X.BIAS_R < X.LIMIT
    rows = _sample(M)
    a, b = o["a"][rows], o["b"]
    ai, bi = _is_integer_bf16(o["a"], X.R_NT)[rows], _is_integer_bf16(b, X.R_NT)
    _is_integer_bf16(o["resid16"], X.BIAS_R)
    assert torch.equal(o["bias"], o["bias"].round()) and float(o["bias"].abs().max()) <= X.BIAS_R
    acc_i = ai @ bi.t()
    assert torch.equal((a.float() @ b.float().t()).to(torch.int64), acc_i) and torch.equal((a.float() @ b.float().t()).double(), acc_i.double())
    acc = X.exact_ref(a, b, "nt")
    assert torch.equal(acc, acc_i.double())
    sub = {"bias": o["bias"], "resid32": o["resid32"][rows], "resid16": o["resid16"][rows]}
    for name, alpha, with_bias in X.NT_EPILOGUES:
        want, pre32 = X.nt_reference(acc, sub, name, alpha, with_bias)
        if pre32 is not None:
            ties = X.tie_fraction(pre32)
            assert ties >= 0.05, f"[{M}x{N}x{K}] {name} alpha {alpha}: only {ties:.1%} of the values are bf16 ties"
            assert torch.equal(X.rne_bf16(pre32), pre32.to(torch.bfloat16))  # the bit-arithmetic rounding is torch's round-to-nearest-even
        if name == "resid_bf16":
            assert X.tie_fraction((pre32.to(torch.bfloat16).float() + sub["resid16"].float())) >= 0.02  # the second rounding sees ties as well


def test_nt_case_table_covers_the_layouts_the_issue_names():
    assert all(shape in X.NT_SHAPES for shape, _ in X.NT_CASES) and X.NT_LOGITS_CASE in X.NT_SHAPES and X.NT_RESCUE_SHAPE in X.NT_SHAPES
    for shape in ((1025, 264, 128), (25444, 768, 512)):
        assert {lay for s, lay in X.NT_CASES if s == shape} == set(X.NT_ALL_LAYOUTS)
    for (M, N, K), lay in X.NT_CASES:
        assert K % 32 == 0 and (lay != "B_cols" or K % 16 == 0) and (lay != "B_rows" or N % 8 == 0)


@pytest.mark.parametrize("shape,r", X.SPLITK_CASES)
def test_splitk_references_are_exact(shape, r):
    M, N, K = shape
    assert r * r * K < X.LIMIT
    o = X.splitk_operands(M, N, K, r)
    _is_integer_bf16(o["a"], r), _is_integer_bf16(o["b"], r), _is_integer_bf16(o["sub_parent"], X.BIAS_R)
    assert set(o["rowscale"].tolist()) <= {0.5, 1.0, 2.0}
    rows, cols = _sample(M, 96), _sample(N, 48)
    a, b = o["a"][rows], o["b"][cols]
    acc = X.exact_ref(a, b, "nt")
    assert torch.equal(acc, (a.to(torch.int64) @ b.to(torch.int64).t()).double()) and torch.equal((a.float() @ b.float().t()).double(), acc)
    sub = dict(o, rowscale=o["rowscale"][rows], sub=o["sub"][rows][:, cols])
    X.f32_exact(X.splitk_reference(sub, acc, True))


def _tn_check(a, b, M_full, r):
    assert r * r * M_full < X.LIMIT
    ai, bi = _is_integer_bf16(a, r), _is_integer_bf16(b, r)
    acc_i = ai.t() @ bi
    assert torch.equal((a.float().t() @ b.float()).double(), acc_i.double())
    assert torch.equal(a.float().sum(0).double(), ai.sum(0).double())
    return acc_i.double()


@pytest.mark.parametrize("M,N,K", list(X.TN_SHAPES))
def test_tn_references_are_exact(M, N, K):
    o = X.tn_operands(M, N, K)
    a, b = o["a"][:, :64], o["b"][:, :64]
    acc = _tn_check(a, b, M, X.R_TN)
    assert torch.equal(o["dw0"], o["dw0"].round()) and float(o["dw0"].abs().max()) <= X.BIAS_R
    for alpha in (1.0, 0.25):
        ref = X.exact_ref(a, b, "tn", alpha, o["dw0"][:a.shape[1], :b.shape[1]])
        assert torch.equal(ref, alpha * acc + o["dw0"][:a.shape[1], :b.shape[1]].double())
        X.f32_exact(ref)
        assert (alpha * X.R_TN * X.R_TN * M + X.BIAS_R) / alpha < X.LIMIT  # the guard of exact_ref at the worst case of the full shape


@pytest.mark.parametrize("M,N,K", [s[:3] for s in X.RESCUE_WGRAD_SHAPES] + [(M, 4 * C, C) for M, C, _ in X.TN_PAIR_CASES])
def test_wgrad_references_of_the_rescue_and_pair_tests_are_exact(M, N, K):
    """these operands are drawn on the GPU (same distribution): a 64-column sample here; the guard is the full reduction length's"""
    g = torch.Generator().manual_seed(M)
    _tn_check(X.int_operand((M, 64), X.R_TN, g), X.int_operand((M, 64), X.R_TN, g), M, X.R_TN)


def test_helpers_detect_what_they_are_for():
    parent, view = X.embed_out((5, 8), torch.float32, "cpu", 2, 8, 24)
    assert parent.shape == (9, 24) and torch.isnan(view).all() and int((parent == X.SENTINEL).sum()) == 9 * 24 - 40
    view.fill_(1.0)
    X.assert_outside_untouched(parent, view, X.SENTINEL)
    parent[6, 16] = 0.0  # first column behind the view's last row
    with pytest.raises(AssertionError, match="OUTSIDE"):
        X.assert_outside_untouched(parent, view, X.SENTINEL)
    want = torch.ones(5, 8)
    X.assert_bit_equal("ok", view, want.double())
    view[4, 7] = float("nan")
    with pytest.raises(AssertionError, match=r"1 of 40 elements differ.*\(4, 7,"):
        X.assert_bit_equal("nan", view, want)
    # ties go to even, both ways; truncation would give 256 and 260
    x = torch.tensor([257.0, 259.0, -257.0, 258.5, 2.0 ** -20])
    assert X.rne_bf16(x).tolist() == [256.0, 260.0, -256.0, 258.0, 2.0 ** -20] and X.tie_fraction(x) == 0.6
    with pytest.raises(AssertionError):
        X.exact_ref(torch.full((1, 2 ** 18), 8.0).bfloat16(), torch.full((1, 2 ** 18), 8.0).bfloat16(), "nt")
