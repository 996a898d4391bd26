"""Exact-arithmetic GEMM checks (helper module of tests/test_gemm_exact.py, tests/test_gemm_exact_gpu.py and tests/test_tile_rescue_gpu.py).

bf16 operands that hold small integers: every product and every partial sum is an integer, and while |sum| < 2^24 every fp32 partial sum is
exact in ANY order -- the MFMA tree, split-K slabs, fp32 atomics and the deterministic slabs alike.  An fp32 output therefore has to be
bit-equal to the integer result, a bf16 output bit-equal to its round-to-nearest-even value, and no tolerance has to be measured.  Operands and
outputs are embedded in larger parents (NaN around inputs, a sentinel around outputs): a kernel that reads a neighbour into a product or stores
outside its view changes a bit somewhere.

The case tables below are data: the CPU test checks the references alone (exactness guard, share of bf16 ties), the GPU tests run the kernels."""
import torch

LIMIT = 2 ** 24  # integers below it are exact in fp32
SENTINEL, SENTINEL_U8 = 12345.0, 255
PAD_ROWS = 8  # rows of parent before and after a view: 8 rows of any even length keep a bf16 / fp32 / uint8 view 16-byte aligned


def report(line):
    """one line into the parity report of tests/test_kernels_gpu.py (same file, same format)"""
    from tests.test_kernels_gpu import _report
    _report(line)


# ---- operands -----------------------------------------------------------------------------------------------------------------
def int_operand(shape, r, generator, device="cpu", dtype=torch.bfloat16):
    """integers drawn uniformly from [-r, r] (with ``generator``, on its device), as ``dtype`` on ``device``; r <= 127: exact in bf16"""
    assert 0 < r <= 127
    t = torch.randint(-r, r + 1, tuple(shape), generator=generator, device=generator.device, dtype=torch.int8)
    return t.to(device=device).to(dtype)


def rne_bf16(x32):
    """fp32 -> bf16, round to nearest even, in integer arithmetic on the bit pattern (finite inputs)"""
    assert x32.dtype == torch.float32
    bits = x32.contiguous().view(torch.int32)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & ~0xFFFF  # (magnitudes far below the exponent's overflow)
    return bits.view(torch.float32).to(torch.bfloat16)  # low 16 bits are zero: the cast drops nothing


def tie_fraction(x32):
    """share of fp32 values exactly halfway between two bf16 values (low 16 bits of the pattern == 0x8000)"""
    return float(((x32.contiguous().view(torch.int32) & 0xFFFF) == 0x8000).double().mean())


def f32_exact(ref64):
    """float64 reference -> fp32, asserting that nothing is lost"""
    r32 = ref64.float()
    assert torch.equal(r32.double(), ref64), "reference not representable in fp32: badly chosen case"
    return r32


def exact_ref(a, b, form, alpha=1.0, add=None):
    """float64  alpha * (a @ b^T)  (form 'nt': a [M, K], b [N, K])  or  alpha * (a^T @ b)  (form 'tn': a [M, N], b [M, K])  + ``add``.
    Guards (a badly chosen case fails here, on its own inputs, not on the kernel): max|a| * max|b| * reduction length < 2^24, so every partial
    sum a kernel can form is an exact fp32 integer in any order; with alpha = 2^-k and ``add`` accumulated into, every intermediate
    add + alpha * partial is a multiple of min(alpha, 1) below 2^24 of those steps."""
    assert form in ("nt", "tn")
    L = a.shape[1] if form == "nt" else a.shape[0]
    ra, rb = float(a.abs().max()), float(b.abs().max())
    assert ra * rb * L < LIMIT, f"|a| <= {ra}, |b| <= {rb}, reduction length {L}: partial sums can pass 2^24"
    ad, bd = a.double(), b.double()
    acc = ad @ bd.t() if form == "nt" else ad.t() @ bd
    assert float(acc.abs().max()) < LIMIT
    step = min(abs(alpha), 1.0)
    addmax = 0.0 if add is None else float(add.abs().max())
    assert (abs(alpha) * ra * rb * L + addmax) / step < LIMIT, "alpha * partial sums + the accumulated-into values leave fp32's exact range"
    ref = acc * alpha
    if add is not None:
        ref = ref + add.double()
    assert float(ref.abs().max()) / step < LIMIT
    return ref


# ---- views --------------------------------------------------------------------------------------------------------------------
def embed(t, pad_rows, col_off, ld, fill, pad_after=None):
    """(parent, view): a parent of ``ld`` columns filled with ``fill``; the view holds ``t``, starts at column ``col_off`` and has ``pad_rows``
    rows of parent before it and ``pad_after`` (default: as many) behind it"""
    rows, cols = t.shape
    assert col_off + cols <= ld
    pad_after = pad_rows if pad_after is None else pad_after
    parent = torch.full((pad_rows + rows + pad_after, ld), fill, dtype=t.dtype, device=t.device)
    view = parent[pad_rows:pad_rows + rows, col_off:col_off + cols]
    view.copy_(t)
    return parent, view


def embed_out(shape, dtype, device, pad_rows, col_off, ld, pad_after=None):
    """an OUTPUT view: the parent holds the sentinel (12345.0; 255 for the uint8 ``aux``), the view itself NaN (255 for ``aux``)"""
    u8 = dtype == torch.uint8
    t = torch.full(tuple(shape), SENTINEL_U8 if u8 else float("nan"), dtype=dtype, device=device)
    return embed(t, pad_rows, col_off, ld, SENTINEL_U8 if u8 else SENTINEL, pad_after)


def _region(parent, view):
    ld = parent.stride(0)
    off = view.storage_offset() - parent.storage_offset()
    assert view.stride(0) == ld and view.stride(1) == 1 and off >= 0
    return off // ld, off % ld


def assert_outside_untouched(parent, view, fill, name=""):
    """every element of ``parent`` outside ``view`` still equals ``fill``"""
    r0, c0 = _region(parent, view)
    masked = parent.clone()
    masked[r0:r0 + view.shape[0], c0:c0 + view.shape[1]] = fill
    if not torch.equal(masked, torch.full_like(parent, fill)):
        bad = (masked != fill).nonzero()
        first = [(int(r) - r0, int(c) - c0, float(parent[r, c])) for r, c in bad[:6].tolist()]
        raise AssertionError(f"{name}: {bad.shape[0]} elements OUTSIDE the output view were written; first (row, col relative to the view, value): {first}")


def _mismatch_message(name, got, want):
    bad = got != want  # a NaN (the view's pre-fill: an element never stored) differs from everything
    idx = bad.nonzero()
    tiles = torch.unique(idx // 256, dim=0)
    first = [(int(r), int(c), float(got[r, c]), float(want[r, c])) for r, c in idx[:6].tolist()] if got.dim() == 2 else \
            [(int(i[0]), float(got[i[0]]), float(want[i[0]])) for i in idx[:6].tolist()]
    return (f"{name}: {idx.shape[0]} of {got.numel()} elements differ; first (row, col, got, want): {first}; "
            f"256 x 256 tiles (tile row, tile col) hit: {tiles[:8].tolist()}{' ...' if tiles.shape[0] > 8 else ''} ({tiles.shape[0]} tiles)")


def assert_bit_equal(name, got, want):
    """``got`` (the kernel's output, fp32 / bf16 / uint8) equals ``want`` element for element; ``want``: same dtype, or the float64 reference of an
    fp32 output (converted with ``f32_exact``)"""
    if want.dtype == torch.float64:
        assert got.dtype == torch.float32
        want = f32_exact(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, want.dtype, got.shape, want.shape)
    if not torch.equal(got, want):
        raise AssertionError(_mismatch_message(name, got, want))


# ---- case tables (data; tests/test_gemm_exact.py checks every reference on the CPU) -------------------------------------------
R_NT = 8
BIAS_R = 64  # integer bias and residual in [-64, 64]
NT_VARIANTS = (0, 4, 5)  # ocn_set_gemm_variant: auto, the general ring kernel, the persistent kernel
# (M, N, K): the branch it reaches
NT_SHAPES = {
    (37, 6, 64): "ring kernel, scalar epilogue, 2 stages",
    (300, 200, 96): "ring kernel, 3 stages",
    (1025, 264, 128): "smallest auto-persistent shape: ragged M and N, one K pair, N % 16 == 8",
    (25444, 768, 512): "300 tiles: half-tile tail, ragged last tile row",
    (25444, 768, 384): "same walk, (K/64) % 4 != 0: whole-tile tail",
    (70000, 776, 384): "several tiles per workgroup, band walk",
}
NT_ALL_LAYOUTS = ("contig", "A_cols", "B_cols", "B_rows", "out_cols")
NT_CASES = ([((37, 6, 64), lay) for lay in ("contig", "A_cols")] + [((300, 200, 96), lay) for lay in ("contig", "A_cols")]
            + [((1025, 264, 128), lay) for lay in NT_ALL_LAYOUTS] + [((25444, 768, 512), lay) for lay in NT_ALL_LAYOUTS]
            + [((25444, 768, 384), lay) for lay in ("contig", "out_cols")] + [((70000, 776, 384), lay) for lay in ("contig", "out_cols")])
NT_LOGITS_CASE = (1025, 264, 128)  # EPI_F32 with ldc = N + 4 (the loss's fp32 logits): the persistent kernel declines, the result stays exact
NT_RESCUE_SHAPE = (25444, 768, 512)
# the exact epilogues: (name, alpha, bias?)
NT_EPILOGUES = (("f32", 1.0, True), ("f32", 0.5, True), ("f32", 2.0, True), ("bf16", 1.0, True), ("bf16", 0.5, False), ("resid_f32", 1.0, True),
                ("resid_bf16", 1.0, True))
GELU_SHAPES = ((1025, 264, 128), (25444, 768, 512))
GELU_LAYOUTS = ("out_cols", "B_cols")

SPLITK_CASES = (((1024, 256, 2048), 4), ((4096, 512, 32768), 2))  # (M, N, K), r

R_TN = 8
TN_SHAPES = {
    (33, 8, 8): "smallest shape",
    (100, 264, 520): "general kernel",
    (3000, 640, 328): "ragged K tile of the 256-wide kernel",
    (8203, 512, 512): "smallest shape that is 'big' under variant 0 (M N K >= 2^31), ragged M",
    (20011, 1536, 512): "many splits",
}
TN_LAYOUTS = ("contig", "A_cols", "dW_cols", "dW_rows")
TN_MODES = (0, 1, 3, "det")  # ocn_set_gemm_variant's TN field (auto, general, hand-scheduled) and the deterministic form
TN_DET_WORKSPACE_SHAPES = ((8203, 512, 512), (20011, 1536, 512))
TN_RESCUE_SHAPE = (8203, 512, 512)
TN_PAIR_CASES = ((8203, 256, True), (3000, 128, False))  # (M, C, paired kernel expected): a1 [M, C], a2 [M, 3C], b [M, C]
# tests/test_tile_rescue_gpu.py::test_wgrad_under_rescue_is_exact_on_integer_operands: (M, N, K, bias)
RESCUE_WGRAD_SHAPES = ((51200, 3072, 768, True), (51200, 768, 3072, False), (20000, 520, 264, True), (4096 * 77 // 8, 512, 2048, True))


def nt_seed(M, N, K):
    return M * 7 + N * 3 + K


def nt_operands(M, N, K, r=R_NT, device="cpu"):
    """the integer operands of one NT shape: a [M, K], b [N, K] bf16 in [-r, r]; bias [N] fp32, resid [M, N] (fp32 and bf16) in [-64, 64]"""
    g = torch.Generator().manual_seed(nt_seed(M, N, K))
    a = int_operand((M, K), r, g, device)
    b = int_operand((N, K), r, g, device)
    bias = int_operand((N,), BIAS_R, g, device, torch.float32)
    resid16 = int_operand((M, N), BIAS_R, g, device)
    return {"a": a, "b": b, "bias": bias, "resid32": resid16.float(), "resid16": resid16}


def nt_reference(acc64, ops_, name, alpha, with_bias):
    """(want, fp32 value in front of the first bf16 rounding | None) of one exact epilogue from the float64 product ``acc64``"""
    pre = acc64 * alpha + (ops_["bias"].double() if with_bias else 0.0)
    assert float(pre.abs().max()) / min(alpha, 1.0) < LIMIT
    if name == "f32":
        return f32_exact(pre), None
    if name == "bf16":
        return rne_bf16(f32_exact(pre)), f32_exact(pre)
    if name == "resid_f32":
        return f32_exact(pre + ops_["resid32"].double()), None
    assert name == "resid_bf16"  # out = bf16(resid + bf16(acc + bias)): both roundings, as ops.EPI_BIAS_RESID_BF16 states them
    lin = rne_bf16(f32_exact(pre))
    return rne_bf16(f32_exact(lin.double() + ops_["resid16"].double())), f32_exact(pre)


def tn_seed(M, N, K):
    return M * 5 + N * 11 + K


def tn_operands(M, N, K, r=R_TN, device="cpu"):
    """a [M, N], b [M, K] bf16 integers in [-r, r]; dW0 [N, K], db0 [N] fp32 integers in [-64, 64] (what dW / dbias hold on entry)"""
    g = torch.Generator().manual_seed(tn_seed(M, N, K))
    a = int_operand((M, N), r, g, device)
    b = int_operand((M, K), r, g, device)
    return {"a": a, "b": b, "dw0": int_operand((N, K), BIAS_R, g, device, torch.float32), "db0": int_operand((N,), BIAS_R, g, device, torch.float32)}


def splitk_operands(M, N, K, r, device="cpu"):
    """split-K NT with its riders, all exact: a [M, K], b [N, K] in [-r, r]; rowscale [M] in {0.5, 1, 2}; ``sub_rows`` = rows off..off+M, columns
    0..N of a larger integer bf16 matrix (the loss's y16[off:off + R, :E]); sub_alpha = 0.125; a device scale of 0.25"""
    g = torch.Generator().manual_seed(M + N + K)
    a = int_operand((M, K), r, g, device)
    b = int_operand((N, K), r, g, device)
    rowscale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (M,), generator=g)].to(device)
    sub_parent = int_operand((M + 2 * 24, N + 40), BIAS_R, g, device)
    return {"a": a, "b": b, "rowscale": rowscale, "sub_parent": sub_parent, "sub": sub_parent[24:24 + M, :N], "sub_alpha": 0.125,
            "scale": torch.tensor([0.25], device=device)}


def splitk_reference(o, acc64, riders):
    """float64 scale * (rowscale * acc - sub_alpha * sub) (riders) or acc; every intermediate is a multiple of 1/8 below 2^24 of them"""
    if not riders:
        return acc64
    inner = acc64 * o["rowscale"].double()[:, None] - o["sub_alpha"] * o["sub"].double()
    assert float((acc64 * o["rowscale"].double()[:, None]).abs().max()) / 0.125 < LIMIT and float(inner.abs().max()) / 0.125 < LIMIT
    return inner * float(o["scale"][0])
