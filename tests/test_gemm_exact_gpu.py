"""Every GEMM path on integer operands and strided views (tests/gemm_exact.py): fp32 outputs bit-equal to the integer result, bf16 outputs bit-equal
to its round-to-nearest-even value, atomic and deterministic wgrads bit-equal to each other, and every output parent untouched outside the view.
The layouts are the views the product passes: ``A_cols`` (lda = K + 72, column 64), ``B_cols`` (the w_t[:, C:] view: ldb = 3K/2, column K/2),
``B_rows`` (w_n[C:] with the bias slice), ``out_cols`` (out, resid and aux with ldc = N + 24 at column 8); for the wgrads ``A_cols`` (G[:, :Np]:
lda = round_up(N, 64) + 64), ``dW_cols`` (into=d_all[:, E:]: ldw = 2K, column K) and ``dW_rows`` (d.wqkv[C:] with d.bqkv[C:]).  Input parents hold
NaN around the view, output parents a sentinel, the output view itself NaN: a neighbour read into a product, a store into the ld gap and an
element never stored all change a bit.  The activation epilogues are not exact arithmetic: they run on the same views with Gaussian operands
under the bounds of tests/test_kernels_gpu.py, with the surroundings check exact."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

from open_clip_amd import _lib, ops  # noqa: E402
from tests import gemm_exact as X  # noqa: E402
from tests.test_kernels_gpu import check, check_saved_derivative  # noqa: E402

DEV = "cuda:0"
BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
NAN = float("nan")
P = X.PAD_ROWS
EPI = {"f32": ops.EPI_F32, "bf16": ops.EPI_BF16, "resid_f32": ops.EPI_BIAS_RESID_F32, "resid_bf16": ops.EPI_BIAS_RESID_BF16}


@pytest.fixture(autouse=True)
def _defaults_afterwards():
    yield
    ops.set_tile_rescue(False)
    _lib.call("ocn_set_gemm_variant", 0)


def _sid(shape):
    return "x".join(str(v) for v in shape)


# ---- NT ---------------------------------------------------------------------------------------------------------------------
_NT = {}


def _nt(shape):
    """operands and the references of every exact epilogue, once per shape (consecutive cases share them)"""
    if shape not in _NT:
        _NT.clear()
        o = X.nt_operands(*shape, device=DEV)
        acc = X.exact_ref(o["a"], o["b"], "nt")
        o["want"], ties = {}, []
        for name, alpha, with_bias in X.NT_EPILOGUES:
            o["want"][(name, alpha, with_bias)], pre32 = X.nt_reference(acc, o, name, alpha, with_bias)
            if pre32 is not None:
                ties.append(X.tie_fraction(pre32))
        o["ties"] = min(ties)
        assert o["ties"] >= 0.05
        _NT[shape] = o
    return _NT[shape]


def _nt_inputs(o, layout, M, N, K):
    a, b, bias = o["a"], o["b"], o["bias"]
    if layout == "A_cols":
        _, a = X.embed(a, P, 64, K + 72, NAN)
    elif layout == "B_cols":  # w_t[:, C:]
        _, b = X.embed(b, P, K // 2, 3 * K // 2, NAN)
    elif layout == "B_rows":  # w_n[C:] and bqkv[C:]
        _, b = X.embed(b, N // 2, 0, K, NAN)
        bias = X.embed(bias[:, None], N // 2, 0, 1, NAN)[1][:, 0]
        assert bias.is_contiguous()
    return a, b, bias


def _nt_exact_case(shape, layout, variant, geometry=None):
    M, N, K = shape
    o = _nt(shape)
    a, b, bias = _nt_inputs(o, layout, M, N, K)
    col, ldc = geometry or ((8, N + 24) if layout == "out_cols" else (0, N))
    try:
        _lib.call("ocn_set_gemm_variant", variant)
        for name, alpha, with_bias in X.NT_EPILOGUES:
            tag = f"gemm_nt exact [{_sid(shape)}] {layout} v{variant} {name} alpha={alpha}{' +bias' if with_bias else ''}"
            outp, out = X.embed_out((M, N), F32 if name in ("f32", "resid_f32") else BF16, DEV, P, col, ldc)
            kw = {"bias": bias} if with_bias else {}
            if name.startswith("resid"):
                kw["resid"] = X.embed(o["resid32" if name == "resid_f32" else "resid16"], P, col, ldc, NAN)[1]
            ops.gemm_nt(EPI[name], a, b, out, alpha=alpha, **kw)
            X.assert_bit_equal(tag, out, o["want"][(name, alpha, with_bias)])
            X.assert_outside_untouched(outp, out, X.SENTINEL, tag)
    finally:
        _lib.call("ocn_set_gemm_variant", 0)
    X.report(f"gemm_nt exact [{_sid(shape)}] {layout:8s} v{variant} ldc={ldc}{' rescue' if ops.tile_rescue() else ''}: {len(X.NT_EPILOGUES)} epilogues bit-equal, "
             f"surroundings untouched; bf16 ties {o['ties']:.1%} ({X.NT_SHAPES[shape]})")


@pytest.mark.parametrize("shape,layout,variant", [(s, lay, v) for (s, lay), v in itertools.product(X.NT_CASES, X.NT_VARIANTS)],
                         ids=lambda v: _sid(v) if isinstance(v, tuple) else str(v))
def test_gemm_nt_exact(shape, layout, variant):
    _nt_exact_case(shape, layout, variant)


@pytest.mark.parametrize("variant", X.NT_VARIANTS)
def test_gemm_nt_exact_logits_layout(variant):
    """ldc = N + 4 (the loss's fp32 logits, round_up(N, 4) columns): not a multiple of 8 -- the persistent kernel declines, the general one is exact"""
    M, N, K = X.NT_LOGITS_CASE
    o = _nt(X.NT_LOGITS_CASE)
    try:
        _lib.call("ocn_set_gemm_variant", variant)
        for alpha in (1.0, 0.5):
            outp, out = X.embed_out((M, N), F32, DEV, P, 0, N + 4)
            ops.gemm_nt(ops.EPI_F32, o["a"], o["b"], out, bias=o["bias"], alpha=alpha)
            X.assert_bit_equal(f"logits layout v{variant} alpha={alpha}", out, o["want"][("f32", alpha, True)])
            X.assert_outside_untouched(outp, out, X.SENTINEL)
    finally:
        _lib.call("ocn_set_gemm_variant", 0)
    X.report(f"gemm_nt exact [{_sid(X.NT_LOGITS_CASE)}] logits   v{variant} ldc={N + 4}: f32 bit-equal, surroundings untouched")


@pytest.mark.parametrize("layout", X.NT_ALL_LAYOUTS)
def test_gemm_nt_exact_rescue_form_nothing_held(layout):
    ops.set_tile_rescue(True)
    assert ops.tile_rescue()
    _nt_exact_case(X.NT_RESCUE_SHAPE, layout, 0)


@pytest.mark.parametrize("shape,layout,variant", [(s, lay, v) for s in X.GELU_SHAPES for lay in X.GELU_LAYOUTS for v in (0, 4)],
                         ids=lambda v: _sid(v) if isinstance(v, tuple) else str(v))
def test_gemm_nt_activation_epilogues_on_views(shape, layout, variant):
    """GELU / QuickGELU / dGELU: Gaussian operands and the bounds of tests/test_kernels_gpu.py (unchanged); exact is the check of the surroundings
    of ``out`` and ``aux``"""
    M, N, K = shape
    g = torch.Generator().manual_seed(M * 7 + N)
    a = (torch.randn(M, K, generator=g)).to(BF16).to(DEV)
    b = (torch.randn(N, K, generator=g) * K ** -0.5).to(BF16).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    dsaved = torch.randint(0, 253, (M, N), generator=g, dtype=U8).to(DEV)
    ref = a.float() @ b.float().t()
    if layout == "B_cols":
        _, b = X.embed(b, P, K // 2, 3 * K // 2, NAN)
    col, ldc = (8, N + 24) if layout == "out_cols" else (0, N)
    tag = f"gemm_nt [{_sid(shape)}] {layout} v{variant}"
    pre = (ref + bias).requires_grad_(True)
    try:
        _lib.call("ocn_set_gemm_variant", variant)
        for name, epi, act in (("gelu", ops.EPI_BIAS_GELU, torch.nn.functional.gelu), ("quickgelu", ops.EPI_BIAS_QUICKGELU, lambda x: x * torch.sigmoid(1.702 * x))):
            outp, out = X.embed_out((M, N), BF16, DEV, P, col, ldc)
            auxp, aux = X.embed_out((M, N), U8, DEV, P, col, ldc)
            ops.gemm_nt(epi, a, b, out, bias=bias, aux=aux)
            pre.grad = None
            y = act(pre)
            y.backward(torch.ones_like(y))
            check(f"{tag} {name}.out", out, y.detach(), bf16_out=True, abs_tol=1e-3)
            check_saved_derivative(f"{tag} {name}.saved_derivative", aux, pre.grad)
            X.assert_outside_untouched(outp, out, X.SENTINEL, f"{tag} {name}.out")
            X.assert_outside_untouched(auxp, aux, X.SENTINEL_U8, f"{tag} {name}.aux")
        outp, out = X.embed_out((M, N), BF16, DEV, P, col, ldc)
        auxp, aux = X.embed(dsaved, P, col, ldc, X.SENTINEL_U8)  # an input here: 255 around it decodes to a value no element may pick up
        before = auxp.clone()
        ops.gemm_nt(ops.EPI_DGELU, a, b, out, aux=aux)
        check(f"{tag} dgelu", out, ref * ops.dgelu_decode(dsaved), bf16_out=True, abs_tol=1e-3)
        X.assert_outside_untouched(outp, out, X.SENTINEL, f"{tag} dgelu.out")
        assert torch.equal(auxp, before), f"{tag}: dGELU wrote to the saved derivative"
    finally:
        _lib.call("ocn_set_gemm_variant", 0)
    X.report(f"{tag}: gelu / quickgelu / dgelu within the bf16 bounds, surroundings of out and aux untouched")


# ---- split-K ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,r", X.SPLITK_CASES, ids=lambda v: _sid(v) if isinstance(v, tuple) else f"r{v}")
def test_gemm_nt_splitk_exact(shape, r):
    M, N, K = shape
    ks = ops.gemm_nt_splitk_plan(M, N, K)
    assert ks >= 2 and (shape != (1024, 256, 2048) or ks == 2), ks
    o = X.splitk_operands(M, N, K, r, DEV)
    acc = X.exact_ref(o["a"], o["b"], "nt")
    _, a = X.embed(o["a"], P, 64, K + 72, NAN)
    assert o["sub"].stride(0) == N + 40 and o["sub"].storage_offset() > 0
    for riders in (False, True):
        outp, out = X.embed_out((M, N), F32, DEV, P, 8, N + 24)
        kw = dict(rowscale=o["rowscale"], sub_rows=o["sub"], sub_alpha=o["sub_alpha"], scale=o["scale"]) if riders else {}
        ops.gemm_nt_splitk(a, o["b"], out, ks, **kw)
        tag = f"gemm_nt_splitk exact [{_sid(shape)}] r={r} ks={ks}{' riders' if riders else ''}"
        X.assert_bit_equal(tag, out, X.splitk_reference(o, acc, riders))
        X.assert_outside_untouched(outp, out, X.SENTINEL, tag)
    X.report(f"gemm_nt_splitk exact [{_sid(shape)}] r={r} ks={ks} lda={K + 72} ldc={N + 24}: plain and with rowscale / sub_rows view / device scale bit-equal")


# ---- TN ---------------------------------------------------------------------------------------------------------------------
_TN = {}


def _tn(shape):
    if shape not in _TN:
        _TN.clear()
        o = X.tn_operands(*shape, device=DEV)
        M = shape[0]
        o["ref"] = {}
        for alpha in (1.0, 0.25):
            assert (alpha * X.R_TN * M + X.BIAS_R) / alpha < X.LIMIT  # the bias gradient's partial sums
            o["ref"][alpha] = (X.f32_exact(X.exact_ref(o["a"], o["b"], "tn", alpha, o["dw0"])), X.f32_exact(alpha * o["a"].double().sum(0) + o["db0"].double()))
        _TN[shape] = o
    return _TN[shape]


def _round_up(v, m):
    return (v + m - 1) // m * m


def _tn_outputs(o, layout, N, K):
    """(dW parent, dW, dbias parent, dbias): pre-loaded with integers, the sentinel around them"""
    if layout == "dW_cols":  # into=d_all[:, E:]
        dwp, dw = X.embed(o["dw0"], P, K, 2 * K, X.SENTINEL)
    elif layout == "dW_rows":  # d.wqkv[C:] and d.bqkv[C:]: the upper two thirds of a larger pair
        dwp, dw = X.embed(o["dw0"], N // 2, 0, K, X.SENTINEL, pad_after=0)
    else:
        dwp, dw = X.embed(o["dw0"], P, 0, K, X.SENTINEL)
    pad = N // 2 if layout == "dW_rows" else P
    dbp, db = X.embed(o["db0"][:, None], pad, 0, 1, X.SENTINEL, pad_after=0 if layout == "dW_rows" else None)
    return dwp, dw, dbp, db


def _tn_exact_case(shape, layout):
    M, N, K = shape
    o = _tn(shape)
    a = X.embed(o["a"], P, 0, _round_up(N, 64) + 64, NAN)[1] if layout == "A_cols" else o["a"]  # G[:, :Np]
    got = {}
    for mode in X.TN_MODES:
        for bias, alpha in ((True, 1.0), (False, 0.25)):
            dwp, dw, dbp, db = _tn_outputs(o, layout, N, K)
            tag = f"gemm_tn exact [{_sid(shape)}] {layout} mode {mode} alpha={alpha}{' +dbias' if bias else ''}"
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
            got[(mode, bias)] = (dw.clone(), db.clone())
    for bias in (True, False):
        for mode in (0, 1, 3):
            assert torch.equal(got[(mode, bias)][0], got[("det", bias)][0]) and torch.equal(got[(mode, bias)][1], got[("det", bias)][1]), \
                f"[{_sid(shape)}] {layout}: atomic form (variant {mode}) != deterministic form"
    need = int(_lib.load().ocn_gemm_tn_det_workspace_bytes(M, N, K))
    if shape in X.TN_DET_WORKSPACE_SHAPES:
        assert need > 0, "the deterministic form of this shape must be the slab form"
    X.report(f"gemm_tn exact [{_sid(shape)}] {layout:8s}{' rescue' if ops.tile_rescue() else ''}: variants 0 / 1 / 3 and deterministic (workspace {need} B) x (dbias, alpha 1 | no dbias, "
             f"alpha 0.25) bit-equal to the integer result and to each other, surroundings untouched ({X.TN_SHAPES[shape]})")


@pytest.mark.parametrize("shape,layout", [(s, lay) for s in X.TN_SHAPES for lay in X.TN_LAYOUTS], ids=lambda v: _sid(v) if isinstance(v, tuple) else str(v))
def test_gemm_tn_exact(shape, layout):
    _tn_exact_case(shape, layout)


@pytest.mark.parametrize("layout", X.TN_LAYOUTS)
def test_gemm_tn_exact_rescue_form_nothing_held(layout):
    ops.set_tile_rescue(True)
    assert ops.tile_rescue()
    _tn_exact_case(X.TN_RESCUE_SHAPE, layout)


@pytest.mark.parametrize("a2_view", [False, True], ids=["a2_contig", "a2_cols"])
@pytest.mark.parametrize("bias", [True, False], ids=["dbias", "nodbias"])
@pytest.mark.parametrize("M,C,paired", X.TN_PAIR_CASES)
def test_gemm_tn_pair_exact(M, C, paired, bias, a2_view):
    """ocn_gemm_tn_accum2: both problems bit-equal to the integer result and to two single launches"""
    assert ((M * 4 * C * C >= 2 ** 31) and C >= 256) == paired  # what sends the pair to the one-launch kernel (gemm.hip)
    g = torch.Generator(device=DEV).manual_seed(M + C)
    a1, a2 = X.int_operand((M, C), X.R_TN, g, DEV), X.int_operand((M, 3 * C), X.R_TN, g, DEV)
    b1, b2 = X.int_operand((M, C), X.R_TN, g, DEV), X.int_operand((M, C), X.R_TN, g, DEV)
    w1, w2 = X.int_operand((C, C), X.BIAS_R, g, DEV, F32), X.int_operand((3 * C, C), X.BIAS_R, g, DEV, F32)
    d1, d2 = X.int_operand((C,), X.BIAS_R, g, DEV, F32), X.int_operand((3 * C,), X.BIAS_R, g, DEV, F32)
    r1, r2 = X.exact_ref(a1, b1, "tn", 1.0, w1), X.exact_ref(a2, b2, "tn", 1.0, w2)
    rb1, rb2 = a1.double().sum(0) + d1.double(), a2.double().sum(0) + d2.double()
    a2v = X.embed(a2, P, 64, 3 * C + 72, NAN)[1] if a2_view else a2
    p1, o1 = X.embed(w1, P, 0, C, X.SENTINEL)
    p2, o2 = X.embed(w2, P, C, 2 * C, X.SENTINEL)
    e1, e2 = d1.clone(), d2.clone()
    ops.gemm_tn_accum2(a1, b1, o1, e1 if bias else None, a2v, b2, o2, e2 if bias else None)
    s1, s2, f1, f2 = w1.clone(), w2.clone(), d1.clone(), d2.clone()
    ops.gemm_tn_accum(a1, b1, s1, f1 if bias else None)
    ops.gemm_tn_accum(a2v, b2, s2, f2 if bias else None)
    tag = f"gemm_tn_accum2 exact [M={M} C={C}]{' a2 view' if a2_view else ''}{' +dbias' if bias else ''}"
    X.assert_bit_equal(tag + " dW1", o1, r1)
    X.assert_bit_equal(tag + " dW2", o2, r2)
    X.assert_bit_equal(tag + " dbias1", e1, X.f32_exact(rb1) if bias else d1)
    X.assert_bit_equal(tag + " dbias2", e2, X.f32_exact(rb2) if bias else d2)
    assert torch.equal(o1, s1) and torch.equal(o2, s2) and torch.equal(e1, f1) and torch.equal(e2, f2), tag + ": pair != two single launches"
    X.assert_outside_untouched(p1, o1, X.SENTINEL, tag + " dW1")
    X.assert_outside_untouched(p2, o2, X.SENTINEL, tag + " dW2")
    X.report(f"{tag}: {'one launch' if paired else 'two-launch fallback'} bit-equal to the integer result and to two single launches")


# ---- host-side refusals: nothing is launched, the output keeps its bits -------------------------------------------------------
def _refused(fn, *outs):
    before = [t.clone() for t in outs]
    with pytest.raises(RuntimeError, match=r"ocn_gemm_\w+ failed \(-1\)"):  # OCN_ERR_INVALID of the entry point's own argument checks
        fn()
    torch.cuda.synchronize()
    for t, b in zip(outs, before):
        assert torch.equal(t, b), "a refused call wrote to its output"


def test_gemm_nt_refuses_what_its_kernels_cannot_take():
    M, N, K = 64, 64, 64
    g = torch.Generator(device=DEV).manual_seed(3)
    big = X.int_operand((M, 2 * K + 40), 8, g, DEV)
    b = X.int_operand((N, K), 8, g, DEV)
    out = torch.full((M, N), X.SENTINEL, device=DEV)
    a = big[:, :K]
    _refused(lambda: ops.gemm_nt(ops.EPI_F32, X.int_operand((M, K + 4), 8, g, DEV)[:, :K], b, out), out)  # lda % 8 != 0
    _refused(lambda: ops.gemm_nt(ops.EPI_F32, a, X.int_operand((N, K + 4), 8, g, DEV)[:, :K], out), out)  # ldb % 8 != 0
    _refused(lambda: ops.gemm_nt(ops.EPI_F32, big[:, 4:4 + K], b, out), out)  # base 8-byte but not 16-byte aligned (column offset 4)
    _refused(lambda: ops.gemm_nt(ops.EPI_F32, a, X.int_operand((N, K + 8), 8, g, DEV)[:, 4:4 + K], out), out)  # the same for B
    obig = torch.full((M, N + 8), X.SENTINEL, device=DEV)
    _refused(lambda: ops.gemm_nt(ops.EPI_F32, a, b, obig[:, 2:2 + N]), obig)  # out on 8 bytes
    _refused(lambda: ops.gemm_nt(ops.EPI_F32, big[:, :48], X.int_operand((N, 48), 8, g, DEV), out), out)  # K % 32 != 0
    wide_b = X.int_operand((N + 8, K), 8, g, DEV)
    tall = torch.full((M + 1, N), X.SENTINEL, device=DEV)
    _refused(lambda: ops.gemm_nt(ops.EPI_F32, a, wide_b, tall.as_strided((M, N + 8), (N, 1))), tall)  # ldc < N
    # the epilogue operands move in 16-byte (bias, resid) and up to 16-byte (aux) pieces: views off those boundaries are refused, never launched
    rbig = torch.zeros(M, N + 8, device=DEV)
    _refused(lambda: ops.gemm_nt(ops.EPI_BIAS_RESID_F32, a, b, obig[:, :N], resid=rbig[:, 2:2 + N]), obig)
    r16 = torch.zeros(M, N + 8, device=DEV, dtype=BF16)
    o16 = torch.full((M, N + 8), X.SENTINEL, device=DEV, dtype=BF16)
    _refused(lambda: ops.gemm_nt(ops.EPI_BIAS_RESID_BF16, a, b, o16[:, :N], resid=r16[:, 4:4 + N]), o16)
    auxbig = torch.full((M, N + 8), 255, device=DEV, dtype=U8)
    _refused(lambda: ops.gemm_nt(ops.EPI_BIAS_GELU, a, b, o16[:, :N], aux=auxbig[:, 4:4 + N]), o16, auxbig)
    _refused(lambda: ops.gemm_nt(ops.EPI_DGELU, a, b, o16[:, :N], aux=auxbig[:, 4:4 + N]), o16)
    _refused(lambda: ops.gemm_nt(ops.EPI_F32, a, b, out, bias=torch.zeros(N + 2, device=DEV)[2:]), out)
    ops.gemm_nt(ops.EPI_F32, a, b, out)  # and the call they were variations of is taken
    X.assert_bit_equal("refusals: the aligned call", out, X.exact_ref(a, b, "nt"))


def test_gemm_tn_refuses_what_its_kernels_cannot_take():
    M = 64
    g = torch.Generator(device=DEV).manual_seed(4)
    for det in (False, True):
        for N, K in ((12, 16), (16, 12)):  # N % 8, K % 8
            dw = torch.full((N, K), X.SENTINEL, device=DEV)
            _refused(lambda: ops.gemm_tn_accum(X.int_operand((M, N), 8, g, DEV), X.int_operand((M, K), 8, g, DEV), dw, deterministic=det), dw)
        dw = torch.full((16, 16), X.SENTINEL, device=DEV)
        a, b = X.int_operand((M, 16), 8, g, DEV), X.int_operand((M, 16), 8, g, DEV)
        _refused(lambda: ops.gemm_tn_accum(X.int_operand((M, 20), 8, g, DEV)[:, :16], b, dw, deterministic=det), dw)  # lda % 8
        _refused(lambda: ops.gemm_tn_accum(a, X.int_operand((M, 20), 8, g, DEV)[:, :16], dw, deterministic=det), dw)  # ldb % 8
        _refused(lambda: ops.gemm_tn_accum(X.int_operand((M, 24), 8, g, DEV)[:, 4:20], b, dw, deterministic=det), dw)  # A on 8 bytes
        _refused(lambda: ops.gemm_tn_accum(a, X.int_operand((M, 24), 8, g, DEV)[:, 4:20], dw, deterministic=det), dw)  # B on 8 bytes
        dw.zero_()
        ops.gemm_tn_accum(a, b, dw, deterministic=det)
        X.assert_bit_equal("refusals: the aligned wgrad", dw, X.exact_ref(a, b, "tn"))
