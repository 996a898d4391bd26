"""The backward's reductions that are not GEMMs on integer operands (tests/reduce_exact.py): the default form (fp32 atomics) and the fixed-order form
(``deterministic=True``) of every op bit-equal to the float64 result -- hence to each other -- and the fixed-order form bit-equal on a second call.
Every output and every accumulated-into tensor is a row range of a taller parent that holds a sentinel; every floating-point input is a row range
of a parent that holds NaN: a store outside a view changes the parent, a neighbour read into a sum shows as NaN.  Accumulated-into tensors start
from integers in [-64, 64], ``dtable`` from zeros (its contract).

What the ops do not let a test do: ``dx32`` / ``dx16`` of ops.layernorm_bwd, ``dpatch`` of ops.embed_assemble_bwd and the fixed-order LayerNorm's
workspace are allocated inside the wrappers, so they cannot be views of a parent and the workspace cannot be handed over poisoned.  The tests free a
NaN-filled block of each such size right before the call, which the caching allocator normally hands straight back (best effort: an output element
never stored, or a slab the finish kernel reads but nobody wrote, then shows as NaN instead of the previous call's identical result).

The loss rows of section 6 are not exact arithmetic: each row of ``det_rows`` is held to the bounds of tests/test_kernels_gpu.py's whole-sum test."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from open_clip_amd import _lib, ops  # noqa: E402
from tests import gemm_exact as X  # noqa: E402
from tests import reduce_exact as R  # noqa: E402
from tests.test_kernels_gpu import rel_l2  # noqa: E402

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
P = X.PAD_ROWS
FORMS = (False, True)  # deterministic


def _2d(t):
    return t if t.dim() == 2 else t.reshape(-1, 1)


def _in(t):
    """a floating-point input on the device, NaN in the parent's rows before and behind it"""
    t2 = _2d(t.to(DEV))
    v = X.embed(t2, P, 0, t2.shape[1], NAN)[1]
    v = v if t.dim() == 2 else v[:, 0]
    assert v.is_contiguous()
    return v


def _acc(t0):
    """(parent, 2-D view, the view in the shape of ``t0``): an output / accumulated-into tensor holding ``t0``, the sentinel around it"""
    t2 = _2d(t0.to(DEV))
    parent, v = X.embed(t2, P, 0, t2.shape[1], X.SENTINEL)
    w = v if t0.dim() == 2 else v[:, 0]
    assert w.is_contiguous()
    return parent, v, w


def _poison(*specs):
    """free NaN-filled blocks of the given (shape, dtype)s: what the next torch.empty of that size normally gets (see the module docstring)"""
    blocks = [torch.full(tuple(shape), NAN, dtype=dtype, device=DEV) for shape, dtype in specs if all(s > 0 for s in shape)]
    del blocks


def _bit_equal(tag, got, want):
    """``want``: the float64 reference (converted without loss) or a tensor of the output's dtype, on either device"""
    X.assert_bit_equal(tag, got, (R.f32_exact(want) if want.dtype == torch.float64 else want).to(got.device))


def _equal(tag, got_parent, got2d, got, want):
    _bit_equal(tag, got, want)
    X.assert_outside_untouched(got_parent, got2d, X.SENTINEL, tag)


def _dt(d):
    return str(d).split(".")[-1]


# ---- 1. token embedding ---------------------------------------------------------------------------------------------------------
def _token(case, packed):
    o = R.token_case(*case, packed=packed)
    B, L, C, V, n = o["B"], o["L"], o["C"], o["V"], o["n"]
    rel = R.chunk_relations(o["runs"])
    assert all(v for k, v in rel.items() if k != "partial_last_chunk")
    dx, tokens, seq_off = _in(o["dx"]), o["tokens"].to(DEV), None
    if packed:
        text = o["plan_text"].to(DEV)
        _, plan, _, _ = ops.seq_pack_plan(text)
        seq_off = plan[:B + 1]
        assert torch.equal(seq_off.cpu(), o["seq_off"])
        _, posidx = ops.seq_pack_rows(text, seq_off, n)
        assert torch.equal(posidx.cpu(), o["posidx"])  # the positions the float64 dpos was indexed by are the op's own
    want_t, want_p = R.f32_exact(o["ref_table"]).to(DEV), R.f32_exact(o["ref_pos"]).to(DEV)
    tag = f"token_embed_bwd exact [{'packed ' if packed else ''}B={B} L={L} C={C} V={V} rows {n} dx {_dt(case[3])}]"
    for det in FORMS:
        for call in range(2 if det else 1):
            tp, t2, t = _acc(torch.zeros(V, C))
            pp, p2, p = _acc(o["dpos0"])
            ops.token_embed_bwd(tokens, dx, t, p, deterministic=det, seq_off=seq_off)
            name = f"{tag} {'fixed-order' if det else 'atomic'} call {call}"
            _equal(name + " dtable", tp, t2, t, want_t)
            _equal(name + " dpos", pp, p2, p, want_p)
            assert not bool(t[o["never"].to(DEV)].any()), name + ": a row of an id that never occurs was written"
    X.report(f"{tag}: atomic and fixed-order (twice) bit-equal; runs vs 64-entry chunks: {', '.join(k for k, v in rel.items() if v)}")


@pytest.mark.parametrize("case", R.TOKEN_DENSE_CASES, ids=lambda c: f"B{c[0]}-L{c[1]}-C{c[2]}-{_dt(c[3])}")
def test_token_embed_bwd_exact_dense(case):
    _token(case, False)


@pytest.mark.parametrize("case", R.TOKEN_PACKED_CASES, ids=lambda c: f"B{c[0]}-L{c[1]}-C{c[2]}-{_dt(c[3])}")
def test_token_embed_bwd_exact_packed(case):
    _token(case, True)


# ---- 2. image embedding ---------------------------------------------------------------------------------------------------------
def _assemble(o, inv, tag):
    B, G, K, C = o["B"], o["G"], o["K"], o["C"]
    demb = _in(o["demb"])
    want_patch = o["ref_patch"].to(DEV)
    for det in FORMS:
        for call in range(2 if det else 1):
            pp, p2, p = _acc(o["dpos0"])
            cp, c2, c = _acc(o["dcls0"])
            _poison(((B * K, C), BF16))
            dpatch = ops.embed_assemble_bwd(demb, p, c, B, G, C, deterministic=det, inv=inv, K=None if inv is None else K)
            name = f"{tag} {'fixed-order' if det else 'atomic'} call {call}"
            _equal(name + " dpos", pp, p2, p, o["ref_pos"])
            _equal(name + " dcls", cp, c2, c, o["ref_cls"])
            _bit_equal(name + " dpatch", dpatch, want_patch)  # every row written: a NaN row would differ
    X.report(f"{tag}: dpos / dcls / dpatch, atomic and fixed-order (twice) bit-equal")


@pytest.mark.parametrize("B,G,C", R.ASSEMBLE_FULL_CASES)
def test_embed_assemble_bwd_exact(B, G, C):
    _assemble(R.assemble_case(B, G, C), None, f"embed_assemble_bwd exact [B={B} G={G} C={C}]")


@pytest.mark.parametrize("B,G,K,C,step", R.ASSEMBLE_KEEP_CASES)
def test_embed_assemble_bwd_exact_with_keep(B, G, K, C, step):
    """the planned keep where it leaves a (chunk, position) unkept (tests/reduce_exact.py::keep_is_good), else the hand-built one; then the
    hand-built one (any order) through ops.patch_keep_inverse in every case"""
    keep, inv = ops.patch_keep_plan(1234 + B, B, G, K, DEV)
    planned = R.keep_is_good(keep.cpu(), G)
    if planned:
        _assemble(R.assemble_case(B, G, C, keep.cpu()), inv, f"embed_assemble_bwd exact [B={B} G={G} K={K} C={C} planned keep]")
    hand = R.hand_keep(B, G, K, step)
    inv = ops.patch_keep_inverse(hand.to(DEV), G)
    _assemble(R.assemble_case(B, G, C, hand), inv, f"embed_assemble_bwd exact [B={B} G={G} K={K} C={C} hand-built keep{'' if planned else '; the planned one left no hole'}]")


# ---- 3. column sums -------------------------------------------------------------------------------------------------------------
def _colsum(o, tag, forms):
    x = _in(o["x"])
    for det in forms:
        for call in range(2 if det else 1):
            op, o2, out = _acc(o["out0"])
            ops.colsum_f32(x, out, deterministic=det)
            _equal(f"{tag} {'fixed-order' if det else 'atomic'} call {call}", op, o2, out, o["ref"])


@pytest.mark.parametrize("C", R.COLSUM_C)
def test_colsum_f32_exact(C):
    for Rr in R.COLSUM_R:
        _colsum(R.colsum_case(Rr, C), f"colsum_f32 exact [R={Rr} C={C}]", FORMS)
    X.report(f"colsum_f32 exact [R in {list(R.COLSUM_R)} x C={C}]: atomic and fixed-order (twice) bit-equal")


def test_colsum_f32_fixed_order_form_adds_once_per_column():
    _colsum(R.colsum_single_add_case(), "colsum_f32 [65 x 65] one addition into 2^24", (True,))
    X.report("colsum_f32 fixed-order [R=65 C=65]: out = 2^24 + 2 -- one addition per column (two additions of 1 would each round back to 2^24)")


# ---- 4. LayerNorm backward ------------------------------------------------------------------------------------------------------
class _Worst:
    def __init__(self):
        self.dx = self.dx16 = self.dcol = 0.0


def _ln_ws_floats(M, C):
    return int(_lib.load().ocn_layernorm_bwd_det_workspace_floats(M, C))


def _ln_run(o, dev, tag, x_dt, dy_dt, dres_dt, dcol, want_f32, want_bf16, worst):
    """both forms of one dtype combination; ``dev``: the case's tensors on the device (inputs inside NaN parents)"""
    M, C = o["M"], o["C"]
    with_dres = dres_dt is not None
    ref_dx = o["ref_dx"][with_dres]
    for det in FORMS:
        for call in range(2 if det else 1):
            wp, w2, dw = _acc(o["dw0"])
            bp, b2, db = _acc(o["db0"])
            cp, c2, dc = _acc(o["dcol0"]) if dcol else (None, None, None)
            _poison(((M, C), F32) if want_f32 else ((0,), F32), ((M, C), BF16) if want_bf16 else ((0,), BF16), ((_ln_ws_floats(M, C) if det else 0,), F32))
            dx32, dx16 = ops.layernorm_bwd(dev["dy", dy_dt], dev["x", x_dt], dev["w"], dev["mean"], dev["rstd"], dw, db, dres=dev["dres", dres_dt] if with_dres else None,
                                           want_f32=want_f32, want_bf16=want_bf16, dcol=dc, deterministic=det)
            name = f"{tag} {'fixed-order' if det else 'atomic'} call {call}"
            _equal(name + " dw", wp, w2, dw, o["ref_dw"])
            _equal(name + " db", bp, b2, db, o["ref_db"])
            assert (dx32 is not None) == want_f32 and (dx16 is not None) == want_bf16
            if o["pow2"]:
                want32 = R.f32_exact(ref_dx).to(DEV)
                if want_f32:
                    _bit_equal(name + " dx32", dx32, want32)
                if want_bf16:
                    _bit_equal(name + " dx16", dx16, R.rne_bf16(want32))
                if dcol:
                    _equal(name + " dcol", cp, c2, dc, o["ref_dcol"][with_dres])
                continue
            # 1 / C is not a power of two: dx and dcol under the bounds of test_layernorm, against the float64 formula
            ref = ref_dx.to(DEV)
            if want_f32:
                r = rel_l2(dx32, ref)
                worst.dx = max(worst.dx, r)
                assert torch.isfinite(dx32).all() and r <= 1e-5, f"{name} dx32: rel_l2 {r:.3e} > 1e-5"
            if want_bf16:
                err = (dx16.double() - ref).abs()
                bound = ref.abs() * 2.0 ** -7 + 1e-6 * float(ref.abs().max())
                worst.dx16 = max(worst.dx16, float((err / bound).max()))
                assert torch.isfinite(dx16.float()).all() and bool((err <= bound).all()), f"{name} dx16: {int((err > bound).sum())} elements beyond one bf16 rounding"
            if dcol:
                want = o["ref_dcol"][with_dres].to(DEV)
                r = float((dc.double() - want).norm() / (want - o["dcol0"].to(DEV).double()).norm())  # relative to the sums alone, not to sums + initial contents
                worst.dcol = max(worst.dcol, r)
                assert r <= 1e-4, f"{name} dcol: rel_l2 {r:.3e} > 1e-4"
                X.assert_outside_untouched(cp, c2, X.SENTINEL, name + " dcol")


class _Dev(dict):
    """the case's inputs on the device, converted on first use: dev["dy", BF16]"""
    def __init__(self, o):
        super().__init__()
        self.o = o
        for k in ("w", "mean", "rstd"):
            self[k] = _in(o[k])

    def __missing__(self, key):
        name, dt = key
        self[key] = _in(self.o[name].to(dt))
        return self[key]


def _ln_tail(o, worst):
    return "dx / dx16 / dcol bit-equal too" if o["pow2"] else f"dx rel_l2 <= {worst.dx:.1e} (1e-5), dx16 <= {worst.dx16:.2f} of one bf16 rounding, dcol rel_l2 <= {worst.dcol:.1e} (1e-4)"


@pytest.mark.parametrize("C", R.LN_POW2_C + R.LN_OTHER_C)
def test_layernorm_bwd_exact_fp32_stream(C):
    worst, n = _Worst(), 0
    for M in R.LN_M:
        o = R.ln_case(M, C)
        dev = _Dev(o)
        for dy_dt in (F32, BF16):
            for dres_dt in (None, F32):
                for dcol in (False, True):
                    _ln_run(o, dev, f"layernorm_bwd exact [M={M} C={C} x fp32 dy {_dt(dy_dt)} dres {_dt(dres_dt)} dcol {int(dcol)}]", F32, dy_dt, dres_dt, dcol, True, True, worst)
                    n += 1
    X.report(f"layernorm_bwd exact [M in {list(R.LN_M)} C={C} x fp32]: {n} combinations of dy fp32 | bf16, dres none | fp32, dcol on | off; atomic and fixed-order "
             f"(twice): dw / db bit-equal, {_ln_tail(o, worst)}")


# (C, want_bf16): the pipelined two-rows-in-flight kernel wants dx16 and C = NV * 256 <= 1280; everything else on the bf16 stream is the one-row kernel
LN_BF16_CASES = ((192, True), (256, True), (512, True), (512, False), (768, True), (1024, True), (1280, True))


@pytest.mark.parametrize("C,want_bf16", LN_BF16_CASES)
def test_layernorm_bwd_exact_bf16_stream(C, want_bf16):
    worst, n = _Worst(), 0
    for M in R.LN_M:
        o = R.ln_case(M, C)
        dev = _Dev(o)
        for dres_dt in (None, BF16, F32):
            for want_f32 in ((True, False) if want_bf16 else (True,)):
                _ln_run(o, dev, f"layernorm_bwd exact [M={M} C={C} x bf16 dres {_dt(dres_dt)} dx32 {int(want_f32)} dx16 {int(want_bf16)}]", BF16, BF16, dres_dt, False,
                        want_f32, want_bf16, worst)
                n += 1
    pipelined = want_bf16 and C % 256 == 0 and C <= 1280
    X.report(f"layernorm_bwd exact [M in {list(R.LN_M)} C={C} x bf16, {'pipelined' if pipelined else 'one-row'} kernel]: {n} combinations of dres none | bf16 | fp32, dx32 on | off; "
             f"atomic and fixed-order (twice): dw / db bit-equal, {_ln_tail(o, worst)}")


@pytest.mark.parametrize("C,x_dt", [(256, BF16), (1280, BF16), (768, F32)], ids=lambda v: _dt(v) if isinstance(v, torch.dtype) else str(v))
def test_layernorm_bwd_exact_every_wave_reaches_a_third_row(C, x_dt):
    """M = 2 * CUs * 16 + 37: the grid is capped at one workgroup per CU with at most 16 waves, so every wave walks more than two strides -- the
    pipelined kernel's refetch two strides ahead and its clamped fetch row past M are both exercised"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M = R.ln_big_m(cus)
    o = R.ln_case(M, C, dcol=False)
    dev, worst = _Dev(o), _Worst()
    if x_dt == BF16:
        _ln_run(o, dev, f"layernorm_bwd exact [M={M} C={C} x bf16 dres bf16]", BF16, BF16, BF16, False, True, True, worst)
    else:
        _ln_run(o, dev, f"layernorm_bwd exact [M={M} C={C} x fp32 dy bf16 dres fp32 dcol]", F32, BF16, F32, True, True, True, worst)
    X.report(f"layernorm_bwd exact [M={M} = 2 x {cus} CUs x 16 waves + 37, C={C} x {_dt(x_dt)}]: atomic and fixed-order (twice): dw / db bit-equal, {_ln_tail(o, worst)}")


# ---- 5. squared gradient norm ---------------------------------------------------------------------------------------------------
def test_sumsq_accum_exact():
    for n in R.SUMSQ_N:
        o = R.sumsq_case(n)
        op, o2, out = _acc(torch.tensor([o["out0"]]))
        ops.sumsq_accum(_in(o["x"]), out)
        _equal(f"sumsq_accum exact [n={n}]", op, o2, out, o["ref"])
    X.report(f"sumsq_accum exact [n in {list(R.SUMSQ_N)}]: bit-equal to the integer sum of squares + the initial contents")


@pytest.mark.parametrize("det", FORMS, ids=["atomic", "fixed-order"])
def test_adamw_clip_norm_exact(det):
    """only the norm: the update itself stays with tests/test_kernels_gpu.py and tests/test_optim_parent_gpu.py"""
    from open_clip_amd.optim import NativeAdamW
    g = torch.Generator().manual_seed(5)
    params = [torch.nn.Parameter(torch.randn(sh, generator=g).to(DEV)) for sh in R.CLIP_SHAPES]
    opt = NativeAdamW(params, lr=5e-4, grad_clip_norm=0.7, deterministic=det)
    for step in range(2):
        o = R.clip_case(step)
        for i, (p, gr) in enumerate(zip(params, o["grads"])):
            if i in R.CLIP_OFFSET_VIEWS:  # a gradient view at a 4-byte offset, NaN in front of it
                buf = torch.full((gr.numel() + 1,), NAN, device=DEV)
                buf[1:].copy_(gr.flatten())
                p.grad = buf[1:].view(p.shape)
            else:
                p.grad = gr.to(DEV)
        opt.step()
        _bit_equal(f"NativeAdamW last_grad_norm_sq [{'fixed-order' if det else 'atomic'} step {step}]", opt.last_grad_norm_sq.reshape(-1), o["ref"])
    X.report(f"NativeAdamW grad norm exact [{len(params)} tensors, two at a 4-byte offset, {'fixed-order' if det else 'atomic'}]: last_grad_norm_sq bit-equal to the integer sum of squares, 2 steps")


# ---- 6. loss rows, judged per row -----------------------------------------------------------------------------------------------
def _g_buffer(Rr, N):
    ldg = (N + 63) // 64 * 64
    return X.embed_out((Rr, ldg), BF16, DEV, P, 0, ldg)


def _check_g(tag, gp, G, N):
    X.assert_outside_untouched(gp, G, X.SENTINEL, tag + " G")
    assert torch.isfinite(G[:, :N].float()).all() and torch.isnan(G[:, N:].float()).all(), tag + ": G not written in [0, N) alone"


def _agree(tag, rows_sum64, atomic, rel):
    for k, name in enumerate(("loss", "dscale", "dbias")[:atomic.numel()]):
        a, b = float(rows_sum64[k]), float(atomic[k])
        assert abs(a - b) <= rel[k] * abs(a), f"{tag} {name}: float64 sum of det_rows {a:.9e} vs the atomic call {b:.9e}"


@pytest.mark.parametrize("peaked", [False, True], ids=["gaussian", "peaked"])
@pytest.mark.parametrize("Rr,N,off", R.LOSS_SHAPES)
def test_loss_rows_per_row(Rr, N, off, peaked):
    """every row of ``det_rows`` against float64 torch on the same fp32 logits: loss within 1e-5 relative + 1e-7 * loss_scale, d/d logit_scale and
    d/d bias within 1e-4 of the row's sum of |term| (the bounds of test_loss_row_kernels, on the scale that is free of cancellation); the float64 sum
    of the rows agrees with the atomic call under that test's bounds (1e-5, 1e-4, 1e-4 relative).

    One bound is not the issue's: d/d logit_scale of a PEAKED cross-entropy row.  fp32 cannot hold softmax(label) - 1 there (the row's exp sum is
    1 + ~1e-13 = 1), so the plain fp32 torch statement of the row itself misses float64 by 0.9601 / 0.8738 / 0.8600 / 0.8236 of the row's sum of |term|
    at the four shapes (tests/test_reduce_exact.py measures it on the CPU) -- 9.6e3 times the 1e-4 bound, on sums that are ~1e-12 of a Gaussian
    row's.  The kernel, which states the row the same way, misses by the same amount (measured on the MI355X: 0.250 / 0.227 / 0.224 / 0.214 of the
    bound below, i.e. 0.96 .. 0.82 of the row's sum of |term|).  The bound there is 4 x 0.961 of the row's sum of |term|
    (tests/reduce_exact.py::CE_PEAKED_DSCALE_BOUND): four times the fp32 statement's own error, not a figure taken from the kernel."""
    lg = R.loss_logits(Rr, N, off, peaked)
    logits = _in(lg)
    tag = f"loss rows [{Rr} x {N} off {off} {'peaked' if peaked else 'gaussian'}]"
    parts = []
    for kind in ("ce", "siglip", "siglip_neg"):
        ref, bounds, (ls, gs, inv_s) = R.loss_rows_reference(lg, off, kind, peaked_bound=peaked)
        rp, rows = X.embed_out((Rr, 3), F32, DEV, P, 0, 3)
        gp, G = _g_buffer(Rr, N)
        acc = torch.zeros(3, device=DEV)
        if kind == "ce":
            ops.softmax_ce_rows(logits, G, N, off, ls, gs, inv_s, acc[0:1], acc[1:2], det_rows=rows)
        else:
            ops.siglip_rows(logits, G, N, off, int(kind == "siglip_neg"), R.SIGLIP_BIAS, ls, gs, inv_s, acc[0:1], acc[1:2], acc[2:3], det_rows=rows)
        assert not bool(acc.any()), f"{tag} {kind}: the det_rows form added to the atomic accumulators as well"
        X.assert_outside_untouched(rp, rows, X.SENTINEL, f"{tag} {kind} det_rows")
        _check_g(f"{tag} {kind}", gp, G, N)
        assert torch.isfinite(rows).all(), f"{tag} {kind}: a row was not written"
        ratio = R.worst_ratio(rows.cpu(), ref, bounds)
        parts.append(f"{kind} loss {ratio[0]:.2e} dscale {ratio[1]:.2e}" + (f" dbias {ratio[2]:.2e}" if kind != "ce" else ""))
        print(f"{tag} {kind}: worst ratio to the bound: loss {ratio[0]:.3e} dscale {ratio[1]:.3e} dbias {ratio[2]:.3e}")
        assert max(ratio) <= 1.0, f"{tag} {kind}: worst ratio to the bound (loss, dscale, dbias) = {ratio}"
        # the same call in its atomic form: the sums of the rows, under the bounds of test_loss_row_kernels
        gp2, G2 = _g_buffer(Rr, N)
        if kind == "ce":
            ops.softmax_ce_rows(logits, G2, N, off, ls, gs, inv_s, acc[0:1], acc[1:2])
        else:
            ops.siglip_rows(logits, G2, N, off, int(kind == "siglip_neg"), R.SIGLIP_BIAS, ls, gs, inv_s, acc[0:1], acc[1:2], acc[2:3])
        _check_g(f"{tag} {kind} atomic", gp2, G2, N)
        assert torch.equal(G2[:, :N], G[:, :N])
        _agree(f"{tag} {kind}", rows.double().sum(0).cpu(), acc.cpu()[:2 if kind == "ce" else 3], (1e-5, 1e-4, 1e-4))
    X.report(f"{tag}: worst ratio of a row to its bound{' (cross-entropy dscale: 4 x the fp32 statement)' if peaked else ''}: {'; '.join(parts)}; sums of the rows agree with the atomic form")
