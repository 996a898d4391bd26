"""CPU: the constructions, references and guards of the exact-arithmetic attention tests (tests/attn_exact.py, run on the MI355X by
tests/test_attn_exact_gpu.py), checked alone.  For every case table entry: the guards hold (winning score 0, masked scores <= -150 / log2(e), counts
powers of two, P / dS / outputs lossless in bf16, every reference a multiple of its grid step, fp32 noise bound below g / 16) and the reference agrees
with a plain float64 softmax-attention autograd of the same inputs to 1e-12 -- it is attention, not a restatement of the construction.  The comparison
logic is shown to bite: a causal mask shifted by one key, one padded key counted, two heads swapped, one grid step, a NaN each make it fail."""
import math

import pytest
import torch

from tests import attn_exact as X

F64 = torch.float64


def _autograd_head(q, k, v, do, vis):
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    s = (q @ k.t()) * X.SCALE
    s = s.masked_fill(~vis, -math.inf)
    out = torch.softmax(s, -1) @ v
    out.backward(do)
    return out.detach(), torch.logsumexp(s, -1).detach(), q.grad, k.grad, v.grad


def _close(a, b, what):
    err = float((a - b).abs().max()) if a.numel() else 0.0
    assert err <= 1e-12 * max(1.0, float(b.abs().max()) if b.numel() else 1.0), f"{what}: reference vs float64 autograd differ by {err:.3e}"


@pytest.mark.parametrize("c", X.SELF_CASES + X.PACKED_CASES, ids=X.case_id)
def test_self_case_guards_hold_and_reference_is_attention(c):
    inp = X.build_self(c)
    ref = X.reference_self(inp)  # strict: every guard
    B, H, D, L, C = c["B"], c["H"], c["D"], c["L"], inp["C"]
    assert inp["qkv"].to(torch.bfloat16).to(F64).equal(inp["qkv"]) and inp["dout"].to(torch.bfloat16).to(F64).equal(inp["dout"])
    assert float(inp["qkv"][:, 2 * C:].abs().max()) <= X.V_R and float(inp["dout"].abs().max()) == 1.0
    for b in range(B):
        n, r0 = inp["lens"][b], inp["off"][b]
        for h in range(H):
            col = h * D
            q, k, v = (inp["qkv"][r0:r0 + n, t * C + col:t * C + col + D] for t in range(3))
            vis = X._vis_self(n, c["causal"])
            out, lse, dq, dk, dv = _autograd_head(q, k, v, inp["dout"][r0:r0 + n, col:col + D], vis)
            tag = f"{X.case_id(c)} seq {b} head {h}"
            _close(ref["out"][r0:r0 + n, col:col + D], out, tag + " out")
            _close(ref["lse"][b, h, :n], lse, tag + " lse")
            for t, g in enumerate((dq, dk, dv)):
                _close(ref["dqkv"][r0:r0 + n, t * C + col:t * C + col + D], g, tag + " d" + "qkv"[t])
            # the sets the construction meant are the keys the reference found
            s = (q @ k.t()) * X.SCALE
            for i, S in enumerate(inp["sets"][(b, h)]):
                assert ((s[i] == 0) & vis[i]).nonzero()[:, 0].tolist() == S and int(ref["count"][b, h, i]) == len(S)
            counts = {len(S) for S in inp["sets"][(b, h)]}
            assert counts == {1} if c["family"] == "selection" else (counts <= {1, 2, 4, 8} and (n < 16 or {2, 4, 8} <= counts))
            sel_last = [i for i, S in enumerate(inp["sets"][(b, h)]) if n - 1 in S]
            assert len(sel_last) >= 1 and n - 1 in sel_last  # a padded copy of the last key that got weight changes these counts
            if c["causal"]:  # decoys: future keys that score 0 -- key i + 1 of every block's last query among them
                dec = [i for i in range(n - 1) if float(s[i, i + 1]) == 0.0]
                assert len(dec) >= (n - 1) // 4, f"{tag}: only {len(dec)} queries with key i + 1 as a decoy"
                assert all(i in dec for i in range(31, n - 1, 32)), f"{tag}: no decoy behind a block's last query"
            if b + 1 < B:  # the next sequence's keys take the whole row of every query of this one
                kn = inp["qkv"][inp["off"][b + 1]:inp["off"][b + 1] + inp["lens"][b + 1], C + col:C + col + D]
                assert float(((q @ kn.t()) * X.SCALE).min()) >= 2048 * X.SCALE
            if b > 0:  # ... and the previous sequence's keys none
                kp = inp["qkv"][inp["off"][b - 1]:r0, C + col:C + col + D]
                assert float(((q @ kp.t()) * X.SCALE).max()) <= 0.0
    if c["family"] == "uniform":  # every head of every sequence: sets with each 32-key block seam (hence each 64-key chunk seam) inside
        for (b, h), sel in inp["sets"].items():
            seams = {j for S in sel for j in S if j % 32 == 0 and j > 0 and j - 1 in S}
            assert seams >= {32 * m for m in X.seams_to_straddle(inp["lens"][b], c["causal"])}, f"seq {b} head {h}: sets straddle only the seams {sorted(seams)}"
    assert X.seams_to_straddle(63, False) == [] and X.seams_to_straddle(63, True) == [1] and X.seams_to_straddle(129, False) == [1, 2, 3, 4]
    if c["family"] == "selection":
        assert float(ref["dqkv"][:, :2 * C].abs().max()) == 0.0 and float(ref["lse"][~ref["lse"].isnan()].abs().max()) == 0.0
    elif L >= 16:  # nonzero dyadic dQ and dK
        assert float(ref["dqkv"][:, :C].abs().max()) >= X.G_DQ and float(ref["dqkv"][:, C:2 * C].abs().max()) >= X.G_DK


def test_case_tables_cover_what_the_kernels_dispatch_on():
    res = {(c["L"], c["causal"], c["family"]) for c in X.RESIDENT_CASES}
    assert res == {(L, cz, f) for L in (1, 31, 32, 33, 50, 64, 65, 77, 96, 97, 128) for cz in (False, True) for f in X.FAMILIES}
    assert {(c["L"], c["causal"]) for c in X.MIXED_CASES} == {(L, cz) for L in (129, 257, 320, 321) for cz in (False, True)}
    assert {(c["D"], c["L"]) for c in X.STREAMED_CASES} == {(D, L) for D in (80, 88, 96, 104, 112, 128) for L in (63, 64, 65, 129, 257)}
    for D in X.STREAMED_D:
        assert len({c["L"] for c in X.STREAMED_CASES if c["D"] == D and c["causal"]}) >= 2
    assert {c["knobs"] for c in X.KNOB_CASES} == {((2, 6),), ((7, 1),)} and {c["L"] for c in X.KNOB_CASES if c["knobs"] == ((7, 1),)} == {50, 77}
    assert all(c["B"] in (2, 3) and c["H"] in (2, 3) for c in X.SELF_CASES) and all(c["H"] >= 2 for c in X.STREAMED_CASES)
    assert sorted(X.PACKED_LENS) == [1, 9, 32, 33, 64, 77] and list(X.PACKED_LENS) != sorted(X.PACKED_LENS)
    order, counts = X.bucket_layout(X.PACKED_LENS, 77)
    assert counts == [3, 2, 1] and order.tolist() == [1, 2, 5, 3, 4, 0]
    assert {c["mode"] for c in X.POOLED_CASES} == {"image_cls", "long", "text_packed", "text_dense"}
    ids = [X.case_id(c) for c in X.SELF_CASES + X.PACKED_CASES + X.POOLED_CASES]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("c", X.PACKED_CASES[::2], ids=X.case_id)
def test_packed_case_and_its_dense_twin_have_the_same_rows(c):
    inp = X.build_self(c)
    ref = X.reference_self(inp)
    twin = X.dense_twin(inp)
    tref = X.reference_self(twin)
    L = c["L"]
    for b, n in enumerate(inp["lens"]):
        r0 = inp["off"][b]
        assert torch.equal(twin["qkv"][b * L:b * L + n], inp["qkv"][r0:r0 + n])
        assert torch.equal(tref["out"][b * L:b * L + n], ref["out"][r0:r0 + n]) and torch.equal(tref["dqkv"][b * L:b * L + n], ref["dqkv"][r0:r0 + n])
        assert torch.equal(tref["lse"][b, :, :n], ref["lse"][b, :, :n])
        if b + 1 < len(inp["lens"]):  # every sequence's successor starts with decoy keys, packed and dense
            C, D = inp["C"], c["D"]
            for rows in (inp["qkv"][inp["off"][b + 1]:inp["off"][b + 1] + 1], twin["qkv"][(b + 1) * L:(b + 1) * L + 1]):
                assert float((inp["qkv"][r0:r0 + n, :D] @ rows[:, C:C + D].t()).min()) >= 2048


@pytest.mark.parametrize("c", X.POOLED_CASES, ids=X.case_id)
def test_pooled_case_guards_hold_and_reference_is_attention(c):
    inp = X.build_pooled(c)
    ref = X.reference_pooled(inp)
    B, H, D, C = c["B"], c["H"], c["D"], inp["C"]
    for b in range(B):
        n, r0 = inp["lens"][b], inp["off"][b]
        vis_max = c["qpos"][b] if c["causal"] else n - 1
        assert int(inp["rows"][b]) == r0 + c["qpos"][b]
        for h in range(H):
            col = h * D
            k, v = inp["kv"][r0:r0 + n, col:col + D], inp["kv"][r0:r0 + n, C + col:C + col + D]
            q = inp["q"][b:b + 1, col:col + D]
            vis = (torch.arange(n) <= vis_max)[None, :]
            out, lse, dq, dk, dv = _autograd_head(q, k, v, inp["dout"][b:b + 1, col:col + D], vis)
            tag = f"{X.case_id(c)} seq {b} head {h}"
            _close(ref["out"][b, col:col + D], out[0], tag + " out")
            _close(ref["lse"][b * H + h], lse[0], tag + " lse")
            _close(ref["dq"][b, col:col + D], dq[0], tag + " dq")
            _close(ref["dkv"][r0:r0 + n, col:col + D], dk, tag + " dk")
            _close(ref["dkv"][r0:r0 + n, C + col:C + col + D], dv, tag + " dv")
            s = (q @ k.t())[0]
            assert bool((s[vis_max + 1:] == 0).all()), "rows behind the pooled token must be decoys (score 0)"
            if b + 1 < B:
                kn = inp["kv"][inp["off"][b + 1]:inp["off"][b + 1] + inp["lens"][b + 1], col:col + D]
                assert float((q @ kn.t()).min()) >= 2048
    if c["mode"] == "text_dense":
        assert int(ref["zero_rows"].sum()) == sum(c["L"] - 1 - p for p in c["qpos"]) > 0
    if c["family"] == "uniform":
        assert float(ref["dq"].abs().max()) > 0 and int(ref["count"].max()) >= 4


# ---- the comparison logic bites ---------------------------------------------------------------------------------------------------------------
def _as_got(ref, inp):
    L = inp["case"]["L"]
    lse = torch.where(ref["lse"].isnan(), torch.zeros_like(ref["lse"]), ref["lse"])  # (rows a packed sequence does not have: never compared)
    return {"out": X.as_kernel_output(ref["out"]), "dqkv": X.as_kernel_output(ref["dqkv"]), "lse": X.as_kernel_output(lse, torch.float32).reshape(-1)}


_BITE = [c for c in X.RESIDENT_CASES if c["L"] == 77 and c["causal"]] + [c for c in X.STREAMED_CASES if (c["D"], c["L"]) == (88, 65)] + X.PACKED_CASES[::2]


@pytest.mark.parametrize("c", _BITE, ids=X.case_id)
def test_a_causal_mask_shifted_by_one_key_fails(c):
    inp = X.build_self(c)
    ref = X.reference_self(inp)
    X.check_self("right", _as_got(ref, inp), ref, inp)
    wrong = X.reference_self(inp, strict=False, causal_shift=1)  # key i + 1 visible
    moved = (wrong["count"] != ref["count"]).sum()
    assert int(moved) >= sum(n - 1 for n in inp["lens"]) * c["H"] // 4  # every query with a decoy behind it
    with pytest.raises(AssertionError, match=" out: differs from the exact result"):
        X.check_self("shifted", _as_got(wrong, inp), ref, inp)
    for nm, fn in (("lse", lambda g: X.assert_lse("lse", g["lse"], ref["lse"], ref["count"])),
                   ("dV", lambda g: X.assert_exact("dV", g["dqkv"][:, 2 * inp["C"]:], ref["dqkv"][:, 2 * inp["C"]:], c["D"]))):
        with pytest.raises(AssertionError):
            fn(_as_got(wrong, inp))
    if c["family"] == "uniform":
        for t, g in ((0, X.G_DQ), (1, X.G_DK)):
            C = inp["C"]
            with pytest.raises(AssertionError, match="off the grid"):
                X.assert_on_grid("d" + "qk"[t], _as_got(wrong, inp)["dqkv"][:, t * C:(t + 1) * C], ref["dqkv"][:, t * C:(t + 1) * C], g, c["D"])


@pytest.mark.parametrize("c", [c for c in X.RESIDENT_CASES if c["L"] in (50, 77)] + [c for c in X.STREAMED_CASES if (c["D"], c["L"]) == (104, 63)]
                         + X.PACKED_CASES[::2], ids=X.case_id)
def test_one_padded_key_that_gets_weight_fails(c):
    inp = X.build_self(c)
    ref = X.reference_self(inp)
    wrong = X.reference_self(inp, strict=False, dup_last_key=True)  # the copy of the last key in the tail of the last block, counted
    got = _as_got(wrong, inp)
    with pytest.raises(AssertionError, match="beyond 8 fp32 ulps"):  # the count of every query that selects the last key
        X.assert_lse("lse", got["lse"], ref["lse"], ref["count"])
    with pytest.raises(AssertionError):
        X.check_self("padded", got, ref, inp)
    if c["family"] == "uniform":  # (a one-hot row keeps its output -- twice the same key at half the weight: there only lse notices)
        with pytest.raises(AssertionError, match=" out: differs"):
            X.assert_exact("padded out", got["out"], ref["out"], c["D"])
        with pytest.raises(AssertionError, match="dV: differs"):
            X.assert_exact("dV", got["dqkv"][:, 2 * inp["C"]:], ref["dqkv"][:, 2 * inp["C"]:], c["D"])


@pytest.mark.parametrize("c", [X.RESIDENT_CASES[16], X.RESIDENT_CASES[19], X.STREAMED_CASES[10], X.STREAMED_CASES[33]], ids=X.case_id)
def test_two_heads_swapped_fails(c):
    inp = X.build_self(c)
    ref = X.reference_self(inp)
    D, C = c["D"], inp["C"]
    # in the inputs' copy: V of heads 0 and 1 exchanged
    swapped = dict(inp, qkv=inp["qkv"].clone())
    swapped["qkv"][:, 2 * C:2 * C + D], swapped["qkv"][:, 2 * C + D:2 * C + 2 * D] = inp["qkv"][:, 2 * C + D:2 * C + 2 * D], inp["qkv"][:, 2 * C:2 * C + D]
    with pytest.raises(AssertionError, match=" out: differs"):
        X.check_self("heads", _as_got(X.reference_self(swapped, strict=False), inp), ref, inp)
    # in the outputs: heads 0 and 1 of one tensor exchanged
    for key, width in (("out", C), ("dqkv", 3 * C)):
        got = _as_got(ref, inp)
        for base in range(0, width, C):
            got[key][:, base:base + D], got[key][:, base + D:base + 2 * D] = got[key][:, base + D:base + 2 * D].clone(), got[key][:, base:base + D].clone()
        with pytest.raises(AssertionError):
            X.check_self("heads", got, ref, inp)
    got = _as_got(ref, inp)
    lse = got["lse"].reshape(c["B"], c["H"], c["L"])
    if c["family"] == "uniform":
        got["lse"] = torch.stack([lse[:, 1], lse[:, 0]] + [lse[:, h] for h in range(2, c["H"])], 1).reshape(-1)
        with pytest.raises(AssertionError, match="ulps"):
            X.check_self("heads", got, ref, inp)


def test_pooled_comparison_bites():
    c = X.POOLED_CASES[7]
    assert c["mode"] == "text_dense" and c["family"] == "uniform"
    inp = X.build_pooled(c)
    ref = X.reference_pooled(inp)

    def got_of(r):
        return {"out": X.as_kernel_output(r["out"]), "dq": X.as_kernel_output(r["dq"]), "dkv": X.as_kernel_output(r["dkv"]),
                "lse": X.as_kernel_output(r["lse"], torch.float32)}
    X.check_pooled("right", got_of(ref), ref, inp)
    wrong = dict(inp, case=dict(c, qpos=tuple(p + 1 for p in c["qpos"])))  # the mask one key late: the first decoy row visible
    wref = X.reference_pooled(wrong, strict=False)
    assert int((wref["count"] != ref["count"]).sum()) == c["B"] * c["H"]
    with pytest.raises(AssertionError, match=" out: differs"):
        X.check_pooled("late", got_of(wref), ref, inp)
    g = got_of(ref)
    g["dkv"][int(ref["zero_rows"].nonzero()[0]), 3] = 2.0 ** -20
    with pytest.raises(AssertionError):
        X.check_pooled("dirty zero row", g, ref, inp)


def test_helpers_detect_what_they_are_for():
    want = torch.tensor([[0.0, 0.5, -3.0, 4.0]], dtype=F64)
    got = X.as_kernel_output(want)
    X.assert_exact("ok", got, want, 4)
    assert X.assert_on_grid("ok", got, want, X.G_DQ, 4) == 0.0
    assert X.assert_on_grid("noise", X.as_kernel_output(torch.tensor([[2.0 ** -10]], dtype=F64)), torch.zeros(1, 1, dtype=F64), X.G_DQ, 1) == 2.0 ** -10
    with pytest.raises(AssertionError, match="off the grid"):
        X.assert_on_grid("step", X.as_kernel_output(want + torch.tensor([0, 0, 0, X.G_DQ * 2])), want, X.G_DQ, 4)  # bf16 next to 4.0: steps of 1/32
    with pytest.raises(AssertionError, match=r"1 of 4 elements; first \(row, head, dim\): \[\(0, 0, 1\)\]"):
        X.assert_exact("step", X.as_kernel_output(want + torch.tensor([0, X.G_OUT, 0, 0])), want, 4)
    bad = got.clone()
    bad[0, 2] = math.nan
    for fn in (lambda: X.assert_exact("nan", bad, want, 4), lambda: X.assert_on_grid("nan", bad, want, X.G_DQ, 4)):
        with pytest.raises(AssertionError, match="non-finite"):
            fn()
    # lse: ln 8 is met within 8 ulps, ln 9 is not; an unwritten value (NaN) is not
    w, cnt = torch.tensor([math.log(8.0), 0.0, math.nan], dtype=F64), torch.tensor([8, 1, 0])
    X.assert_lse("ok", torch.tensor([math.log(8.0) + 7 * 2.0 ** -22, 7 * 2.0 ** -23, 123.0]), w, cnt)
    for wrong in ([math.log(9.0), 0.0, 0.0], [math.log(8.0), 9 * 2.0 ** -23, 0.0], [math.nan, 0.0, 0.0]):
        with pytest.raises(AssertionError, match="ulps"):
            X.assert_lse("bad", torch.tensor(wrong), w, cnt)
    view = X.embed_rows(torch.ones(5, 24, dtype=F64), torch.bfloat16, "cpu")
    assert view.shape == (5, 24) and view.is_contiguous() and float(view.sum()) == 120.0
    parent = torch.as_strided(view, (5 + 2 * X.PAD_ROWS, 24), (24, 1), view.storage_offset() - X.PAD_ROWS * 24)
    assert bool(parent[:X.PAD_ROWS].isnan().all()) and bool(parent[-X.PAD_ROWS:].isnan().all())
    # the guards refuse a badly chosen case: a count of three, a score that does not underflow, a value off bf16
    q, k = torch.zeros(1, 4, dtype=F64), torch.zeros(3, 4, dtype=F64)
    v, do, vis = torch.tensor([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]], dtype=F64), torch.ones(1, 4, dtype=F64), torch.ones(1, 3, dtype=torch.bool)
    with pytest.raises(AssertionError, match="powers of two"):
        X.head_reference(q, k, v, do, vis)
    q2, k2 = torch.tensor([[-8.0, 0, 0, 0]], dtype=F64), torch.tensor([[0.0, 0, 0, 0], [8.0, 0, 0, 0]], dtype=F64)
    with pytest.raises(AssertionError, match="neither scores 0"):
        X.head_reference(q2, k2, v[:2], do, vis[:, :2])
    with pytest.raises(AssertionError, match="not representable in bf16"):
        X.head_reference(q[:, :4], k[:2], v[:2] * 257.0, do, vis[:, :2])
