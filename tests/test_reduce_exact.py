"""CPU: the builders and references of the exact-arithmetic reduction tests (tests/reduce_exact.py, run on the MI355X by
tests/test_reduce_exact_gpu.py), judged alone.  Every builder's 2^24 guard holds (the builders assert it themselves: building a case is the
check), every float64 reference converts to fp32 without loss, the run-length tables of the token ids contain each relation between a run and the
64-entry chunk, every keep of the image embedding leaves a (chunk, position) unkept, and the LayerNorm formula evaluated in fp32 in two different
summation orders equals its float64 value bit for bit where the GPU test asks for bit equality."""
import pytest
import torch

from tests import reduce_exact as R


def _is_int(t, r):
    assert torch.equal(t.double(), t.double().round()) and float(t.abs().max()) <= r


# ---- 1. token embedding ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.TOKEN_DENSE_CASES + R.TOKEN_PACKED_CASES, ids=lambda c: f"B{c[0]}-L{c[1]}-C{c[2]}-{str(c[3]).split('.')[-1]}")
def test_token_cases_hit_every_chunk_relation_and_are_exact(case):
    packed = case in R.TOKEN_PACKED_CASES
    o = R.token_case(*case, packed=packed)
    rel = R.chunk_relations(o["runs"])
    n = o["n"]
    assert rel.pop("partial_last_chunk") == (n % R.CH != 0)
    assert all(rel.values()), [k for k, v in rel.items() if not v]
    # the relations are read from the sorted list itself, not from the table that built it
    keys = o["tokens"].reshape(-1).sort().values
    assert keys.tolist() == [tok for tok, c in o["runs"] for _ in range(c)]
    cl = keys.clamp(0, o["V"] - 1)
    starts = [0] + (cl.diff().nonzero().reshape(-1) + 1).tolist()
    ends = [s - 1 for s in starts[1:]] + [n - 1]
    assert [(int(cl[a]), a, b) for a, b in zip(starts, ends)] == R.clamped_runs(o["runs"])
    assert {-5, -1, 0} <= set(keys.tolist()) and {o["V"] - 1, o["V"], o["V"] + 7} <= set(keys.tolist())
    _is_int(o["dx"], R.DX_R), _is_int(o["dpos0"], R.ACC_R)
    assert torch.equal(o["dx"].double().to(o["dx"].dtype), o["dx"])
    R.f32_exact(o["ref_table"]), R.f32_exact(o["ref_pos"])
    assert int((o["ref_table"].abs().sum(1) > 0).sum()) <= int((~o["never"]).sum())
    if packed:
        B, L = o["B"], o["L"]
        assert torch.equal(o["plan_text"].argmax(1) + 1, o["lens"]) and int(o["seq_off"][-1]) == n
        has = torch.zeros(B, L, dtype=torch.bool)
        has[torch.arange(B)[:, None].expand(B, L)[torch.arange(L)[None, :] < o["lens"][:, None]], o["posidx"].long()] = True
        first, later = has[:128].any(0), has[128:].any(0)
        assert int((~first).sum()) > L // 2 and bool(later.all())  # most positions: nothing in the first chunk of 128, something later


def test_dense_token_cases_cover_the_partial_last_chunk_and_the_batch_chunk():
    assert sum((B * L) % R.CH != 0 for B, L, _, _ in R.TOKEN_DENSE_CASES) >= 3
    assert {B for B, _, _, _ in R.TOKEN_DENSE_CASES} == {5, 128, 129, 300}
    assert {C for _, _, C, _ in R.TOKEN_DENSE_CASES} == {64, 192, 512, 768, 1280}
    assert {d for _, _, _, d in R.TOKEN_DENSE_CASES} == {torch.float32, torch.bfloat16}
    assert all(B * L <= 25000 for B, L, _, _ in R.TOKEN_DENSE_CASES + R.TOKEN_PACKED_CASES) and R.TOKEN_V <= 2000


# ---- 2. image embedding ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,G,C", R.ASSEMBLE_FULL_CASES)
def test_assemble_references_without_keep(B, G, C):
    o = R.assemble_case(B, G, C)
    _is_int(o["demb"], R.DX_R)
    R.f32_exact(o["ref_pos"]), R.f32_exact(o["ref_cls"])
    d3 = o["demb"].reshape(B, G + 1, C)
    assert torch.equal(R.f32_exact(o["ref_pos"]), o["dpos0"] + d3.sum(0)) and torch.equal(R.f32_exact(o["ref_cls"]), o["dcls0"] + d3[:, 0].sum(0))


@pytest.mark.parametrize("B,G,K,C,step", R.ASSEMBLE_KEEP_CASES)
def test_assemble_hand_built_keep_leaves_a_chunk_position_unkept(B, G, K, C, step):
    keep = R.hand_keep(B, G, K, step)
    hole, all_kept = R.keep_coverage(keep, G)
    assert hole and R.keep_is_good(keep, G) and all_kept == (B > R.ASSEMBLE_BCHUNK)
    assert bool((keep.diff(dim=1) < 0).any())  # not ascending everywhere: "any order"
    o = R.assemble_case(B, G, C, keep)
    R.f32_exact(o["ref_pos"]), R.f32_exact(o["ref_cls"])
    # a position nobody kept keeps its initial contents
    kept = torch.zeros(G, dtype=torch.bool)
    kept[keep.long().reshape(-1)] = True
    assert torch.equal(R.f32_exact(o["ref_pos"])[1:][~kept], o["dpos0"][1:][~kept])
    with pytest.raises(AssertionError):
        R.assemble_case(B, G, C, torch.arange(G, dtype=torch.int32).expand(B, G).contiguous())  # everything kept: no hole


# ---- 3. column sums -------------------------------------------------------------------------------------------------------------
def test_colsum_cases():
    assert {1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1031} == set(R.COLSUM_R) and {1, 63, 64, 65, 200, 3} == set(R.COLSUM_C)
    for Rr in R.COLSUM_R:
        for C in R.COLSUM_C:
            o = R.colsum_case(Rr, C)
            _is_int(o["x"], R.COLSUM_X_R)
            assert torch.equal(R.f32_exact(o["ref"]), o["out0"] + o["x"].sum(0)) and torch.equal(R.f32_exact(o["ref"]), o["out0"] + o["x"].flip(0).sum(0))
    o = R.colsum_single_add_case()
    one = torch.ones(())
    assert torch.equal(R.f32_exact(o["ref"]), o["out0"] + 2.0) and torch.equal((o["out0"] + one) + one, o["out0"])  # one addition vs two


# ---- 4. LayerNorm ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", R.LN_POW2_C + R.LN_OTHER_C)
def test_layernorm_formula_is_exact_in_fp32_in_two_orders(C):
    for M in R.LN_M:
        o = R.ln_case(M, C)
        assert set(o["rstd"].tolist()) <= {0.5, 1.0, 2.0} and set(o["w"].tolist()) <= {-2.0, -1.0, 1.0, 2.0}
        _is_int(o["mean"], 2), _is_int(o["dy"], 3), _is_int(o["x"] - o["mean"][:, None], R.ln_ranges(C)[0]), _is_int(o["dres"], R.ln_ranges(C)[1])
        for with_dres in (False, True):
            for order in (0, 1):
                dx, dw, db, dcol = R.ln_formula_f32(o, with_dres, order)
                assert torch.equal(dw, R.f32_exact(o["ref_dw"])) and torch.equal(db, R.f32_exact(o["ref_db"])), (M, C, order)
                if o["pow2"]:
                    assert torch.equal(dx, R.f32_exact(o["ref_dx"][with_dres])), (M, C, with_dres, order)
                    assert torch.equal(dcol, R.f32_exact(o["ref_dcol"][with_dres])), (M, C, with_dres, order)
                    assert torch.equal(R.rne_bf16(dx), dx.to(torch.bfloat16))


def test_layernorm_large_m_case_is_inside_the_guard():
    """the large M of the GPU test depends on the device's CU count: the guard is checked here at the 256 CUs of an MI355X and at twice that"""
    for cus in (256, 512):
        M = R.ln_big_m(cus)
        assert M > 2 * cus * R.LN_WAVES_MAX
        for C in (256, 768, 1280):
            o = R.ln_case(M, C, dcol=False)
            R.f32_exact(o["ref_dw"]), R.f32_exact(o["ref_db"])
            if o["pow2"]:
                R.f32_exact(o["ref_dx"][True])
    with pytest.raises(AssertionError, match="dcol"):
        R.ln_case(R.ln_big_m(256), 2048)  # the column sums of dx over that many rows leave the guard: the builder says so


# ---- 5. gradient norm -----------------------------------------------------------------------------------------------------------
def test_sumsq_and_clip_references():
    for n in R.SUMSQ_N:
        o = R.sumsq_case(n)
        _is_int(o["x"], R.SUMSQ_R)
        assert float(R.f32_exact(o["ref"])) == o["out0"] + float((o["x"] ** 2).sum())
    o = R.clip_case()
    assert [tuple(t.shape) for t in o["grads"]] == list(R.CLIP_SHAPES)
    for t in o["grads"]:
        _is_int(t, R.CLIP_R)
    assert float(R.f32_exact(o["ref"])) == sum(float((t ** 2).sum()) for t in o["grads"])


# ---- 6. loss rows ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R_,N,off", R.LOSS_SHAPES)
def test_loss_row_bounds_against_the_plain_fp32_statement(R_, N, off):
    """the fp32 torch statement of each row stays inside the issue's bounds against float64 on the same logits -- except d/d logit_scale of a peaked
    cross-entropy row, where fp32 cannot hold softmax(label) - 1 (1 / (1 + 1e-13) is 1): its error is the whole row, R.CE_PEAKED_DSCALE_FP32 of the
    row's sum of |term| at the most, and the GPU test's bound for that quantity is four times that figure"""
    worst = 0.0
    for peaked in (False, True):
        lg = R.loss_logits(R_, N, off, peaked)
        if peaked:
            rows = torch.arange(R_)
            others = lg.clone()
            others[rows, rows + off] = -float("inf")
            assert torch.equal(lg[rows, rows + off], others.max(1).values + 30.0)
        for kind in ("ce", "siglip", "siglip_neg"):
            r64, bounds, _ = R.loss_rows_reference(lg, off, kind)
            r32, _, _ = R.loss_rows_reference(lg, off, kind, torch.float32)
            ratio = R.worst_ratio(r32, r64, bounds)
            if kind == "ce" and peaked:
                worst = max(worst, ratio[1] * R.DSUM_REL)
                ratio[1] = 0.0
            assert max(ratio) < 0.5, (kind, peaked, ratio)
    assert 0.5 < worst <= R.CE_PEAKED_DSCALE_FP32, worst
