"""The attention kernels (csrc/attention.hip, attention_generic.hip, attention_pooled.hip) through ``open_clip_amd.ops`` on the exact-arithmetic inputs
of tests/attn_exact.py: softmax exactly one-hot or exactly uniform over 2^k keys, small integers everywhere else.  Nothing here is a measured tolerance:
``out`` and ``dV`` are bit-equal to the float64 reference (bf16 against bf16), ``dQ`` / ``dK`` within g / 8 of it (g: the case's grid step; the fp32 noise
that survives where the true dS is 0 is bounded below g / 16, a wrong, missing or extra key moves a value by >= g), ``lse`` within 8 fp32 ulps of ln(count).
Every input is a row slice of an allocation whose rows in front of and behind it are NaN; the guards of the reference run again before each comparison.
The measured dQ / dK maxima go to the parity report."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from open_clip_amd import _lib, ops  # noqa: E402
from tests import attn_exact as X  # noqa: E402

DEV = "cuda:0"
BF16 = torch.bfloat16


def _run_self(inp, layout=None):
    """forward and backward of one self-attention case -> the kernels' outputs (the backward takes the forward's own out and lse, as the model does)"""
    c = inp["case"]
    qkv, dout = X.embed_rows(inp["qkv"], BF16, DEV), X.embed_rows(inp["dout"], BF16, DEV)
    args = (c["B"], c["L"], c["H"], c["causal"], X.SCALE, c["D"])
    try:
        for knob, value in c["knobs"]:
            _lib.call("ocn_set_tuning", knob, value)
        out, lse = ops.attn_fwd(qkv, *args, seq_off=layout)
        dqkv = ops.attn_bwd(qkv, out, dout, lse, *args, seq_off=layout)
    finally:
        for knob, _ in c["knobs"]:
            _lib.call("ocn_set_tuning", knob, 0)
    torch.cuda.synchronize()
    return {"out": out, "lse": lse, "dqkv": dqkv}


def _line(c, name, ref, dq, dk):
    counts = sorted(set(ref["count"].reshape(-1).tolist()) - {0})
    X.report(f"attn exact {name:62s} out / dV bit-equal, lse within 8 ulps, counts {counts}; max|dQ - ref| {dq:.3e} max|dK - ref| {dk:.3e} "
             f"(g / 8 = {X.G_DQ / 8:.3e}, noise bound {ref['noise']:.2e}){' -- ' + c['branch'] if c.get('branch') else ''}")


@pytest.mark.parametrize("c", X.SELF_CASES, ids=X.case_id)
def test_attention_exact(c):
    inp = X.build_self(c)
    ref = X.reference_self(inp)  # (guards)
    name = X.case_id(c)
    dq, dk = X.check_self(name, _run_self(inp), ref, inp)
    _line(c, name, ref, dq, dk)


@pytest.mark.parametrize("c", X.PACKED_CASES, ids=X.case_id)
def test_attention_exact_packed_and_its_dense_twin(c):
    """ops.SeqLayout, causal: lengths {77, 1, 32, 33, 64, 9} in an order that interleaves the buckets; behind every sequence the next one's decoy keys.
    The dense batch that holds the same rows must give identical bits on them."""
    inp = X.build_self(c)
    ref = X.reference_self(inp)
    seq_off = torch.tensor(inp["off"], dtype=torch.int32, device=DEV)
    order, counts = X.bucket_layout(inp["lens"], c["L"])
    layout = ops.SeqLayout(seq_off, order.to(DEV), counts) if c["bucketed"] else ops.SeqLayout(seq_off)
    name = X.case_id(c)
    got = _run_self(inp, layout)
    dq, dk = X.check_self(name, got, ref, inp)
    _line(c, name, ref, dq, dk)
    twin = X.dense_twin(inp)
    tref = X.reference_self(twin)
    tgot = _run_self(twin)
    X.check_self(name + " dense twin", tgot, tref, twin)
    L = c["L"]
    lse_p, lse_d = got["lse"].reshape(c["B"], c["H"], L), tgot["lse"].reshape(c["B"], c["H"], L)
    for b, n in enumerate(inp["lens"]):
        r0 = inp["off"][b]
        for key in ("out", "dqkv"):
            assert torch.equal(got[key][r0:r0 + n], tgot[key][b * L:b * L + n]), f"{name}: {key} of sequence {b} differs between the packed and the dense batch"
        assert torch.equal(lse_p[b, :, :n], lse_d[b, :, :n]), f"{name}: lse of sequence {b} differs between the packed and the dense batch"


@pytest.mark.parametrize("c", X.POOLED_CASES, ids=X.case_id)
def test_attention_pooled_exact(c):
    """ops.attn_pooled_fwd / attn_pooled_bwd: image CLS at 50 and 257 tokens, packed text (ragged, a length of 1), dense causal text with the query in
    mid-sequence -- the rows behind it are decoys (the code of a selected key) and their dK / dV rows must come back as exact zeros"""
    inp = X.build_pooled(c)
    ref = X.reference_pooled(inp)
    q, kv, dout = (X.embed_rows(inp[k], BF16, DEV) for k in ("q", "kv", "dout"))
    rows = inp["rows"].to(DEV)
    seq_off = torch.tensor(inp["off"], dtype=torch.int32, device=DEV) if c["lens"] else None
    args = (rows, c["B"], c["L"], c["H"], c["causal"], X.SCALE, seq_off)
    out, lse = ops.attn_pooled_fwd(q, kv, *args)
    dq, dkv = ops.attn_pooled_bwd(q, kv, out, dout, lse, *args)
    torch.cuda.synchronize()
    name = X.case_id(c)
    mq, mk = X.check_pooled(name, {"out": out, "lse": lse, "dq": dq, "dkv": dkv}, ref, inp)
    _line(c, name, ref, mq, mk)
