"""The cases behind tests/golden/variants_parent.npz: LayerNorm forward and backward and the deterministic wgrad, as the commit computed them that
still had the wgrad's 32x32x16 main loop and LayerNorm's cache-policy variants beside the kernels the product runs.  Inputs are Gaussian, drawn
from a seeded CPU generator (the backward's ``mean`` / ``rstd`` too: no kernel's output is another case's input), and go through ``ops`` only.

LayerNorm, C x M of ``LN_C`` x ``LN_M``: C = 128 and 1536 take the guarded one-row kernels (C is no multiple of 256), C = 256, 768 and 1280 the
pipelined kernels on a bf16 stream (1280 is their register limit), C = 2048 is the full NV = 8.  The backward runs on ``BWD_GRID`` workgroups
(tuning key 14): M = 149 = 3 * 3 * 16 + 5 then gives every wave of the widest workgroup at least three rows and a ragged last round on a device of
any size.  ``dx32`` / ``dx16`` come from the default launch (no addition in them depends on an order), ``dw`` / ``db`` / ``dcol`` from the
deterministic one.  The wgrad's deterministic form cuts M by the device's CU count, which is why the fixture records that count.

The fixture holds one SHA-256 per array (``tests.optim_util.digest``)."""
import os

import numpy as np
import torch

from tests.optim_util import digest  # noqa: F401  (re-exported: the fixture's one digest)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "variants_parent.npz")
CU_KEY = "cu_count"

LN_C = (128, 256, 768, 1280, 1536, 2048)
LN_M = (1, 149)
BWD_GRID = 3
WGRAD_SHAPE = (8203, 512, 512)
F32, BF16 = torch.float32, torch.bfloat16


def cu_count(dev):
    return int(torch.cuda.get_device_properties(dev).multi_processor_count)


def _np(t):
    return (t.view(torch.int16) if t.dtype == BF16 else t).cpu().numpy().copy()


def _draw(gen, shape, dtype, dev, scale=1.0):
    return (torch.randn(shape, generator=gen) * scale).to(dtype).to(dev)


def fwd_cases():
    """(name, C, M, x dtype, want y16, want y32)"""
    return [(f"fwd/C{C}/M{M}/x{'16' if xd == BF16 else '32'}/{out}", C, M, xd, out != "y32", out != "y16")
            for C in LN_C for M in LN_M for xd in (F32, BF16) for out in ("y16", "y32", "both")]


def bwd_cases():
    """(name, C, M, x dtype, dy dtype, dres dtype | None, dcol, dx32)"""
    cases = []
    for C in LN_C:
        for M in LN_M:
            for dyd in (F32, BF16):
                for dres in (None, F32):
                    for dcol in (True, False):
                        cases.append((f"bwd/C{C}/M{M}/x32/dy{'32' if dyd == F32 else '16'}/dres{'32' if dres else '0'}/dcol{int(dcol)}",
                                      C, M, F32, dyd, dres, dcol, True))
            for dres in (None, BF16, F32):
                for dx32 in (True, False):
                    tag = {None: "0", BF16: "16", F32: "32"}[dres]
                    cases.append((f"bwd/C{C}/M{M}/x16/dres{tag}/dx32{int(dx32)}", C, M, BF16, BF16, dres, False, dx32))
    return cases


def run_fwd(dev):
    from open_clip_amd import ops
    out = {}
    for name, C, M, xd, y16, y32 in fwd_cases():
        gen = torch.Generator().manual_seed(1000 + C + M)
        x, w, b = _draw(gen, (M, C), xd, dev, 1.5), _draw(gen, (C,), F32, dev), _draw(gen, (C,), F32, dev)
        got = ops.layernorm_fwd(x, w, b, want_bf16=y16, want_f32=y32)
        for key, t in zip(("y16", "y32", "mean", "rstd"), got):
            if t is not None:
                out[f"{name}/{key}"] = _np(t)
    return out


def run_bwd(dev):
    from open_clip_amd import _lib, ops
    out = {}
    try:
        _lib.call("ocn_set_tuning", 14, BWD_GRID)
        for name, C, M, xd, dyd, dres_d, dcol, dx32 in bwd_cases():
            gen = torch.Generator().manual_seed(2000 + C + M)
            x, dy, w = _draw(gen, (M, C), xd, dev, 1.5), _draw(gen, (M, C), dyd, dev), _draw(gen, (C,), F32, dev)
            mean, rstd = _draw(gen, (M,), F32, dev, 0.1), (0.5 + torch.rand(M, generator=gen)).to(dev)
            dres = None if dres_d is None else _draw(gen, (M, C), dres_d, dev)
            acc0 = [_draw(gen, (C,), F32, dev) for _ in range(3)]  # dw, db, dcol are accumulated into
            for det in (False, True):
                dw, db, dc = (t.clone() for t in acc0)
                o32, o16 = ops.layernorm_bwd(dy, x, w, mean, rstd, dw, db, dres=dres, want_f32=dx32, want_bf16=True, dcol=dc if dcol else None,
                                             deterministic=det)
                if not det:
                    out[f"{name}/dx16"] = _np(o16)
                    if dx32:
                        out[f"{name}/dx32"] = _np(o32)
                else:
                    out[f"{name}/dw"], out[f"{name}/db"] = _np(dw), _np(db)
                    if dcol:
                        out[f"{name}/dcol"] = _np(dc)
    finally:
        _lib.call("ocn_set_tuning", 14, 0)
    return out


def run_wgrad(dev):
    from open_clip_amd import ops
    M, N, K = WGRAD_SHAPE
    gen = torch.Generator().manual_seed(3000)
    a, b = _draw(gen, (M, N), BF16, dev), _draw(gen, (M, K), BF16, dev)
    dw, db = _draw(gen, (N, K), F32, dev), _draw(gen, (N,), F32, dev)
    ops.gemm_tn_accum(a, b, dw, db, deterministic=True)
    return {"wgrad/dW": _np(dw), "wgrad/dbias": _np(db)}


def run_all(dev):
    """{"<case>/<array>": array} over every case"""
    out = {**run_fwd(dev), **run_bwd(dev), **run_wgrad(dev)}
    torch.cuda.synchronize()
    return out
