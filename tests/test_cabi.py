"""CPU: the C-ABI library builds/loads and exports exactly what include/openclip_hip.h declares."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "openclip_hip.h")


DEBUG_HEADER = os.path.join(ROOT, "include", "openclip_hip_debug.h")


def _declared(header=HEADER):
    src = open(header).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ocn_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib_path():
    from open_clip_amd import build
    return build.build()


def test_header_declares_the_python_table(lib_path):
    from open_clip_amd import _lib
    declared = _declared()
    table = sorted(list(_lib.SIGNATURES) + list(_lib._SPECIAL))
    assert declared == table, (set(declared) ^ set(table))
    # the developer knobs live in their own header and table: none of them is part of the boundary
    assert _declared(DEBUG_HEADER) == sorted(_lib.DEBUG_SIGNATURES), set(_declared(DEBUG_HEADER)) ^ set(_lib.DEBUG_SIGNATURES)
    assert not set(declared) & set(_lib.DEBUG_SIGNATURES)


def test_library_exports_every_declared_symbol(lib_path):
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (ocn_[a-z0-9_]+)", out))
    missing = (set(_declared()) | set(_declared(DEBUG_HEADER))) - exported
    assert not missing, missing


def test_library_loads_and_reports_errors(lib_path):
    from open_clip_amd import _lib
    lib = _lib.load()
    hdr = int(re.search(r"#define OCN_ABI_VERSION (\d+)", open(HEADER).read()).group(1))
    assert lib.ocn_version() == hdr == _lib.ABI_VERSION  # header == library == ctypes table: load() refuses any other library
    # argument validation happens on the host before any launch: safe without a GPU
    with pytest.raises(RuntimeError, match="K=48 must be a multiple of 32"):
        _lib.call("ocn_gemm_nt", 0, 16, 48, 16, 48, 16, 64, 8, 64, 48, 0, 0, 0, 1.0, 0)
    with pytest.raises(RuntimeError, match="null operand"):
        _lib.call("ocn_layernorm_fwd", 0, 0, 0, 0, 0, 0, 0, 0, 4, 64, 1e-5, 0)


def test_attention_and_token_embed_layout_rules(lib_path):
    """the dense / packed layout rules of ocn_attn_fwd / ocn_attn_bwd / ocn_token_embed_fwd / ocn_token_embed_bwd are checked on the host before any
    launch, each refusal naming its rule.  Device operands are fake (never dereferenced); bucket_counts is a host array the library reads."""
    import ctypes
    from open_clip_amd import _lib
    p, B, H = 4096, 4, 2  # a fake 16-byte aligned device pointer
    counts = lambda L: (ctypes.c_int32 * ((L + 31) // 32))(B)

    def attn(fn, seq_off, order, bucket_counts, L, head_dim, delta_ws=p):
        operands = (p, p, p) if fn == "ocn_attn_fwd" else (p, p, p, p, p, delta_ws)  # qkv, out, lse | qkv, out, dout, lse, dqkv, delta_ws
        _lib.call(fn, *operands, seq_off, order, bucket_counts, B, L, H, head_dim, 1, 0.125, 0)

    for fn in ("ocn_attn_fwd", "ocn_attn_bwd"):
        with pytest.raises(RuntimeError, match=fn + r" failed \(-1\): " + fn + ": order and bucket_counts go together"):
            attn(fn, p, p, None, 77, 64)
        with pytest.raises(RuntimeError, match=fn + r" failed \(-1\): " + fn + ": order and bucket_counts go together"):
            attn(fn, p, None, counts(77), 77, 64)
        with pytest.raises(RuntimeError, match=fn + r" failed \(-1\): " + fn + ": order / bucket_counts bucket a packed batch, but seq_off is NULL"):
            attn(fn, None, p, counts(77), 77, 64)
        with pytest.raises(RuntimeError, match=fn + r" failed \(-3\): " + fn + r": a packed batch .* needs head_dim == 64 and L <= 320 \(head_dim=80, L=77\)"):
            attn(fn, p, None, None, 77, 80)
        with pytest.raises(RuntimeError, match=fn + r" failed \(-3\): " + fn + r": a packed batch .* needs head_dim == 64 and L <= 320 \(head_dim=64, L=321\)"):
            attn(fn, p, p, counts(321), 321, 64)
    with pytest.raises(RuntimeError, match=r"ocn_attn_bwd failed \(-1\): ocn_attn_bwd: the streamed backward \(head_dim=80, L=77\) needs delta_ws"):
        attn("ocn_attn_bwd", None, None, None, 77, 80, delta_ws=None)
    with pytest.raises(RuntimeError, match=r"ocn_token_embed_fwd: M=100 is not a multiple of L=77 \(dense"):
        _lib.call("ocn_token_embed_fwd", p, None, p, p, p, 100, 77, 64, 1000, 0)
    with pytest.raises(RuntimeError, match=r"ocn_token_embed_bwd: M=100 rows, but a dense batch \(seq_off == NULL\) has B\*L = 4\*77"):
        _lib.call("ocn_token_embed_bwd", p, p, p, 0, p, p, None, B, 77, 100, 64, 1000, 0, 0)


def test_removed_wgrad_variants_are_refused(lib_path):
    """ocn_set_gemm_variant's TN values 6 / 7 chose between two main loops of the hand-scheduled wgrad kernel; one loop is left, and a tool that
    still asks for either must fail (host-side check, no launch) instead of timing one kernel twice.  The values that remain are accepted."""
    from open_clip_amd import _lib
    try:
        for tn in (6, 7):
            with pytest.raises(RuntimeError, match=rf"ocn_set_gemm_variant failed \(-1\): ocn_set_gemm_variant: TN value {tn} is gone"):
                _lib.call("ocn_set_gemm_variant", (tn << 4) | 5)
        for tn in (0, 1, 3):
            for nt in (0, 4, 5, 6, 7):
                _lib.call("ocn_set_gemm_variant", (tn << 4) | nt)
    finally:
        _lib.call("ocn_set_gemm_variant", 0)


def test_library_contains_gfx950_code_object(lib_path):
    data = open(lib_path, "rb").read()
    assert b"gfx950" in data
