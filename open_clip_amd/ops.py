"""Tensor-level wrappers over the C ABI (include/openclip_hip.h).

PyTorch is plumbing here: it owns device memory (caching allocator) and the stream.  Every wrapper checks
device / dtype / contiguity, then enqueues the HIP kernel on ``torch.cuda.current_stream()``.  There is no
CPU or ATen fallback: a CPU tensor or a missing library raises.
"""
import torch

from . import _lib

EPI_BF16, EPI_BIAS_GELU, EPI_BIAS_RESID_F32, EPI_DGELU, EPI_F32 = 0, 1, 2, 3, 4
EPI_BIAS_QUICKGELU = 7  # EPI_BIAS_GELU with x * sigmoid(1.702 x) (layers.py:29-32); its backward is the same EPI_DGELU
EPI_BIAS_RESID_BF16 = 8  # out bf16 = bf16(resid bf16 + bf16(acc + bias)): the residual add on the image tower's bf16 stream (as the reference's autocast)
BF16, F32 = torch.bfloat16, torch.float32


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _chk(t, dtype, name):
    if t is None:
        return 0
    if not t.is_cuda:
        raise RuntimeError(f"open_clip_amd: '{name}' must live on the MI355X (got {t.device}); there is no CPU path")
    if t.dtype != dtype:
        raise RuntimeError(f"open_clip_amd: '{name}' must be {dtype} (got {t.dtype})")
    if not t.is_contiguous():
        raise RuntimeError(f"open_clip_amd: '{name}' must be contiguous")
    return t.data_ptr()


def _chk2d(t, dtype, name):
    """2-D, unit inner stride, arbitrary row stride -> (ptr, ld)"""
    if not t.is_cuda:
        raise RuntimeError(f"open_clip_amd: '{name}' must live on the MI355X (got {t.device}); there is no CPU path")
    if t.dtype != dtype or t.dim() != 2 or t.stride(1) != 1:
        raise RuntimeError(f"open_clip_amd: '{name}' must be a 2-D {dtype} matrix with unit inner stride")
    return t.data_ptr(), t.stride(0)


def empty(shape, dtype, like):
    return torch.empty(shape, dtype=dtype, device=like.device)


# ---- GEMMs ------------------------------------------------------------------------------------------
def gemm_nt(epi, a, b, out, bias=None, resid=None, aux=None, alpha=1.0):
    """out[M,N] = a[M,K] @ b[N,K]^T (+ epilogue); a, b bf16; out bf16 or fp32 depending on ``epi``.  ``aux`` (uint8 [M,N]) holds the
    GELU derivative in 8-bit fixed point (written by EPI_BIAS_GELU, read by EPI_DGELU; see ``dgelu_encode`` / ``dgelu_decode``)."""
    pa, lda = _chk2d(a, BF16, "a")
    pb, ldb = _chk2d(b, BF16, "b")
    odt = F32 if epi in (EPI_BIAS_RESID_F32, EPI_F32) else BF16
    rdt = BF16 if epi == EPI_BIAS_RESID_BF16 else F32
    po, ldc = _chk2d(out, odt, "out")
    M, K = a.shape
    N = b.shape[0]
    if b.shape[1] != K or out.shape[0] != M or out.shape[1] != N:
        raise RuntimeError(f"gemm_nt: shape mismatch a{tuple(a.shape)} b{tuple(b.shape)} out{tuple(out.shape)}")
    if resid is not None and (resid.shape != out.shape or resid.stride(0) != ldc):
        raise RuntimeError("gemm_nt: resid must match out")
    if aux is not None and (aux.shape != out.shape or aux.stride(0) != ldc):
        raise RuntimeError("gemm_nt: aux must match out")
    _lib.call("ocn_gemm_nt", epi, pa, lda, pb, ldb, po, ldc, M, N, K, _chk(bias, F32, "bias"),
              0 if resid is None else _chk2d(resid, rdt, "resid")[0], 0 if aux is None else _chk2d(aux, torch.uint8, "aux")[0],
              float(alpha), _stream())
    return out


def set_tile_rescue(on: bool):
    """``ocn_set_tile_rescue``: the persistent GEMMs' multi-GPU form (finishing workgroups hand out the shares of workgroups whose CU is held by a
    collective's kernel; include/openclip_hip.h).  Process-wide; same results (NT bit-identical, wgrad up to the order of its fp32 atomics)."""
    _lib.call("ocn_set_tile_rescue", int(bool(on)))


def tile_rescue() -> bool:
    return bool(_lib.load().ocn_get_tile_rescue())


def multi_gpu_defaults(world_size: int):
    """What a data-parallel run switches on in the kernels (called by the distributed losses and by ``NativeGradSync`` when world_size > 1, i.e. wherever
    collectives' kernels will hold CUs while GEMMs are launched): the GEMMs' rescue form.  ``set_tile_rescue(False)`` afterwards switches it off again;
    the environment variable OCN_TILE_RESCUE=0 keeps it off."""
    import os
    if int(world_size) > 1 and torch.cuda.is_available() and os.environ.get("OCN_TILE_RESCUE", "1") != "0":
        set_tile_rescue(True)


def gemm_nt_splitk_plan(M, N, K):
    """K-slices ``gemm_nt_splitk`` should use for out[M,N] = a[M,K] @ b[N,K]^T (1: the product fills the chip as it is -- use ``gemm_nt``)"""
    return int(_lib.load().ocn_gemm_nt_splitk_plan(int(M), int(N), int(K)))


def gemm_nt_splitk(a, b, out, ksplit, rowscale=None, sub_rows=None, sub_alpha=0.0, scale=None):
    """out[M,N] fp32 = scale * (rowscale[:, None] * (a[M,K] @ b[N,K]^T) - sub_alpha * sub_rows) with K cut into ``ksplit`` slices that run as tiles of their own
    (few output tiles, long K: ocn_gemm_nt_splitk); ``rowscale`` fp32 [M], ``sub_rows`` bf16 [M,N], ``scale`` a 1-element fp32 device tensor, each optional"""
    pa, lda = _chk2d(a, BF16, "a")
    pb, ldb = _chk2d(b, BF16, "b")
    po, ldc = _chk2d(out, F32, "out")
    M, K = a.shape
    N = b.shape[0]
    if b.shape[1] != K or tuple(out.shape) != (M, N):
        raise RuntimeError(f"gemm_nt_splitk: shape mismatch a{tuple(a.shape)} b{tuple(b.shape)} out{tuple(out.shape)}")
    ws = torch.empty(int(ksplit) * M * ldc, dtype=F32, device=a.device)
    ps, lds = (0, 0) if sub_rows is None else _chk2d(sub_rows, BF16, "sub_rows")
    _lib.call("ocn_gemm_nt_splitk", pa, lda, pb, ldb, po, ldc, M, N, K, int(ksplit), ws.data_ptr(), _chk(rowscale, F32, "rowscale"), ps, lds, float(sub_alpha),
              _chk(scale, F32, "scale"), _stream())
    return out


def scale_rows_bf16(x16, scale):
    """bf16(scale[r] * x16[r, :])"""
    px, ldx = _chk2d(x16, BF16, "x16")
    out = empty(x16.shape, BF16, x16)
    _lib.call("ocn_scale_rows_bf16", px, ldx, _chk(scale, F32, "scale"), out.data_ptr(), out.stride(0), x16.shape[0], x16.shape[1], _stream())
    return out


def sub_scaled_rows(out, x16, scale, alpha):
    """out[r, :] -= (alpha / scale[r]) * x16[r, :]   (out fp32 [R, E], a row-contiguous view is fine)"""
    po, ldo = _chk2d(out, F32, "out")
    px, ldx = _chk2d(x16, BF16, "x16")
    _lib.call("ocn_sub_scaled_rows", po, ldo, px, ldx, _chk(scale, F32, "scale"), float(alpha), x16.shape[0], x16.shape[1], _stream())
    return out


DGELU_SCALE, DGELU_OFFSET = 200.0, 0.13  # csrc/ocn_common.h: q = round((gelu' + 0.13) * 200), |error| <= 0.0025


def dgelu_decode(q):
    """the values the backward epilogue multiplies with, from the stored bytes (test / tooling helper; torch arithmetic)"""
    return q.float() / DGELU_SCALE - DGELU_OFFSET


def dgelu_encode(d):
    """bytes for given derivative values in [-0.13, 1.145] (test / tooling helper)"""
    return torch.round((d.float() + DGELU_OFFSET) * DGELU_SCALE).clamp_(0, 255).to(torch.uint8)


def gemm_tn_accum(a, b, dw, dbias=None, alpha=1.0, deterministic=False):
    """dw[N,K] += alpha * a[M,N]^T @ b[M,K]; dbias[N] += alpha * colsum(a).  a, b bf16; dw, dbias fp32.
    ``deterministic``: the reproducible form (ocn_gemm_tn_accum_det: per-split slabs summed in a fixed order instead of fp32 atomics)"""
    pa, lda = _chk2d(a, BF16, "a")
    pb, ldb = _chk2d(b, BF16, "b")
    pw, ldw = _chk2d(dw, F32, "dw")
    M, N = a.shape
    K = b.shape[1]
    if b.shape[0] != M or dw.shape[0] != N or dw.shape[1] != K:
        raise RuntimeError(f"gemm_tn_accum: shape mismatch a{tuple(a.shape)} b{tuple(b.shape)} dw{tuple(dw.shape)}")
    if deterministic:
        need = _lib.load().ocn_gemm_tn_det_workspace_bytes(M, N, K)
        ws = torch.empty(need, dtype=torch.uint8, device=a.device) if need > 0 else None
        _lib.call("ocn_gemm_tn_accum_det", pa, lda, pb, ldb, pw, ldw, M, N, K, _chk(dbias, F32, "dbias"), float(alpha),
                  0 if ws is None else ws.data_ptr(), need, _stream())
        return dw
    _lib.call("ocn_gemm_tn_accum", pa, lda, pb, ldb, pw, ldw, M, N, K, _chk(dbias, F32, "dbias"), float(alpha), _stream())
    return dw


def gemm_tn_accum2(a1, b1, dw1, dbias1, a2, b2, dw2, dbias2, alpha=1.0):
    """two weight gradients over the same rows and the same K in ONE launch (ocn_gemm_tn_accum2):
    dw1 += alpha * a1^T @ b1, dw2 += alpha * a2^T @ b2 (+ both bias gradients or neither)"""
    M, K = b1.shape
    if a1.shape[0] != M or a2.shape[0] != M or tuple(b2.shape) != (M, K) or tuple(dw1.shape) != (a1.shape[1], K) or tuple(dw2.shape) != (a2.shape[1], K):
        raise RuntimeError(f"gemm_tn_accum2: shape mismatch a1{tuple(a1.shape)} b1{tuple(b1.shape)} dw1{tuple(dw1.shape)} "
                           f"a2{tuple(a2.shape)} b2{tuple(b2.shape)} dw2{tuple(dw2.shape)}")
    if (dbias1 is None) != (dbias2 is None):
        raise RuntimeError("gemm_tn_accum2: both bias gradients or neither")
    pa1, lda1 = _chk2d(a1, BF16, "a1")
    pb1, ldb1 = _chk2d(b1, BF16, "b1")
    pw1, ldw1 = _chk2d(dw1, F32, "dw1")
    pa2, lda2 = _chk2d(a2, BF16, "a2")
    pb2, ldb2 = _chk2d(b2, BF16, "b2")
    pw2, ldw2 = _chk2d(dw2, F32, "dw2")
    _lib.call("ocn_gemm_tn_accum2", pa1, lda1, pb1, ldb1, pw1, ldw1, _chk(dbias1, F32, "dbias1"), a1.shape[1],
              pa2, lda2, pb2, ldb2, pw2, ldw2, _chk(dbias2, F32, "dbias2"), a2.shape[1], M, K, float(alpha), _stream())
    return dw1, dw2


# ---- casts --------------------------------------------------------------------------------------------
def cast_bf16(src, out=None):
    out = empty(src.shape, BF16, src) if out is None else out
    _lib.call("ocn_cast_f32_bf16", _chk(src, F32, "src"), _chk(out, BF16, "out"), src.numel(), _stream())
    return out


def cast_bf16_scaled(src, scale, out=None):
    """bf16(src * scale) with ``scale`` a 1-element fp32 DEVICE tensor (no host read of its value)"""
    out = empty(src.shape, BF16, src) if out is None else out
    _lib.call("ocn_cast_f32_bf16_scaled", _chk(src, F32, "src"), _chk(out, BF16, "out"), src.numel(), _chk(scale, F32, "scale"), _stream())
    return out


def cast_f32(src, out=None):
    """fp32 copy of a bf16 tensor (exact; ocn_cast_bf16_f32)"""
    out = empty(src.shape, F32, src) if out is None else out
    _lib.call("ocn_cast_bf16_f32", _chk(src, BF16, "src"), _chk(out, F32, "out"), src.numel(), _stream())
    return out


def cast_transpose_bf16(src, out=None):
    R, C = src.shape
    out = empty((C, R), BF16, src) if out is None else out
    _lib.call("ocn_cast_transpose_f32_bf16", _chk(src, F32, "src"), _chk(out, BF16, "out"), R, C, _stream())
    return out


# ---- LayerNorm -----------------------------------------------------------------------------------------
def layernorm_fwd(x, w, b, want_bf16=True, want_f32=False, eps=1e-5):
    """``x`` fp32 or bf16 (the image tower's bf16 residual stream); statistics and arithmetic are fp32 either way"""
    M, C = x.shape
    y16 = empty((M, C), BF16, x) if want_bf16 else None
    y32 = empty((M, C), F32, x) if want_f32 else None
    mean, rstd = empty((M,), F32, x), empty((M,), F32, x)
    x16 = x.dtype == BF16
    _lib.call("ocn_layernorm_fwd", _chk(x, BF16 if x16 else F32, "x"), int(x16), _chk(w, F32, "w"), _chk(b, F32, "b"), _chk(y16, BF16, "y16"),
              _chk(y32, F32, "y32"), _chk(mean, F32, "mean"), _chk(rstd, F32, "rstd"), M, C, float(eps), _stream())
    return y16, y32, mean, rstd


def layernorm_bwd(dy, x, w, mean, rstd, dw, db, dres=None, want_f32=True, want_bf16=False, dcol=None, deterministic=False):
    """(dx fp32 | None, dx bf16 | None); ``dres`` = the residual branch's fp32 gradient, added in; dw / db are accumulated into;
    ``dcol`` (fp32 [C], accumulated into): column sums of dx in fp32 = the bias gradient of the linear in front of this LayerNorm's input;
    ``deterministic``: dw / db / dcol through per-workgroup slabs added in a fixed order instead of fp32 atomics.
    ``x`` fp32 or bf16; with a bf16 ``x`` (image tower, bf16 residual stream) ``dy`` is bf16 and ``dres`` bf16 or fp32"""
    M, C = x.shape
    is32 = dy.dtype == F32
    x16 = x.dtype == BF16
    dr16 = dres is not None and dres.dtype == BF16
    dx32 = empty((M, C), F32, x) if want_f32 else None
    dx16 = empty((M, C), BF16, x) if want_bf16 else None
    ws = empty((_lib.load().ocn_layernorm_bwd_det_workspace_floats(M, C),), F32, x) if deterministic else None
    _lib.call("ocn_layernorm_bwd", _chk(dy, F32 if is32 else BF16, "dy"), int(is32), _chk(x, BF16 if x16 else F32, "x"), int(x16), _chk(w, F32, "w"),
              _chk(mean, F32, "mean"), _chk(rstd, F32, "rstd"), _chk(dres, BF16 if dr16 else F32, "dres"), int(dr16), _chk(dx32, F32, "dx32"), _chk(dx16, BF16, "dx16"),
              _chk(dw, F32, "dw"), _chk(db, F32, "db"), _chk(dcol, F32, "dcol"), _chk(ws, F32, "det_workspace"), M, C, _stream())
    return dx32, dx16


def colsum_f32(x, out, deterministic=False):
    """out[C] += column sums of x [R, C] (fp32); ``deterministic``: a single, fixed order of additions"""
    R, C = x.shape
    _lib.call("ocn_colsum_f32", _chk(x, F32, "x"), _chk(out, F32, "out"), R, C, int(deterministic), _stream())
    return out


# ---- attention -------------------------------------------------------------------------------------------
class SeqLayout:
    """layout of a packed ("varlen") batch as the attention launches take it: ``seq_off`` (int32 [B+1], device) and, optionally, the
    buckets of ocn_seq_bucket_plan -- ``order`` (int32 [B], device) + ``counts`` (host ints, one per 32-row block count)"""
    __slots__ = ("seq_off", "order", "counts", "_c")

    def __init__(self, seq_off, order=None, counts=None):
        import ctypes
        self.seq_off, self.order, self.counts = seq_off, order, (list(counts) if counts is not None else None)
        self._c = (ctypes.c_int32 * len(self.counts))(*self.counts) if self.counts is not None else None

    def args(self, B, L):
        so = _chk(self.seq_off, torch.int32, "seq_off")
        if self.order is None:
            return so, 0, 0
        if self.order.numel() != B or len(self.counts) != (L + 31) // 32 or sum(self.counts) != B:
            raise RuntimeError(f"SeqLayout: order of {self.order.numel()} ids / counts {self.counts} do not describe B={B}, L={L}")
        return so, _chk(self.order, torch.int32, "order"), self._c


def _layout(seq_off):
    return seq_off if isinstance(seq_off, SeqLayout) else SeqLayout(seq_off)


def attn_fwd(qkv, B, L, H, causal, scale, head_dim=64, seq_off=None):
    """``seq_off`` (int32 [B+1] on the device, or a SeqLayout): packed batch -- sequence b owns rows seq_off[b]..seq_off[b+1] of qkv
    (head_dim 64 only)"""
    C = H * head_dim
    so, order, counts = (0, 0, 0)
    if seq_off is not None:
        lay = _layout(seq_off)
        if head_dim != 64 or qkv.shape[1] != 3 * C or lay.seq_off.numel() != B + 1:
            raise RuntimeError(f"attn_fwd(varlen): needs head_dim 64 and seq_off of B+1 entries (qkv {tuple(qkv.shape)}, head_dim {head_dim})")
        so, order, counts = lay.args(B, L)
    elif qkv.shape != (B * L, 3 * C):
        raise RuntimeError(f"attn_fwd: qkv shape {tuple(qkv.shape)} != {(B * L, 3 * C)} (H={H}, head_dim={head_dim})")
    out = empty((qkv.shape[0], C), BF16, qkv)
    lse = empty((B * H * L,), F32, qkv)
    _lib.call("ocn_attn_fwd", _chk(qkv, BF16, "qkv"), _chk(out, BF16, "out"), _chk(lse, F32, "lse"), so, order, counts, B, L, H, head_dim,
              int(causal), float(scale), _stream())
    return out, lse


def attn_bwd(qkv, out, dout, lse, B, L, H, causal, scale, head_dim=64, seq_off=None):
    dqkv = empty(qkv.shape, BF16, qkv)
    so, order, counts = _layout(seq_off).args(B, L) if seq_off is not None else (0, 0, 0)
    delta = empty((B * H * L,), F32, qkv) if seq_off is None else None  # workspace of the streamed kernels (exchanged between their launches); dense only
    _lib.call("ocn_attn_bwd", _chk(qkv, BF16, "qkv"), _chk(out, BF16, "out"), _chk(dout, BF16, "dout"), _chk(lse, F32, "lse"),
              _chk(dqkv, BF16, "dqkv"), _chk(delta, F32, "delta"), so, order, counts, B, L, H, head_dim, int(causal), float(scale), _stream())
    return dqkv


def attn_pooled_fwd(q, kv, rows, B, L, H, causal, scale, seq_off=None):
    """single-query attention of a tower's last block (head_dim 64): q [B, C] = the pooled rows' queries, kv [M, 2C] = K | V of every row;
    ``rows`` int32 [B] = absolute row of each sequence's pooled token; ``seq_off`` as in attn_fwd (packed rows).  -> out [B, C], lse [B*H]"""
    C = H * 64
    if q.shape != (B, C) or kv.shape[1] != 2 * C:
        raise RuntimeError(f"attn_pooled_fwd: q {tuple(q.shape)} / kv {tuple(kv.shape)} do not match B={B}, H={H}, head_dim 64")
    so = _chk(_layout(seq_off).seq_off, torch.int32, "seq_off") if seq_off is not None else 0
    out = empty((B, C), BF16, q)
    lse = empty((B * H,), F32, q)
    _lib.call("ocn_attn_pooled_fwd", _chk(q, BF16, "q"), _chk(kv, BF16, "kv"), _chk(out, BF16, "out"), _chk(lse, F32, "lse"), so,
              _chk(rows, torch.int32, "rows"), B, L, H, int(causal), float(scale), _stream())
    return out, lse


def attn_pooled_bwd(q, kv, out, dout, lse, rows, B, L, H, causal, scale, seq_off=None):
    """-> dq [B, C] bf16, dkv [M, 2C] bf16.  The kernel writes every key row of every sequence; rows of ``kv`` that belong to NO sequence can only
    exist with a packed layout whose last offset is below M -- the model never builds one (_TextPack allocates M = seq_off[B] rows, read from the
    same plan) -- and the dense layout must cover kv exactly, which is checked here: dkv feeds the K,V weight-gradient GEMM, an unwritten row
    would be uninitialised memory."""
    so = _chk(_layout(seq_off).seq_off, torch.int32, "seq_off") if seq_off is not None else 0
    C = H * 64
    if q.shape != (B, C) or kv.shape[1] != 2 * C or (seq_off is None and kv.shape[0] != B * L):
        raise RuntimeError(f"attn_pooled_bwd: q {tuple(q.shape)} / kv {tuple(kv.shape)} do not match B={B}, L={L}, H={H}, head_dim 64")
    dq = empty(q.shape, BF16, q)
    dkv = empty(kv.shape, BF16, kv)  # packed: M == seq_off[B] (model._TextPack takes M from the plan that wrote seq_off), so no row stays unwritten
    _lib.call("ocn_attn_pooled_bwd", _chk(q, BF16, "q"), _chk(kv, BF16, "kv"), _chk(out, BF16, "out"), _chk(dout, BF16, "dout"), _chk(lse, F32, "lse"),
              _chk(dq, BF16, "dq"), _chk(dkv, BF16, "dkv"), so, _chk(rows, torch.int32, "rows"), B, L, H, int(causal), float(scale), _stream())
    return dq, dkv


# ---- embeddings / pooling ----------------------------------------------------------------------------------
def _chk_keep(keep, B, G, name="keep"):
    """int32 [B, K] device tensor of kept patch indices (1 <= K <= G) -> (ptr, K); None = every patch in grid order -> (0, G)"""
    if keep is None:
        return 0, G
    if keep.dim() != 2 or keep.shape[0] != B or not 1 <= keep.shape[1] <= G:
        raise RuntimeError(f"open_clip_amd: '{name}' must be int32 [B = {B}, K] with 1 <= K <= {G} (got {tuple(keep.shape)})")
    return _chk(keep, torch.int32, name), keep.shape[1]


def patch_keep_plan(seed, B, G, K, device):
    """the kept patches of a patch-dropout step, chosen on the device (ocn_patch_keep_plan): (keep int32 [B, K] ascending per image,
    inv int32 [B, G]).  ``seed`` is a host integer; nothing is read back."""
    if not 1 <= K <= G:
        raise RuntimeError(f"patch_keep_plan: K = {K} outside [1, G = {G}]")
    keep = torch.empty((B, K), dtype=torch.int32, device=device)
    inv = torch.empty((B, G), dtype=torch.int32, device=device)
    _lib.call("ocn_patch_keep_plan", int(seed) & 0x7FFFFFFFFFFFFFFF, B, G, K, _chk(keep, torch.int32, "keep"), _chk(inv, torch.int32, "inv"), _stream())
    return keep, inv


def patch_keep_inverse(keep, G):
    """inv int32 [B, G] of a caller-supplied ``keep`` (distinct indices per image, any order): position of patch g in keep[b], or -1"""
    B = keep.shape[0]
    kp, K = _chk_keep(keep, B, G)
    inv = torch.empty((B, G), dtype=torch.int32, device=keep.device)
    _lib.call("ocn_patch_keep_inverse", kp, _chk(inv, torch.int32, "inv"), B, G, K, _stream())
    return inv


def patchify(image, P, Kpad, keep=None):
    """``keep`` (int32 [B, K]): only those patches, row b*K + j = patch keep[b, j] of image b (patch dropout)"""
    B, Cin, H, W = image.shape
    if Cin != 3:
        raise RuntimeError("patchify: images must have 3 channels")
    is16 = image.dtype == BF16
    kp, K = _chk_keep(keep, B, (H // P) * (W // P))
    out = empty((B * K, Kpad), BF16, image)
    _lib.call("ocn_patchify", _chk(image, BF16 if is16 else F32, "image"), int(is16), kp, K, _chk(out, BF16, "patches"), B, H, W, P, Kpad, _stream())
    return out


def patchify_u8(image, P, Kpad, mean, std, hwc, keep=None):
    """uint8 pixels -> normalised bf16 patch matrix (ToTensor + Normalize fused; see ocn_patchify_u8); ``keep`` as in ``patchify``"""
    import ctypes
    if image.dtype != torch.uint8 or image.dim() != 4:
        raise RuntimeError("patchify_u8: expected a 4-D uint8 image batch")
    B = image.shape[0]
    H, W = (image.shape[1], image.shape[2]) if hwc else (image.shape[2], image.shape[3])
    if (image.shape[3] if hwc else image.shape[1]) != 3:
        raise RuntimeError("patchify_u8: images must have 3 channels")
    m3, s3 = (ctypes.c_float * 3)(*[float(v) for v in mean]), (ctypes.c_float * 3)(*[float(v) for v in std])
    kp, K = _chk_keep(keep, B, (H // P) * (W // P))
    out = empty((B * K, Kpad), BF16, image)
    _lib.call("ocn_patchify_u8", _chk(image, torch.uint8, "image"), int(hwc), m3, s3, kp, K, _chk(out, BF16, "patches"), B, H, W, P, Kpad, _stream())
    return out


def resized_crop_u8(src, boxes, size, out=None):
    """crop + antialiased bicubic resize on the device (ocn_resized_crop_u8): ``src`` uint8 [B, Hs, Ws, 3], ``boxes`` int32 [B, 4] =
    (top, left, height, width) on the same device, ``size`` an int or (Ho, Wo) -> uint8 [B, Ho, Wo, 3] (``out`` when given).  The box contents are
    not checked here (they are device data; ``input_pipeline.check_boxes`` checks them on the host): the kernel clamps a bad box."""
    Ho, Wo = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    if src.dtype != torch.uint8:
        raise RuntimeError(f"resized_crop_u8: 'src' must be uint8 (got {src.dtype})")
    if src.dim() != 4 or src.shape[3] != 3:
        raise RuntimeError(f"resized_crop_u8: 'src' must be [B, Hs, Ws, 3] (channels last, 3 channels; got {tuple(src.shape)})")
    B, Hs, Ws = src.shape[0], src.shape[1], src.shape[2]
    if boxes.dim() != 2 or tuple(boxes.shape) != (B, 4):
        raise RuntimeError(f"resized_crop_u8: 'boxes' must be int32 [B = {B}, 4] = (top, left, height, width) (got {tuple(boxes.shape)})")
    sp, bp = _chk(src, torch.uint8, "src"), _chk(boxes, torch.int32, "boxes")
    if boxes.device != src.device:
        raise RuntimeError(f"resized_crop_u8: 'boxes' ({boxes.device}) and 'src' ({src.device}) must be on one device")
    if out is None:
        out = empty((B, Ho, Wo, 3), torch.uint8, src)
    elif tuple(out.shape) != (B, Ho, Wo, 3) or out.device != src.device:
        raise RuntimeError(f"resized_crop_u8: 'out' must be uint8 {(B, Ho, Wo, 3)} on {src.device} (got {tuple(out.shape)} on {out.device})")
    _lib.call("ocn_resized_crop_u8", sp, B, Hs, Ws, bp, _chk(out, torch.uint8, "out"), Ho, Wo, _stream())
    return out


def resample_u8(arena, offsets, plan, size, fill=0, out=None):
    """antialiased bicubic resampling of ragged sources on the device (ocn_resample_u8; defined in include/openclip_hip.h): ``arena`` uint8 [bytes]
    (a multiple of 4; 16-byte aligned) holds B tightly packed HWC images, ``offsets`` int64 [B] their byte offsets (multiples of 16), ``plan`` int32
    [B, 10] = (Hs, Ws, top, left, nh, nw, Rh, Rw, oy, ox) on the same device, ``size`` an int or (Ho, Wo), ``fill`` the colour 0..255 of output pixels
    outside the resized image -> uint8 [B, Ho, Wo, 3] (``out`` when given).  The contents of ``offsets`` and ``plan`` are not checked here (they are
    device data; ``input_pipeline.check_resample_plan`` checks them on the host): the kernel clamps every size, coordinate and address."""
    Ho, Wo = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    if arena.dtype != torch.uint8:
        raise RuntimeError(f"resample_u8: 'arena' must be uint8 (got {arena.dtype})")
    if arena.dim() != 1 or arena.numel() == 0 or arena.numel() % 4 != 0:
        raise RuntimeError(f"resample_u8: 'arena' must be a flat byte buffer [bytes] with bytes a positive multiple of 4 (got {tuple(arena.shape)})")
    if offsets.dim() != 1 or offsets.numel() == 0:
        raise RuntimeError(f"resample_u8: 'offsets' must be int64 [B] with B >= 1 (got {tuple(offsets.shape)})")
    B = offsets.shape[0]
    if tuple(plan.shape) != (B, 10):
        raise RuntimeError(f"resample_u8: 'plan' must be int32 [B = {B}, 10] = (Hs, Ws, top, left, nh, nw, Rh, Rw, oy, ox) (got {tuple(plan.shape)})")
    if isinstance(fill, bool) or not isinstance(fill, int) or not 0 <= fill <= 255:
        raise RuntimeError(f"resample_u8: 'fill' must be an int in [0, 255] (got {fill!r})")
    ap, op, pp = _chk(arena, torch.uint8, "arena"), _chk(offsets, torch.int64, "offsets"), _chk(plan, torch.int32, "plan")
    if offsets.device != arena.device or plan.device != arena.device:
        raise RuntimeError(f"resample_u8: 'offsets' ({offsets.device}), 'plan' ({plan.device}) and 'arena' ({arena.device}) must be on one device")
    if out is None:
        out = empty((B, Ho, Wo, 3), torch.uint8, arena)
    elif tuple(out.shape) != (B, Ho, Wo, 3) or out.device != arena.device:
        raise RuntimeError(f"resample_u8: 'out' must be uint8 {(B, Ho, Wo, 3)} on {arena.device} (got {tuple(out.shape)} on {out.device})")
    _lib.call("ocn_resample_u8", ap, arena.numel(), op, pp, B, _chk(out, torch.uint8, "out"), Ho, Wo, fill, _stream())
    return out


POS_RESAMPLE_MODES = {"linear": 0, "bilinear": 0, "bicubic": 1}


def _pos_resample(name, t, rows_in, rows_out, prefix, src_hw, dst_hw, mode, antialias):
    if mode not in POS_RESAMPLE_MODES:
        raise NotImplementedError(f"{name}: mode {mode!r} is not implemented (one of {sorted(POS_RESAMPLE_MODES)})")
    if t.dim() != 2 or t.shape[0] != rows_in:
        raise RuntimeError(f"{name}: the table {tuple(t.shape)} is not [prefix + H*W = {rows_in}, C]")
    out = empty((rows_out, t.shape[1]), F32, t)
    _lib.call("ocn_" + name, _chk(t, F32, "table"), _chk(out, F32, "out"), int(prefix), int(src_hw[0]), int(src_hw[1]), int(dst_hw[0]), int(dst_hw[1]),
              t.shape[1], POS_RESAMPLE_MODES[mode], int(bool(antialias)), _stream())
    return out


def pos_resample(table, prefix, src_hw, dst_hw, mode="bicubic", antialias=True):
    """a position table at another grid (ocn_pos_resample_fwd; defined in include/openclip_hip.h): ``table`` fp32 [prefix + Hs*Ws, C] ->
    fp32 [prefix + Ho*Wo, C]; the ``prefix`` rows are copied, the grid rows are ``F.interpolate(size=dst_hw, mode, antialias, align_corners=False)`` per
    channel.  ``mode``: "bicubic", "bilinear" or "linear"; the 1-D text table is ``src_hw = (1, L)``, ``dst_hw = (1, L')``."""
    return _pos_resample("pos_resample_fwd", table, prefix + src_hw[0] * src_hw[1], prefix + dst_hw[0] * dst_hw[1], prefix, src_hw, dst_hw, mode, antialias)


def pos_resample_bwd(dout, prefix, src_hw, dst_hw, mode="bicubic", antialias=True):
    """the transposed map (ocn_pos_resample_bwd): ``dout`` fp32 [prefix + Ho*Wo, C], the gradient of ``pos_resample``'s result -> the gradient
    fp32 [prefix + Hs*Ws, C] of its ``table``; gather form, the same bits every run"""
    return _pos_resample("pos_resample_bwd", dout, prefix + dst_hw[0] * dst_hw[1], prefix + src_hw[0] * src_hw[1], prefix, src_hw, dst_hw, mode, antialias)


def color_jitter_u8(img, factors, plan, out=None):
    """colour jitter + grayscale on the device (ocn_color_jitter_u8; the arithmetic is defined in include/openclip_hip.h): ``img`` uint8 [B, H, W, 3],
    ``factors`` float32 [B, 4] = (brightness, contrast, saturation, hue) and ``plan`` int32 [B] (four 3-bit step codes from the low bits up, bit 12 =
    grayscale) on the same device -> uint8 [B, H, W, 3]: a new tensor, or ``out`` when given (``out=img`` works in place).  The parameters are not
    checked here (they are device data; ``input_pipeline.check_jitter`` checks them on the host): the kernel takes no address from them."""
    if img.dtype != torch.uint8:
        raise RuntimeError(f"color_jitter_u8: 'img' must be uint8 (got {img.dtype})")
    if img.dim() != 4 or img.shape[3] != 3:
        raise RuntimeError(f"color_jitter_u8: 'img' must be [B, H, W, 3] (channels last, 3 channels; got {tuple(img.shape)})")
    B, H, W = img.shape[0], img.shape[1], img.shape[2]
    if tuple(factors.shape) != (B, 4):
        raise RuntimeError(f"color_jitter_u8: 'factors' must be float32 [B = {B}, 4] = (brightness, contrast, saturation, hue) (got {tuple(factors.shape)})")
    if tuple(plan.shape) != (B,):
        raise RuntimeError(f"color_jitter_u8: 'plan' must be int32 [B = {B}] (got {tuple(plan.shape)})")
    ip, fp, pp = _chk(img, torch.uint8, "img"), _chk(factors, F32, "factors"), _chk(plan, torch.int32, "plan")
    if factors.device != img.device or plan.device != img.device:
        raise RuntimeError(f"color_jitter_u8: 'factors' ({factors.device}), 'plan' ({plan.device}) and 'img' ({img.device}) must be on one device")
    if out is None:
        out = empty((B, H, W, 3), torch.uint8, img)
    elif tuple(out.shape) != (B, H, W, 3) or out.device != img.device:
        raise RuntimeError(f"color_jitter_u8: 'out' must be uint8 {(B, H, W, 3)} on {img.device} (got {tuple(out.shape)} on {out.device})")
    mean_ws = empty((B,), F32, img)  # the contrast means: written by the first launch, read by the second
    _lib.call("ocn_color_jitter_u8", ip, B, H, W, fp, pp, _chk(mean_ws, F32, "mean_ws"), _chk(out, torch.uint8, "out"), _stream())
    return out


def embed_assemble_fwd(patch_out, cls, pos, B, G, C, keep=None):
    """emb fp32 [B * (K + 1), C]: class token + position 0, then patch_out[b*K + j] + pos[1 + keep[b, j]] (``keep`` None: all G patches in order)"""
    kp, K = _chk_keep(keep, B, G)
    if tuple(patch_out.shape) != (B * K, C) or tuple(pos.shape) != (G + 1, C) or cls.numel() != C:
        raise RuntimeError("embed_assemble_fwd: patch_out must be [B*K, C], pos [G+1, C], cls [C]")
    emb = empty((B * (K + 1), C), F32, patch_out)
    _lib.call("ocn_embed_assemble_fwd", _chk(patch_out, F32, "patch_out"), _chk(cls, F32, "cls"), _chk(pos, F32, "pos"), kp,
              _chk(emb, F32, "emb"), B, G, K, C, _stream())
    return emb


def embed_assemble_bwd(demb, dpos, dcls, B, G, C, deterministic=False, inv=None, K=None, zero_dpatch=False):
    """dpatch bf16 [B*K, C]; dpos [G+1, C] / dcls [C] are accumulated into (``inv`` int32 [B, G] from patch_keep_plan / patch_keep_inverse, with the
    ``K`` of its keep; None: all G patches in order).
    The kernel reaches dpatch through ``inv`` alone: a row of ``keep`` that ``inv`` does not point back to (a caller's keep with a repeated or an
    out-of-range index) is never written.  ``zero_dpatch``: start from zeros, so that such a row adds nothing to the weight gradient (for an
    ``inv`` built from a caller's keep; the plan kernel's own ``inv`` covers every row)."""
    K = G if K is None else K
    if (inv is not None and tuple(inv.shape) != (B, G)) or tuple(demb.shape) != (B * (K + 1), C) or tuple(dpos.shape) != (G + 1, C) or dcls.numel() != C:
        raise RuntimeError("embed_assemble_bwd: demb must be [B*(K+1), C], inv [B, G], dpos [G+1, C], dcls [C]")
    dpatch = torch.zeros((B * K, C), dtype=BF16, device=demb.device) if zero_dpatch else empty((B * K, C), BF16, demb)
    _lib.call("ocn_embed_assemble_bwd", _chk(demb, F32, "demb"), _chk(inv, torch.int32, "inv"), _chk(dpatch, BF16, "dpatch"),
              _chk(dpos, F32, "dpos"), _chk(dcls, F32, "dcls"), B, G, K, C, int(deterministic), _stream())
    return dpatch


def token_embed_fwd(tokens, table, pos, posidx=None):
    """x fp32 [M, C] = table[tokens] + pos[position]: ``tokens`` is [B, L] (dense: row b*L + l carries position l) or, with ``posidx``
    (int32 [M]), the [M] ids of a packed batch (seq_pack_rows)"""
    if tokens.dim() != (2 if posidx is None else 1) or (posidx is not None and posidx.shape != tokens.shape):
        raise RuntimeError(f"token_embed_fwd: tokens must be [B, L], or [M] with posidx [M] (got {tuple(tokens.shape)})")
    M, L = tokens.numel(), (tokens.shape[1] if posidx is None else pos.shape[0])
    vocab, C = table.shape
    x = empty((M, C), F32, table)
    _lib.call("ocn_token_embed_fwd", _chk(tokens, torch.int64, "tokens"), _chk(posidx, torch.int32, "posidx"), _chk(table, F32, "table"),
              _chk(pos, F32, "pos"), _chk(x, F32, "x"), M, L, C, vocab, _stream())
    return x


def token_embed_bwd(tokens, dx, dtable, dpos, deterministic=False, seq_off=None):
    """dtable += the rows of ``dx`` by token id (``dtable`` must be zero on entry), dpos += by position.  ``tokens`` is [B, L], or the [M]
    packed ids with ``seq_off`` (int32 [B+1]; L = the rows of ``dpos``).  The device sort of the ids is index plumbing (torch.sort); all
    arithmetic is in ocn_token_embed_bwd."""
    if tokens.dim() != (2 if seq_off is None else 1):
        raise RuntimeError(f"token_embed_bwd: tokens must be [B, L], or [M] with seq_off (got {tuple(tokens.shape)})")
    B, L = tokens.shape if seq_off is None else (seq_off.numel() - 1, dpos.shape[0])
    vocab, C = dtable.shape
    keys, order = torch.sort(tokens.reshape(-1), stable=bool(deterministic))  # the reproducible form sums a run in sorted order: equal ids must keep their order
    is16 = dx.dtype == BF16
    _lib.call("ocn_token_embed_bwd", _chk(keys, torch.int64, "sorted_tokens"), _chk(order, torch.int64, "order"),
              _chk(dx, BF16 if is16 else F32, "dx"), int(is16), _chk(dtable, F32, "dtable"), _chk(dpos, F32, "dpos"),
              _chk(seq_off, torch.int32, "seq_off"), B, L, tokens.numel(), C, vocab, int(deterministic), _stream())


def seq_pack_plan(text, vocab=None, buckets=False):
    """(eot [B], plan, last_row [B], order) int32 on the device: the packed layout of a text batch.  plan[0..B] = seq_off
    (ocn_seq_pack_plan; plan[B] = the packed row count M), plan[B+1] = the number of ids outside [0, vocab) when ``vocab`` is given
    (ocn_token_range_check), plan[B+2 ..] = the ceil(L / 32) bucket counts when ``buckets`` (ocn_seq_bucket_plan; ``order`` = the
    sequence ids grouped by block count, else None)"""
    B, L = text.shape
    nbk = (L + 31) // 32 if buckets else 0
    eot, plan, last_row = empty((B,), torch.int32, text), empty((B + 2 + nbk,), torch.int32, text), empty((B,), torch.int32, text)
    _lib.call("ocn_seq_pack_plan", _chk(text, torch.int64, "text"), _chk(eot, torch.int32, "eot"), _chk(plan, torch.int32, "seq_off"),
              _chk(last_row, torch.int32, "last_row"), B, L, _stream())
    if vocab is not None:
        _lib.call("ocn_token_range_check", text.data_ptr(), B * L, int(vocab), plan.data_ptr() + 4 * (B + 1), _stream())
    else:
        plan[B + 1:B + 2].zero_()
    order = None
    if buckets:
        order = empty((B,), torch.int32, text)
        _lib.call("ocn_seq_bucket_plan", plan.data_ptr(), _chk(order, torch.int32, "order"), plan.data_ptr() + 4 * (B + 2), B, L, _stream())
    return eot, plan, last_row, order


def token_range_check(text, vocab):
    """int32 [1] on the device: how many ids of ``text`` lie outside [0, vocab)"""
    bad = empty((1,), torch.int32, text)
    _lib.call("ocn_token_range_check", _chk(text, torch.int64, "text"), text.numel(), int(vocab), _chk(bad, torch.int32, "bad"), _stream())
    return bad


def seq_pack_rows(text, seq_off, M):
    B, L = text.shape
    tokens, posidx = empty((M,), torch.int64, text), empty((M,), torch.int32, text)
    _lib.call("ocn_seq_pack_rows", _chk(text, torch.int64, "text"), _chk(seq_off, torch.int32, "seq_off"), _chk(tokens, torch.int64, "tokens"),
              _chk(posidx, torch.int32, "posidx"), B, L, _stream())
    return tokens, posidx


def argmax_rows(text):
    B, L = text.shape
    idx = empty((B,), torch.int32, text)
    _lib.call("ocn_argmax_rows", _chk(text, torch.int64, "text"), _chk(idx, torch.int32, "idx"), B, L, _stream())
    return idx


def gather_rows(x, idx, B, L):
    """fp32 [B, C] rows of ``x`` (fp32, or bf16: the image tower's bf16 residual stream)"""
    C = x.shape[1]
    out = empty((B, C), F32, x)
    x16 = x.dtype == BF16
    _lib.call("ocn_gather_rows", _chk(x, BF16 if x16 else F32, "x"), int(x16), _chk(idx, torch.int32, "idx"), _chk(out, F32, "out"), B, L, C, _stream())
    return out


def gather_rows_bf16(x, idx, B, L):
    C = x.shape[1]
    out = empty((B, C), BF16, x)
    _lib.call("ocn_gather_rows_bf16", _chk(x, BF16, "x"), _chk(idx, torch.int32, "idx"), _chk(out, BF16, "out"), B, L, C, _stream())
    return out


def scatter_rows(d, idx, dx, B, L, dx16=None):
    C = d.shape[1]
    _lib.call("ocn_scatter_rows", _chk(d, F32, "d"), _chk(idx, torch.int32, "idx"), _chk(dx, F32, "dx"), _chk(dx16, BF16, "dx16"), B, L, C, _stream())
    return dx


def scatter_add_rows(d, idx, dx, B, L, dx16=None):
    """dx[row_b] += d[b]; dx16[row_b] = bf16(dx[row_b]); ``dx`` None (bf16 gradient stream): dx16[row_b] = bf16(dx16[row_b] + d[b])"""
    C = d.shape[1]
    _lib.call("ocn_scatter_add_rows", _chk(d, F32, "d"), _chk(idx, torch.int32, "idx"), _chk(dx, F32, "dx"), _chk(dx16, BF16, "dx16"), B, L, C, _stream())
    return dx


def mean_pool_fwd(x, B, T, skip=1):
    """fp32 [B, C]: the mean over the tokens ``skip .. T-1`` of every image of ``x`` [B*T, C] (fp32, or bf16: the image tower's bf16 residual stream);
    fp32 sums in a fixed order and one correctly rounded division by ``T - skip`` (``x[:, 1:].mean(dim=1)`` with ``skip = 1``)"""
    C = x.shape[1]
    if x.dim() != 2 or x.shape[0] != B * T:
        raise RuntimeError(f"mean_pool_fwd: x {tuple(x.shape)} is not [B*T = {B * T}, C]")
    out = empty((B, C), F32, x)
    x16 = x.dtype == BF16
    _lib.call("ocn_mean_pool_fwd", _chk(x, BF16 if x16 else F32, "x"), int(x16), _chk(out, F32, "out"), B, T, int(skip), C, _stream())
    return out


def mean_pool_bwd(dpooled, B, T, skip=1, want_f32=True, want_bf16=True):
    """(dx fp32 | None, dx bf16 | None), each [B*T, C] and written in full: zeros in the rows ``t < skip`` of every image, ``dpooled[b] / (T - skip)`` in
    the others (the bf16 form is the rounding of the fp32 one)"""
    if dpooled.dim() != 2 or dpooled.shape[0] != B or not (want_f32 or want_bf16):
        raise RuntimeError(f"mean_pool_bwd: dpooled {tuple(dpooled.shape)} is not [B = {B}, C], or no output was asked for")
    C = dpooled.shape[1]
    dx = empty((B * T, C), F32, dpooled) if want_f32 else None
    dx16 = empty((B * T, C), BF16, dpooled) if want_bf16 else None
    _lib.call("ocn_mean_pool_bwd", _chk(dpooled, F32, "dpooled"), _chk(dx, F32, "dx"), _chk(dx16, BF16, "dx16"), B, T, int(skip), C, _stream())
    return dx, dx16


def l2norm_fwd(x, eps=1e-12):
    B, E = x.shape
    y, y16, inv = empty((B, E), F32, x), empty((B, E), BF16, x), empty((B,), F32, x)
    _lib.call("ocn_l2norm_fwd", _chk(x, F32, "x"), _chk(y, F32, "y"), _chk(y16, BF16, "y16"), _chk(inv, F32, "inv"), B, E, float(eps), _stream())
    return y, y16, inv


def l2norm_bwd(dy, y, inv):
    B, E = y.shape
    dx = empty((B, E), F32, y)
    _lib.call("ocn_l2norm_bwd", _chk(dy, F32, "dy"), _chk(y, F32, "y"), _chk(inv, F32, "inv"), _chk(dx, F32, "dx"), B, E, _stream())
    return dx


# ---- losses ---------------------------------------------------------------------------------------------------
def softmax_ce_rows(logits, G, N, label_offset, loss_scale, grad_scale, inv_logit_scale, loss_sum, dscale_sum, det_rows=None):
    """``det_rows`` (fp32 [R, 3]): the rows' contributions are written there instead of being added atomically (reproducible form)"""
    pl, ld = _chk2d(logits, F32, "logits")
    pg, ldg = _chk2d(G, BF16, "G")
    _lib.call("ocn_softmax_ce_rows", pl, ld, pg, ldg, logits.shape[0], N, int(label_offset), float(loss_scale), float(grad_scale),
              float(inv_logit_scale), _chk(loss_sum, F32, "loss_sum"), _chk(dscale_sum, F32, "dscale_sum"), _chk(det_rows, F32, "det_rows"), _stream())


def distill_rows(student, teacher, G, N, loss_scale, grad_scale, inv_logit_scale, loss_sum, dscale_sum, det_rows=None):
    """rows of softmax(teacher) against log_softmax(student) (ocn_distill_rows): G = (p - q) * grad_scale, loss_sum += (lse(l) - sum q l) * loss_scale,
    dscale_sum += sum(G * l) * inv_logit_scale; ``det_rows`` as for ``softmax_ce_rows``"""
    if student.shape != teacher.shape:
        raise RuntimeError(f"distill_rows: student logits {tuple(student.shape)} and teacher logits {tuple(teacher.shape)} differ in shape")
    ps, ld_s = _chk2d(student, F32, "student")
    pt, ld_t = _chk2d(teacher, F32, "teacher")
    pg, ldg = _chk2d(G, BF16, "G")
    _lib.call("ocn_distill_rows", ps, ld_s, pt, ld_t, pg, ldg, student.shape[0], N, float(loss_scale), float(grad_scale), float(inv_logit_scale),
              _chk(loss_sum, F32, "loss_sum"), _chk(dscale_sum, F32, "dscale_sum"), _chk(det_rows, F32, "det_rows"), _stream())


def fused_logits_ce(xs16, y16, G, N, label_offset, loss_scale, grad_scale, loss_sum, dscale_sum):
    """cross-entropy of the rows of xs16 @ y16[:N]^T against arange + label_offset without materialising the logits, in ONE pass of the MFMA GEMM
    (ocn_fused_logits_ce): fills G bf16 [R, ldg] with exp(logit - shift_r) and returns ``rowscale`` fp32 [R] = grad_scale / sum_j G[r, j] -- the softmax part
    of the logit gradient is G * rowscale[:, None]; accumulates loss_sum and dscale_sum (= sum((softmax - onehot) * grad_scale * logits))"""
    px, ldx = _chk2d(xs16, BF16, "xs16")
    py, ldy = _chk2d(y16, BF16, "y16")
    pg, ldg = _chk2d(G, BF16, "G")
    R, E = xs16.shape
    ws = torch.empty(_lib.load().ocn_fused_logits_ce_workspace_floats(R, N), dtype=F32, device=xs16.device)
    rowscale = torch.empty(R, dtype=F32, device=xs16.device)
    _lib.call("ocn_fused_logits_ce", px, ldx, py, ldy, R, N, E, int(label_offset), float(loss_scale), float(grad_scale), pg, ldg,
              ws.data_ptr(), rowscale.data_ptr(), _chk(loss_sum, F32, "loss_sum"), _chk(dscale_sum, F32, "dscale_sum"), _stream())
    return rowscale


def fused_logits_ce_supported(R, N, E):
    return E % 128 == 0 and N % 8 == 0 and R >= 256


def siglip_rows(logits, G, N, label_offset, negative_only, bias, loss_scale, grad_scale, inv_logit_scale, loss_sum, dscale_sum, dbias_sum, det_rows=None):
    """``bias``: the bias the logits carry -- a python float, or a 1-element fp32 DEVICE tensor (no host read); dscale_sum += sum(g * (logits - bias))"""
    pl, ld = _chk2d(logits, F32, "logits")
    pg, ldg = _chk2d(G, BF16, "G")
    bias_dev = _chk(bias, F32, "bias") if torch.is_tensor(bias) else 0
    _lib.call("ocn_siglip_rows", pl, ld, pg, ldg, logits.shape[0], N, int(label_offset), int(negative_only), 0.0 if bias_dev else float(bias), bias_dev,
              float(loss_scale), float(grad_scale), float(inv_logit_scale), _chk(loss_sum, F32, "loss_sum"),
              _chk(dscale_sum, F32, "dscale_sum"), _chk(dbias_sum, F32, "dbias_sum"), _chk(det_rows, F32, "det_rows"), _stream())


# ---- optimizer ----------------------------------------------------------------------------------------------------
def sumsq_accum(x, out):
    _lib.call("ocn_sumsq_accum", _chk(x, F32, "x"), x.numel(), _chk(out, F32, "out"), _stream())


def adamw_step(w, g, m, v, lr, beta1, beta2, eps, weight_decay, step, w_bf16=None, clip_coef=None):
    _lib.call("ocn_adamw_step", _chk(w, F32, "w"), _chk(g, F32, "g"), _chk(m, F32, "m"), _chk(v, F32, "v"),
              _chk(w_bf16, BF16, "w_bf16"), w.numel(), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
              int(step), _chk(clip_coef, F32, "clip_coef"), _stream())


def sumsq_multi(entries, chunks, n_chunks, out, chunk_ws=None):
    """out[0] += sum of g^2 over an AdamEntry table (ocn_sumsq_multi; tables.py::AdamTables); ``chunk_ws`` fp32 [n_chunks]: the fixed-order form"""
    _lib.call("ocn_sumsq_multi", _chk(entries, torch.uint8, "entries"), _chk(chunks, torch.int32, "chunks"), int(n_chunks), _chk(out, F32, "out"),
              _chk(chunk_ws, F32, "chunk_ws"), _stream())


def adamw_multi(entries, chunks, n_chunks, beta1, beta2, eps, gnorm_sq=None, max_norm=0.0):
    """torch.optim.AdamW's update of every chunk in one launch, operand copies included (ocn_adamw_multi); ``gnorm_sq``: the clip's squared norm"""
    _lib.call("ocn_adamw_multi", _chk(entries, torch.uint8, "entries"), _chk(chunks, torch.int32, "chunks"), int(n_chunks), float(beta1), float(beta2),
              float(eps), _chk(gnorm_sq, F32, "gnorm_sq"), float(max_norm), _stream())


def nadamw_multi(entries, chunks, n_chunks, one_minus_beta1, beta2, one_minus_beta2, eps, gnorm_sq=None, max_norm=0.0):
    """torch.optim.NAdam(decoupled_weight_decay=True)'s update over the same tables (ocn_nadamw_multi)"""
    _lib.call("ocn_nadamw_multi", _chk(entries, torch.uint8, "entries"), _chk(chunks, torch.int32, "chunks"), int(n_chunks), float(one_minus_beta1),
              float(beta2), float(one_minus_beta2), float(eps), _chk(gnorm_sq, F32, "gnorm_sq"), float(max_norm), _stream())


def ema_lerp_multi(entries, chunks, n_chunks, weight):
    """ema = lerp(ema, src, weight) for every record of ``entries`` in one launch (ocn_ema_lerp_multi; tables as ema.py::ema_plan builds them)"""
    _lib.call("ocn_ema_lerp_multi", _chk(entries, torch.uint8, "entries"), _chk(chunks, torch.int32, "chunks"), int(n_chunks), float(weight), _stream())


# ---- Muon (optim.py::NativeMuon) ------------------------------------------------------------------------------------
def _chk3d(t, name):
    """bf16 [batch, rows, cols], unit inner stride, any row / batch stride -> (ptr, ld, batch stride)"""
    if not t.is_cuda:
        raise RuntimeError(f"open_clip_amd: '{name}' must live on the MI355X (got {t.device}); there is no CPU path")
    if t.dtype != BF16 or t.dim() != 3 or t.stride(2) != 1:
        raise RuntimeError(f"open_clip_amd: '{name}' must be a 3-D {BF16} stack of matrices with unit inner stride")
    return t.data_ptr(), t.stride(1), (t.stride(0) if t.shape[0] > 1 else 0)


def gemm_nt_batched(a, b, out, resid=None, out_t=None, alpha=1.0, beta=0.0):
    """out[i] = bf16(alpha * a[i] @ b[i]^T + beta * resid[i]) for every i in one launch (ocn_gemm_nt_batched); a [batch, M, K], b [batch, N, K],
    out / resid [batch, M, N], out_t [batch, N, M] (optional: the transposed result as well).  ``out`` may be ``resid`` itself."""
    pa, lda, sa = _chk3d(a, "a")
    pb, ldb, sb = _chk3d(b, "b")
    po, ldc, sc = _chk3d(out, "out")
    batch, M, K = a.shape
    N = b.shape[1]
    if b.shape != (batch, N, K) or out.shape != (batch, M, N) or (resid is not None and resid.shape != out.shape) or \
            (out_t is not None and out_t.shape != (batch, N, M)):
        raise RuntimeError(f"gemm_nt_batched: shape mismatch a{tuple(a.shape)} b{tuple(b.shape)} out{tuple(out.shape)}")
    pr, ldr, sr = (0, 0, 0) if resid is None else _chk3d(resid, "resid")
    pt, ldt, st = (0, 0, 0) if out_t is None else _chk3d(out_t, "out_t")
    _lib.call("ocn_gemm_nt_batched", pa, lda, sa, pb, ldb, sb, po, ldc, sc, pr, ldr, sr, pt, ldt, st, M, N, K, batch, float(alpha), float(beta), _stream())
    return out


def muon_momentum_multi(entries, n_entries, chunks, n_chunks, momentum, nesterov, gnorm_sq, max_norm, chunk_ws, inv_norm):
    """momentum buffers, update directions' tile partials and inv_norm = 1 / (||u|| + 1e-7) per matrix (ocn_muon_momentum_multi; tables as optim.py builds them)"""
    _lib.call("ocn_muon_momentum_multi", _chk(entries, torch.uint8, "entries"), int(n_entries), _chk(chunks, torch.int32, "chunks"), int(n_chunks),
              float(momentum), int(bool(nesterov)), _chk(gnorm_sq, F32, "gnorm_sq"), float(max_norm), _chk(chunk_ws, F32, "chunk_ws"),
              _chk(inv_norm, F32, "inv_norm"), _stream())


def muon_normalize_multi(entries, chunks, n_chunks, momentum, nesterov, gnorm_sq, max_norm, inv_norm):
    """X = bf16(u * inv_norm) into the workspace images of every matrix (ocn_muon_normalize_multi)"""
    _lib.call("ocn_muon_normalize_multi", _chk(entries, torch.uint8, "entries"), _chk(chunks, torch.int32, "chunks"), int(n_chunks), float(momentum),
              int(bool(nesterov)), _chk(gnorm_sq, F32, "gnorm_sq"), float(max_norm), _chk(inv_norm, F32, "inv_norm"), _stream())


def muon_apply_multi(entries, chunks, n_chunks):
    """w = w * decay - step * X and the bf16 operand copies, for every matrix (ocn_muon_apply_multi)"""
    _lib.call("ocn_muon_apply_multi", _chk(entries, torch.uint8, "entries"), _chk(chunks, torch.int32, "chunks"), int(n_chunks), _stream())


def muon_axpby(acc, resid, out, out_t=None, beta=1.0):
    """out = bf16(acc + beta * resid), out_t = out^T (optional); acc fp32 [rows, cols], the rest bf16, all contiguous (ocn_muon_axpby)"""
    rows, cols = acc.shape
    if resid.shape != acc.shape or out.shape != acc.shape or (out_t is not None and out_t.shape != (cols, rows)):
        raise RuntimeError("muon_axpby: shape mismatch")
    _lib.call("ocn_muon_axpby", _chk(acc, F32, "acc"), _chk(resid, BF16, "resid"), _chk(out, BF16, "out"), _chk(out_t, BF16, "out_t"), rows, cols,
              float(beta), _stream())
    return out


# ---- validation metrics (open_clip_train/metrics.py, zero_shot.py) -------------------------------------------------
def _on_gpu(t, dtype, name):
    """device and dtype as ``_chk``; a strided view is made contiguous here (the rank kernels take dense rows only)"""
    if not t.is_cuda:
        raise RuntimeError(f"open_clip_amd: '{name}' must live on the MI355X (got {t.device}); there is no CPU path")
    if t.dtype != dtype:
        raise RuntimeError(f"open_clip_amd: '{name}' must be {dtype} (got {t.dtype})")
    return t.contiguous()


def split_bf16x3(x, role):
    """fp32 [R, E] -> bf16 [R, 3 * Ep] (Ep = E rounded up to 32): hi = bf16(x), lo = bf16(x - hi); ``role`` "query" writes [hi | lo | hi], "candidate"
    [hi | hi | lo] -- one product of the two is hi.hi + lo.hi + hi.lo (ocn_split_bf16x3)"""
    if role not in ("query", "candidate"):
        raise ValueError(f"split_bf16x3: role must be 'query' or 'candidate' (got {role!r})")
    if x.dim() != 2:
        raise RuntimeError("split_bf16x3: x must be 2-D")
    x = _on_gpu(x, F32, "x")
    R, E = x.shape
    out = empty((R, 3 * ((E + 31) // 32 * 32)), BF16, x)
    _lib.call("ocn_split_bf16x3", x.data_ptr(), out.data_ptr(), R, E, 0 if role == "query" else 1, _stream())
    return out


def pad_cast_bf16(x):
    """fp32 [R, E] -> bf16 [R, Ep], zero-padded to a multiple of 32 columns: the one-segment operand of the bf16 rank mode (ocn_cast_f32_bf16)"""
    if x.dim() != 2:
        raise RuntimeError("pad_cast_bf16: x must be 2-D")
    x = _on_gpu(x, F32, "x")
    E = x.shape[1]
    if E % 32:
        x = torch.nn.functional.pad(x, (0, 32 - E % 32))
    return cast_bf16(x)


def label_ranks(q16, c16, labels=None, return_target=False):
    """rank[r] = #{j : s[r, j] > t[r] or (s[r, j] == t[r] and j < labels[r])} with s = q16 @ c16^T in fp32 and t[r] = s[r, labels[r]] (ocn_label_ranks;
    metrics.py:156-163).  q16 bf16 [R, K], c16 bf16 [N, K], K % 32 == 0; labels int32 [R] in [0, N) or None = arange(R).  Returns int32 [R] (and the fp32
    targets, which leave the same tile routine as every other score)."""
    if q16.dim() != 2 or c16.dim() != 2 or q16.shape[1] != c16.shape[1]:
        raise RuntimeError(f"label_ranks: shape mismatch q{tuple(q16.shape)} c{tuple(c16.shape)}")
    q16, c16 = _on_gpu(q16, BF16, "q16"), _on_gpu(c16, BF16, "c16")
    R, K = q16.shape
    N = c16.shape[0]
    pl = 0
    if labels is not None:
        labels = _on_gpu(labels, torch.int32, "labels")
        if labels.shape != (R,):
            raise RuntimeError(f"label_ranks: labels must have shape ({R},), got {tuple(labels.shape)}")
        pl = labels.data_ptr()
    target, rank = empty((R,), F32, q16), empty((R,), torch.int32, q16)
    _lib.call("ocn_label_ranks", q16.data_ptr(), c16.data_ptr(), pl, target.data_ptr(), rank.data_ptr(), R, N, K, _stream())
    return (rank, target) if return_target else rank
