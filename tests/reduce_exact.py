"""Exact-arithmetic checks of the backward's reductions that are not GEMMs (helper module of tests/test_reduce_exact.py and
tests/test_reduce_exact_gpu.py): the table / position gradients of the token embedding, the position / class gradients of the image embedding,
ocn_colsum_f32, the LayerNorm backward's dw / db / dcol (and dx where 1 / C is a power of two) and the squared gradient norm of the clip.

The method is tests/gemm_exact.py's: operands hold small integers (or dyadic numbers with a known number of fraction bits), so every partial sum
a kernel can form is exact in fp32 in ANY order -- fp32 atomics, per-workgroup slabs, whole-run walks, LDS trees alike.  The output has to be
bit-equal to the float64 result, the atomic and the fixed-order form bit-equal to each other, and nothing has to be measured.  Every builder
asserts its own guard  largest magnitude x 2^(fraction bits) x summands < 2^24  (evaluated on the actual operands as  sum of |summand| / unit, which
bounds every partial sum of every subset): a badly chosen case fails here, on its inputs, not on the kernel.

Builders return CPU tensors and float64 references; the case tables are data.  The CPU test judges builders and references alone."""
import torch

from tests.gemm_exact import LIMIT, f32_exact, int_operand, rne_bf16  # noqa: F401  (re-exported to the two test modules)

ACC_R = 64  # what an accumulated-into tensor holds on entry: integers in [-64, 64]
CH = 64  # entries of the sorted id list per workgroup of the table-gradient kernel


def guard(sum_abs, unit=1.0, what=""):
    """every partial sum of summands whose absolute values add up to ``sum_abs`` (a number or a tensor: the largest element counts), all multiples
    of ``unit``, is exact in fp32"""
    worst = float(sum_abs.max()) if torch.is_tensor(sum_abs) else float(sum_abs)
    assert worst / unit < LIMIT, f"{what}: sum of |summands| {worst} in units of {unit} passes 2^24: partial sums can be inexact"


def acc_init(shape, generator):
    return int_operand(shape, ACC_R, generator, dtype=torch.float32)


# ---- 1. token embedding ---------------------------------------------------------------------------------------------------------
TOKEN_V = 2000
DX_R = 8
# (B, L, C, dx dtype): B across the 128-sequence chunk of dpos, C across the 128 x 4 columns a workgroup covers in one pass
TOKEN_DENSE_CASES = ((5, 150, 64, torch.float32), (128, 7, 192, torch.bfloat16), (129, 7, 512, torch.float32), (300, 5, 768, torch.bfloat16),
                     (128, 8, 1280, torch.float32))
# (B, L, C, dx dtype) of the packed form: the first 128 sequences have at most 3 tokens, so that for positions >= 3 the first batch chunk of
# dpos holds no sequence at all while the later ones do
TOKEN_PACKED_CASES = ((300, 20, 64, torch.float32), (300, 20, 768, torch.bfloat16))
_BASE_RUNS = (  # (raw id, count), ascending ids; entry ranges [first, last] in the comments
    (-5, 40), (-1, 24), (0, 2),  # ids below the vocabulary and id 0: ONE run of the clamped id 0 = [0, 65], the raw id changes exactly on the edge 63 | 64
    (2, 58), (5, 4),  # [124, 127]: a run that ends on entry 63 of its chunk
    (7, 64),  # [128, 191]: one whole chunk, other ids on both sides
    (8, 65),  # [192, 256]: 65 entries, ends on entry 0 of the next chunk ("at 64")
    (11, 62), (12, 1), (13, 1),  # single entries on both sides of the edge 319 | 320
    (20, 2), (21, 63),  # [323, 385]: ends on entry 1 of a chunk ("at 65")
    (30, 150),  # [386, 535]: spans three chunks, the shape of SOT / EOT / padding
)
_BASE_N = sum(c for _, c in _BASE_RUNS)


def token_runs(n, V=TOKEN_V):
    """the run-length table of a sorted id list of ``n`` entries: the fixed head above, rare ids in runs of 1 / 2 / 3 (every second id: the rows
    between them must stay zero), and at the end V-1, V, V+7 -- one run of the clamped id V-1 astride the last chunk edge, the raw id changing on it"""
    edge = (n - 1) // CH * CH  # the last chunk edge with entries on both sides
    assert n - edge >= 3 and edge - 3 > _BASE_N, n
    runs, left, tok, k = list(_BASE_RUNS), edge - 3 - _BASE_N, 40, 0
    while left > 0:
        c = min(left, 1 + k % 3)
        runs.append((tok, c))
        left, tok, k = left - c, tok + 2, k + 1
    assert tok < V - 1
    return runs + [(V - 1, 3), (V, 2), (V + 7, n - edge - 2)]


def clamped_runs(runs, V=TOKEN_V):
    """[(clamped id, first entry, last entry)] of the sorted list: what the kernel sees as runs"""
    out, i = [], 0
    for tok, c in runs:
        t = min(max(tok, 0), V - 1)
        if out and out[-1][0] == t:
            out[-1] = (t, out[-1][1], i + c - 1)
        else:
            out.append((t, i, i + c - 1))
        i += c
    return out


def chunk_relations(runs, V=TOKEN_V):
    """which relations between run edges and the 64-entry chunks the sorted list contains (the CPU test wants every one)"""
    cr = clamped_runs(runs, V)
    n = cr[-1][2] + 1
    multi = [(t, a, b) for t, a, b in cr if b > a]
    single = {a for t, a, b in cr if a == b}
    raw = [tok for tok, c in runs for _ in range(c)]
    astride = [(t, a, b) for t, a, b in cr if any(a < e <= b and raw[e - 1] != raw[e] for e in range(CH, n, CH))]
    return {
        "ends_at_63": any(b % CH == CH - 1 and b - a + 1 < CH for t, a, b in multi),
        "ends_at_64": any(b % CH == 0 for t, a, b in multi),
        "ends_at_65": any(b % CH == 1 for t, a, b in multi),
        "whole_chunk": any(a % CH == 0 and b - a + 1 == CH and a > 0 and b < n - 1 for t, a, b in cr),
        "run_of_65": any(b - a + 1 == CH + 1 for t, a, b in cr),
        "three_chunks": any(b - a + 1 >= 130 and b // CH - a // CH >= 2 for t, a, b in cr),
        "singles_across_edge": any(e - 1 in single and e in single for e in range(CH, n, CH)),
        "partial_last_chunk": n % CH != 0,
        "low_ids_one_run_astride_edge": any(t == 0 for t, a, b in astride),
        "high_ids_one_run_astride_edge": any(t == V - 1 for t, a, b in astride),
    }


def packed_lengths(B, L):
    """sequence lengths of the packed cases: 1 .. 3 for the first 128 sequences, then everything from 1 to L (both included)"""
    lens = [1 + b % 3 if b < 128 else 1 + (b * 7) % L for b in range(B)]
    lens[128], lens[B - 1] = L, 1
    assert 1 in lens[:128] and max(lens[:128]) <= 3 and L in lens and min(lens) >= 1
    return torch.tensor(lens, dtype=torch.int64)


def token_case(B, L, C, dx_dtype, packed=False, V=TOKEN_V):
    """dense: tokens [B, L]; packed: tokens [M] with ``lens`` / ``seq_off`` / ``posidx`` and ``plan_text`` [B, L] (its argmax per row is len - 1: what
    ops.seq_pack_plan turns into seq_off).  ``ref_table`` / ``ref_pos`` float64; dtable starts zeroed (its contract), dpos from ``dpos0``"""
    g = torch.Generator().manual_seed(B * 1009 + L * 31 + C)
    o = {"B": B, "L": L, "C": C, "V": V}
    if packed:
        lens = packed_lengths(B, L)
        n = int(lens.sum())
        off = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)])
        posidx = torch.cat([torch.arange(int(k)) for k in lens])
        plan_text = torch.zeros(B, L, dtype=torch.int64)
        plan_text[torch.arange(B), lens - 1] = 1
        o.update(lens=lens, seq_off=off.to(torch.int32), posidx=posidx.to(torch.int32), plan_text=plan_text)
    else:
        n = B * L
        posidx = torch.arange(n) % L
    runs = token_runs(n, V)
    keys = torch.tensor([tok for tok, c in runs for _ in range(c)], dtype=torch.int64)
    assert keys.numel() == n and bool((keys.diff() >= 0).all())
    tokens = torch.empty(n, dtype=torch.int64)
    tokens[torch.randperm(n, generator=g)] = keys  # a fixed permutation scatters the sorted list over the batch
    dx = int_operand((n, C), DX_R, g, dtype=dx_dtype)
    dpos0 = acc_init((L, C), g)
    cl = tokens.clamp(0, V - 1)
    guard(DX_R * max(int(torch.bincount(cl).max()), B) + ACC_R, 1.0, "token_embed_bwd")
    ref_table = torch.zeros(V, C, dtype=torch.float64).index_add_(0, cl, dx.double())
    ref_pos = dpos0.double().index_add_(0, posidx.long(), dx.double())
    never = torch.ones(V, dtype=torch.bool)
    never[cl] = False
    assert int(never.sum()) > V // 4 and not ref_table[never].any()  # rows of ids that never occur stay zero
    o.update(runs=runs, n=n, tokens=tokens if packed else tokens.reshape(B, L), dx=dx, dpos0=dpos0, ref_table=ref_table, ref_pos=ref_pos, never=never)
    return o


# ---- 2. image embedding ---------------------------------------------------------------------------------------------------------
ASSEMBLE_BCHUNK = 32  # images per batch chunk of the default form
ASSEMBLE_FULL_CASES = ((3, 4, 64), (32, 49, 128), (33, 49, 192), (70, 196, 64))  # (B, G, C)
# (B, G, K, C, step of the hand-built keep, see hand_keep)
ASSEMBLE_KEEP_CASES = ((33, 49, 25, 64, 25), (70, 49, 12, 128, 5), (5, 196, 49, 192, 30))


def hand_keep(B, G, K, step):
    """a keep that needs no device: image b keeps the K patches behind b * step, cyclically, listed from the b-th of them on (distinct per image,
    not ascending)"""
    b, j = torch.arange(B)[:, None], torch.arange(K)[None, :]
    return ((b * step + (j + b) % K) % G).to(torch.int32)


def keep_coverage(keep, G):
    """(a (chunk, position) is kept by no image of that chunk, every position is kept by some image).  A batch of one chunk cannot have both:
    there the first is wanted (a position whose dpos row must keep its initial contents), with more chunks both"""
    B = keep.shape[0]
    kept = torch.zeros(B, G, dtype=torch.bool)
    kept[torch.arange(B)[:, None], keep.long()] = True
    chunks = [kept[b:b + ASSEMBLE_BCHUNK].any(0) for b in range(0, B, ASSEMBLE_BCHUNK)]
    return any(not bool(c.all()) for c in chunks), bool(kept.any(0).all())


def keep_is_good(keep, G):
    B = keep.shape[0]
    ok = bool(((keep >= 0) & (keep < G)).all()) and all(len(set(row)) == len(row) for row in keep.tolist())
    hole, all_kept = keep_coverage(keep, G)
    return ok and hole and (all_kept or B <= ASSEMBLE_BCHUNK)


def assemble_case(B, G, C, keep=None):
    """demb [B * (K + 1), C] integers in [-8, 8]; float64 references of dpos / dcls (initial contents included) and the bf16 dpatch (exact)"""
    K = G if keep is None else keep.shape[1]
    g = torch.Generator().manual_seed(B * 131 + G * 17 + K * 3 + C)
    demb = int_operand((B * (K + 1), C), DX_R, g, dtype=torch.float32)
    dpos0, dcls0 = acc_init((G + 1, C), g), acc_init((C,), g)
    if keep is not None:
        assert keep_is_good(keep, G), "this keep leaves no (chunk, position) unkept, or a position unkept in a batch of several chunks"
    guard(DX_R * B + ACC_R, 1.0, "embed_assemble_bwd")
    d3 = demb.reshape(B, K + 1, C).double()
    pos_of = (torch.arange(G).expand(B, G) if keep is None else keep.long()) + 1  # [B, K]: the dpos row of token 1 + j of image b
    ref_pos = dpos0.double()
    ref_pos[0] += d3[:, 0].sum(0)
    ref_pos.index_add_(0, pos_of.reshape(-1), d3[:, 1:].reshape(B * K, C))
    ref_cls = dcls0.double() + d3[:, 0].sum(0)
    dpatch = demb.reshape(B, K + 1, C)[:, 1:].reshape(B * K, C).to(torch.bfloat16)
    assert torch.equal(dpatch.float(), demb.reshape(B, K + 1, C)[:, 1:].reshape(B * K, C))
    return {"B": B, "G": G, "K": K, "C": C, "demb": demb, "dpos0": dpos0, "dcls0": dcls0, "ref_pos": ref_pos, "ref_cls": ref_cls, "ref_patch": dpatch}


# ---- 3. column sums -------------------------------------------------------------------------------------------------------------
COLSUM_R = (1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1031)  # across the 1 / 8 / 32 row slices and the four row groups of a workgroup
COLSUM_C = (1, 3, 63, 64, 65, 200)  # across the 64 columns of a workgroup; 3 = the [R, 3] rows of the reproducible losses
COLSUM_X_R = 64


def colsum_case(R, C):
    g = torch.Generator().manual_seed(R * 211 + C)
    x = int_operand((R, C), COLSUM_X_R, g, dtype=torch.float32)
    out0 = acc_init((C,), g)
    guard(x.abs().sum(0) + ACC_R, 1.0, "colsum_f32")
    return {"x": x, "out0": out0, "ref": out0.double() + x.double().sum(0)}


def colsum_single_add_case():
    """the fixed-order form promises ONE addition into ``out`` per column (one row slice, four partial sums folded before the atomic).  out = 2^24 on
    entry, ones in rows 0 and 4 (different row slices whenever there are several): one addition gives 2^24 + 2 exactly; two additions of 1, in
    either order, are each a tie that rounds back to the even 2^24.  Not an any-order case -- only the fixed-order form is held to it."""
    R, C = 65, 65
    x = torch.zeros(R, C)
    x[0], x[4] = 1.0, 1.0
    out0 = torch.full((C,), float(LIMIT))
    assert float(out0[0] + 1.0) == LIMIT and float(out0[0] + 2.0) == LIMIT + 2  # the tie and the exact sum, in fp32
    return {"x": x, "out0": out0, "ref": out0.double() + 2.0}


# ---- 4. LayerNorm backward ------------------------------------------------------------------------------------------------------
LN_POW2_C = (64, 256, 512, 1024, 2048)
LN_OTHER_C = (192, 768, 1280, 1536)
LN_M = (1, 7, 16, 17)
LN_WAVES_MAX = 16  # the largest wave count per workgroup in the kernels' tables


def ln_ranges(C):
    """(range of x - mean, range of dres): narrowed with C until the dx guard (units of 1 / 8C) holds"""
    return (2, 4) if C >= 2048 else ((4, 8) if C >= 1024 else (8, 16))


def ln_big_m(cus):
    """every wave of the capped grid (one workgroup per CU) reaches a third row: more than two strides of cus * 16 rows"""
    return 2 * cus * LN_WAVES_MAX + 37


def ln_case(M, C, seed=0, dcol=True):
    """mean in [-2, 2], rstd in {0.5, 1, 2}, x = mean + integers, dy integers in [-3, 3], w in {-2, -1, 1, 2}, dres integers: xhat is a multiple of
    0.5, dw and db are exact in any order for every C, dx / dcol are for a power-of-two C (1 / C exact; every term a multiple of 1 / 8C).  All
    tensors fp32 and exactly representable in bf16.  References float64.  ``dcol`` False: a case that asks for no column sums of dx (the large M)"""
    pow2 = C & (C - 1) == 0
    rx, rres = ln_ranges(C)
    g = torch.Generator().manual_seed(M * 7919 + C + seed)
    mean = int_operand((M,), 2, g, dtype=torch.float32)
    rstd = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (M,), generator=g)]
    x = int_operand((M, C), rx, g, dtype=torch.float32) + mean[:, None]
    dy = int_operand((M, C), 3, g, dtype=torch.float32)
    w = torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, (C,), generator=g)]
    dres = int_operand((M, C), rres, g, dtype=torch.float32)
    dw0, db0, dcol0 = acc_init((C,), g), acc_init((C,), g), acc_init((C,), g)
    for t in (x, dy, dres):
        assert torch.equal(t.to(torch.bfloat16).float(), t)
    xh = (x.double() - mean.double()[:, None]) * rstd.double()[:, None]
    gg = dy.double() * w.double()
    guard((dy.double() * xh).abs().sum(0) + ACC_R, 0.5, "layernorm_bwd dw")
    guard(dy.double().abs().sum(0) + ACC_R, 1.0, "layernorm_bwd db")
    o = {"M": M, "C": C, "pow2": pow2, "mean": mean, "rstd": rstd, "x": x, "dy": dy, "w": w, "dres": dres, "dw0": dw0, "db0": db0, "dcol0": dcol0,
         "ref_dw": dw0.double() + (dy.double() * xh).sum(0), "ref_db": db0.double() + dy.double().sum(0)}
    s1, s2 = gg.sum(1, keepdim=True), (gg * xh).sum(1, keepdim=True)
    c1, c2 = s1 / C, s2 / C
    core = rstd.double()[:, None] * (gg - c1 - xh * c2)
    o["ref_dx"] = {False: core, True: core + dres.double()}
    o["ref_dcol"] = {k: dcol0.double() + v.sum(0) for k, v in o["ref_dx"].items()}
    if pow2:
        guard(gg.abs().sum(1), 1.0, "layernorm_bwd c1")  # the row sums, in any order
        guard((gg * xh).abs().sum(1), 0.5, "layernorm_bwd c2")
        guard(2 * xh.abs().max() * 2 * s2.abs().max(), 1.0, "layernorm_bwd xhat * c2")  # integer x integer: the product's significand
        guard((gg - c1).abs(), 1.0 / C, "layernorm_bwd g - c1")
        guard((gg - c1 - xh * c2).abs(), 0.25 / C, "layernorm_bwd g - c1 - xhat c2")
        guard(core.abs(), 0.125 / C, "layernorm_bwd dx")
        guard((core + dres.double()).abs(), 0.125 / C, "layernorm_bwd dx + dres")
        for v in o["ref_dx"].values() if dcol else ():
            guard(v.abs().sum(0) + ACC_R, 0.125 / C, "layernorm_bwd dcol")
    return o


def ln_formula_f32(o, with_dres, order):
    """the same formula in fp32 with torch, the row and column sums taken in two different orders (0: torch's own; 1: columns reversed, four strided
    partial sums per row folded last to first, rows summed back to front).  (dx, dw, db, dcol) fp32"""
    x, dy, w, mean, rstd = o["x"], o["dy"], o["w"], o["mean"], o["rstd"]
    C, M = o["C"], o["M"]
    xh = (x - mean[:, None]) * rstd[:, None]
    gg = dy * w

    def rowsum(t):
        if order == 0:
            return t.sum(1, keepdim=True)
        p = t.flip(1).reshape(M, C // 4, 4).sum(1)  # four strided partial sums
        return (((p[:, 3] + p[:, 2]) + p[:, 1]) + p[:, 0])[:, None]

    def colsum(t):
        if order == 0:
            return t.sum(0)
        acc = torch.zeros(C)
        for r in range(M - 1, -1, -1):
            acc = acc + t[r]
        return acc

    c1, c2 = rowsum(gg) * (1.0 / C), rowsum(gg * xh) * (1.0 / C)
    dx = rstd[:, None] * (gg - c1 - xh * c2)
    if with_dres:
        dx = dx + o["dres"]
    return dx, o["dw0"] + colsum(dy * xh), o["db0"] + colsum(dy), o["dcol0"] + colsum(dx)


# ---- 5. squared gradient norm ---------------------------------------------------------------------------------------------------
SUMSQ_N = (1, 255, 256, 257, 100003)
SUMSQ_R = 8
CLIP_SHAPES = ((128, 192), (64, 64), (768,), (), (50, 768), (100003,), (192, 3, 8, 8), (24577,))  # tests/test_kernels_gpu.py's fused-clip test
CLIP_OFFSET_VIEWS = (0, 5)  # the gradients held as views at a 4-byte offset
CLIP_R = 2


def sumsq_case(n):
    g = torch.Generator().manual_seed(n)
    x = int_operand((n,), SUMSQ_R, g, dtype=torch.float32)
    out0 = 7.0
    guard(float((x.double() ** 2).sum()) + out0, 1.0, "sumsq_accum")
    return {"x": x, "out0": out0, "ref": torch.tensor([out0], dtype=torch.float64) + (x.double() ** 2).sum()}


def clip_case(step=0):
    g = torch.Generator().manual_seed(77 + step)
    grads = [int_operand(sh, CLIP_R, g, dtype=torch.float32) for sh in CLIP_SHAPES]
    total = sum(float((t.double() ** 2).sum()) for t in grads)
    guard(total, 1.0, "grad norm")
    return {"grads": grads, "ref": torch.tensor([total], dtype=torch.float64)}


# ---- 6. loss rows (not exact arithmetic: bounds per row) ------------------------------------------------------------------------
LOSS_SHAPES = ((6, 6, 0), (64, 200, 64), (300, 300, 0), (5, 1000, 995))  # (R, N, label offset); the last: four 256-thread passes, labels in the last, partial one
LOSS_SCALE_S = 14.3
SIGLIP_BIAS = -3.0
LOSS_REL, LOSS_ABS, DSUM_REL = 1e-5, 1e-7, 1e-4  # the bounds of test_loss_row_kernels, per row
# d/d logit_scale of a PEAKED cross-entropy row: fp32 cannot hold softmax(label) - 1 there (the row's exp sum is 1 + 1e-13 = 1), so the plain fp32
# torch statement of the row misses float64 by up to 0.961 of the row's sum of |term| (0.9601 / 0.8738 / 0.8600 / 0.8236 at the four shapes, measured by
# tests/test_reduce_exact.py; the sums themselves are ~1e-12 of a Gaussian row's) -- 9.6e3 times the 1e-4 bound.  The bound of that one quantity
# is four times the fp32 statement's own error, as a share of the row's sum of |term|:
CE_PEAKED_DSCALE_FP32 = 0.961
CE_PEAKED_DSCALE_BOUND = 4 * CE_PEAKED_DSCALE_FP32


def loss_logits(R, N, off, peaked):
    g = torch.Generator().manual_seed(R + N)
    logits = torch.randn(R, N, generator=g) * 4
    if peaked:  # the trained regime: the label's logit 30 above everything else in its row
        rows = torch.arange(R)
        logits[rows, rows + off] = -float("inf")
        logits[rows, rows + off] = logits.max(1).values + 30.0
    return logits


def _ce_rows(logits, off, loss_scale, grad_scale, inv_s):
    """(rows [R, 3], sum of |term| of dscale per row) of the cross-entropy rows, in the dtype of ``logits``"""
    R = logits.shape[0]
    rows, lab = torch.arange(R), torch.arange(R) + off
    lse = torch.logsumexp(logits, 1)
    p = torch.softmax(logits, 1)
    p[rows, lab] -= 1.0
    term = p * grad_scale * logits * inv_s
    out = torch.stack([(lse - logits[rows, lab]) * loss_scale, term.sum(1), torch.zeros_like(lse)], 1)
    return out, term.abs().sum(1)


def _siglip_rows(logits, off, neg, bias, loss_scale, grad_scale, inv_s):
    R, N = logits.shape
    lab = -torch.ones_like(logits)
    onehot = torch.zeros_like(logits)
    if not neg:
        lab[torch.arange(R), torch.arange(R) + off] = 1.0
        onehot[torch.arange(R), torch.arange(R) + off] = 1.0
    ls = -torch.nn.functional.logsigmoid(lab * logits)
    gr = (torch.sigmoid(logits) - onehot) * grad_scale
    ds = gr * (logits - bias) * inv_s
    return torch.stack([ls.sum(1) * loss_scale, ds.sum(1), gr.sum(1)], 1), ds.abs().sum(1), gr.abs().sum(1)


def loss_rows_reference(logits32, off, kind, dtype=torch.float64, peaked_bound=False):
    """per-row references on the SAME fp32 logits, evaluated in ``dtype`` (float64: the reference; float32: the plain fp32 statement, whose own error
    is the yardstick where a bound proves too tight).  kind 'ce' | 'siglip' | 'siglip_neg'; ``peaked_bound``: CE_PEAKED_DSCALE_BOUND for the
    cross-entropy's dscale.  Returns (rows [R, 3], bounds [R, 3], scales)"""
    R = logits32.shape[0]
    lg = logits32.to(dtype)
    if kind == "ce":
        sc = (0.5 / R, 0.5 / R, 1.0 / LOSS_SCALE_S)
        rows, a1 = _ce_rows(lg, off, *sc)
        a2 = torch.zeros_like(a1)
    else:
        sc = (1.0 / R, 1.0 / R, 1.0 / LOSS_SCALE_S)
        rows, a1, a2 = _siglip_rows(lg, off, kind == "siglip_neg", SIGLIP_BIAS, *sc)
    rel1 = CE_PEAKED_DSCALE_BOUND if (kind == "ce" and peaked_bound) else DSUM_REL
    bounds = torch.stack([LOSS_REL * rows[:, 0].abs() + LOSS_ABS * sc[0], rel1 * a1, DSUM_REL * a2], 1)
    return rows, bounds, sc


def worst_ratio(got, ref, bounds):
    """per column of the rows: max over rows of |got - ref| / bound (a zero bound with a zero error counts as 0)"""
    err = (got.double() - ref.double()).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bounds.double().clamp_min(1e-300))
    return [float(ratio[:, k].max()) for k in range(ratio.shape[1])]

