"""Exact-arithmetic attention checks (helper module of tests/test_attn_exact.py and tests/test_attn_exact_gpu.py).

Inputs for which softmax is exactly one-hot ("selection") or exactly uniform over 2^k keys ("uniform"), small integers everywhere else: every result of
the attention kernels is then a known dyadic rational, and a wrong, missing or extra key moves an output by a whole grid step, not by 1e-3.

Construction (per sequence and head, its own seeded sets; scale = 0.125 for every head dim):
  * key j carries the code (j mod 32, j div 32): K[j] = 32 e_a + 32 e_{32+b} on the first 48 of the head's dims (16 high dims: up to 512 keys);
  * query i carries -32 on every code dim outside its sets A_i (low part) and B_i (high part), 0 inside: a key with a in A_i and b in B_i scores 0,
    every other key -1024 * scale or -2048 * scale = -184 or less in log2 units, where fp32 exp2 underflows to exactly 0 -- also across the rescale of
    the online softmax.  The winning score is 0, not a large number: ulp(score) never enters P;
  * the SELECTED keys of a query are the members of A_i x B_i that it may see; the members it may NOT see (future keys under the causal mask, key
    i + 1 in particular) are decoys: they score 0 as well, so a mask that leaks one changes the count.  Rows behind a pooled query in dense causal
    text copy the code of a selected key.  The last key of every sequence is selected by several queries: the kernels fill the tail of the last
    32-row block with copies of it, and a padded key that gets weight changes the count of exactly those queries;
  * sequence boundaries: every query of sequence b carries +64 on dim 48 + b % 3, every key of sequence b + 1 carries +64 on that same dim (inside a
    sequence the two dims differ: no contribution).  A kernel that runs past the end of a sequence meets keys that score +2048 * scale or more and
    take the whole row; behind the last sequence, and in front of the first, the allocation holds NaN;
  * V: integers in [-2, 2], rows pairwise distinct over the whole case; dO: two entries of +-1 in the rows that carry a gradient (uniform family: at
    most two such queries per key, so dK / dV stay within bf16's 8 bits); dims of Q and K behind the code are 0, V and dO use all D dims.  With head
    dim 88 / 104 the columns that the zero-padded contraction has to ignore are the neighbouring head's first code dims (entries -32 / +32).

The float64 reference (``head_reference``) is plain softmax attention with the kernels' rounding points -- P -> bf16, dS -> bf16, every output -> bf16,
exp2 of -150 or less -> 0 -- and asserts that every one of them is lossless; tests/test_attn_exact.py compares it with float64 autograd.  What survives
in a kernel is fp32 noise where the true dS is 0 (P is 2^-k up to a relative ``P_REL``): the guard bounds it below g / 16 for the stated grid step g."""
import math
import random

import torch

SCALE = 0.125
LOG2E = 1.4426950408889634
MASKED_MAX = -150.0 / LOG2E  # a scaled score at or below it has P = 0 exactly in fp32
LO, CODE_DIMS, SPARE = 32, 48, 48  # dims 0..31: j mod 32; 32..47: j div 32; 48..50: the sequence-boundary decoys
ENTRY, SPARE_ENTRY, V_R = 32, 64, 2
G_OUT = G_DV = 2.0 ** -3  # means of up to 8 integers; 2^-3 * dO
G_DQ = G_DK = 2.0 ** -4   # 32 * dS, dS = 2^-k (dP - delta) * scale a multiple of 2^-9 at k = 3
# P = exp2(0 - lse * log2(e)) with lse = fp32(k * ln 2): two roundings of k (<= 3 * 2^-24 relative, times k ln 2 <= 2.08 in the exponent) and the
# hardware exp2 (2^-22): below 2^-20 relative
P_REL = 2.0 ** -20
EPS32 = 2.0 ** -23
PAD_ROWS = 8
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def report(line):
    """one line into the parity report of tests/test_kernels_gpu.py (same file, same format)"""
    from tests.test_kernels_gpu import _report
    _report(line)


# ---- case tables (data; tests/test_attn_exact.py validates every entry on the CPU) -------------------------------------------------------------
def _self(L, causal, family, D=64, B=2, H=2, knobs=(), lens=None, branch=""):
    return {"kind": "self", "L": L, "causal": causal, "family": family, "D": D, "B": B if lens is None else len(lens), "H": H, "knobs": tuple(knobs),
            "lens": lens, "branch": branch}


def case_id(c):
    s = f"{c['kind']}-{c.get('mode') or 'L%d' % c['L']}-hd{c['D']}-B{c['B']}H{c['H']}-{'causal' if c['causal'] else 'full'}-{c['family']}"
    if c.get("lens"):
        s += "-packed" + ("-bucketed" if c.get("bucketed") else "")
    return s + "".join(f"-knob{k}={v}" for k, v in c.get("knobs", ()))


FAMILIES = ("selection", "uniform")
RESIDENT_L = (1, 31, 32, 33, 50, 64, 65, 77, 96, 97, 128)
# head-resident kernels, head dim 64, dense: backward with delta from P and dP (<= 2 blocks), attn_bwd_causal_kernel (2-3 blocks, causal), two-pass form
RESIDENT_CASES = [_self(L, causal, fam, B=2 + L % 2, H=2 + (L // 32) % 2, branch="head-resident")
                  for L in RESIDENT_L for causal in (False, True) for fam in FAMILIES]
KNOB_CASES = [_self(50, False, "uniform", H=3, knobs=((2, 6),), branch="O-reading backward on a 2-block shape"),
              _self(50, False, "uniform", B=3, knobs=((7, 1),), branch="streamed kernels forced"), _self(50, False, "selection", knobs=((7, 1),)),
              _self(77, True, "uniform", H=3, knobs=((7, 1),), branch="streamed kernels forced"), _self(77, True, "selection", knobs=((7, 1),))]
MIXED_CASES = [_self(L, causal, fam, branch="streamed forward" + (", resident 640-thread backward" if L <= 320 else " and backward"))
               for L in (129, 257, 320, 321) for causal in (False, True) for fam in FAMILIES]
STREAMED_D = (80, 88, 96, 104, 112, 128)
STREAMED_L = (63, 64, 65, 129, 257)
STREAMED_CASES = [_self(L, L in (65, 257), fam, D=D, B=2 + (D // 8) % 2, branch="streamed, zero-padded contraction" if D in (88, 104) else "streamed")
                  for D in STREAMED_D for L in STREAMED_L for fam in FAMILIES]
PACKED_LENS = (77, 1, 32, 33, 64, 9)  # in this order: the buckets (1, 2 and 3 blocks) interleave
PACKED_CASES = [dict(_self(77, True, fam, H=2, lens=PACKED_LENS, branch="packed"), bucketed=bk) for fam in FAMILIES for bk in (True, False)]
SELF_CASES = RESIDENT_CASES + KNOB_CASES + MIXED_CASES + STREAMED_CASES


def _pooled(mode, family):
    L, causal, lens, qpos = {"image_cls": (50, False, None, (0, 0, 0)), "long": (257, False, None, (0, 0, 0)),
                             "text_packed": (77, True, (77, 1, 33), (76, 0, 32)), "text_dense": (77, True, None, (40, 0, 63))}[mode]
    return {"kind": "pooled", "mode": mode, "L": L, "causal": causal, "family": family, "D": 64, "B": 3, "H": 2, "lens": lens, "qpos": qpos}


POOLED_CASES = [_pooled(m, f) for m in ("image_cls", "long", "text_packed", "text_dense") for f in FAMILIES]


def case_seed(c):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(case_id(dict(c, bucketed=False, knobs=()))))  # the same rows with and without knobs / buckets


# ---- construction -----------------------------------------------------------------------------------------------------------------------------
_SHAPES = {1: ((1, 1),), 2: ((2, 1), (1, 2)), 4: ((4, 1), (2, 2)), 8: ((8, 1), (4, 2))}  # (|A|, |B|) of a count


def _visible(A, B, vis_max):
    return sorted(32 * b + a for b in B for a in A if 32 * b + a <= vis_max)


def choose_sets(rng, vis_max, family, decoy=None, include=None, seam=None):
    """(A, B, S): low and high code sets of one query and the keys 0..vis_max they select.  ``decoy``: a key behind vis_max whose code has to lie in
    A x B; ``include``: a key that has to be selected; ``seam`` = m: keys 32 m - 1 and 32 m have to be selected (a block seam inside the set; a
    64-row chunk seam for even m).  Rejection sampling: |S| must be 1 (selection) or 2, 4, 8 (uniform)."""
    if seam is not None:
        include = 32 * seam
    want = (1,) if family == "selection" or vis_max == 0 else (2, 4, 8)
    vblk = vis_max // 32
    for attempt in range(900):
        if attempt == 300:
            decoy = None
        if attempt == 600:
            want = (1, 2, 4, 8)  # e.g. two visible keys in different blocks and columns: no product set of two
        ka, kb = rng.choice(_SHAPES[rng.choice(want)])
        j0 = include if include is not None else rng.randrange(vis_max + 1)
        a0, b0 = j0 % 32, j0 // 32
        B = {b0}
        if kb == 2:
            if vblk == 0:
                continue
            adjacent = [b for b in (b0 - 1, b0 + 1) if 0 <= b <= vblk]
            B.add(rng.choice(adjacent) if rng.random() < 0.6 else rng.choice([b for b in range(vblk + 1) if b != b0]))
        if rng.random() < 0.6:  # a run of consecutive columns (mod 32): a run through 31 -> 0 over two adjacent blocks has a block seam inside
            start = a0 - rng.randrange(ka)
            A = {(start + t) % 32 for t in range(ka)}
        else:
            A = {a0} | set(rng.sample([a for a in range(32) if a != a0], ka - 1))
        if seam is not None:
            A.add(31)
            B.add(seam - 1)
        if decoy is not None:
            A.add(decoy % 32)
            B.add(decoy // 32)
        S = _visible(A, B, vis_max)
        if len(S) in want and (include is None or include in S) and (seam is None or 32 * seam - 1 in S):
            return A, B, S
    raise AssertionError(f"no sets for vis_max={vis_max} family={family} include={include}")


def seams_to_straddle(n, causal):
    """the block seams m (keys 32 m - 1 | 32 m) that some set of a sequence of n keys has to hold.  All of them, except the last one of a sequence
    of 32 m + 31 keys without the causal mask: column 31 then exists in one block less than every other column, and every product set that holds
    the seam has an odd number of keys"""
    return [m for m in range(1, (n - 1) // 32 + 1) if causal or not (n % 32 == 31 and m == (n - 1) // 32)]


def _query_row(D, A, B):
    q = torch.zeros(D, dtype=F64)
    q[:CODE_DIMS] = -ENTRY
    q[sorted(A)] = 0.0
    q[[LO + b for b in sorted(B)]] = 0.0
    return q


def _key_row(D, j):
    k = torch.zeros(D, dtype=F64)
    k[j % 32] = ENTRY
    k[LO + j // 32] = ENTRY
    return k


def _dout_row(rng, D):
    r = torch.zeros(D, dtype=F64)
    for d in rng.sample(range(D), 2):
        r[d] = rng.choice((-1.0, 1.0))
    return r


def _offsets(lens):
    off = [0]
    for n in lens:
        off.append(off[-1] + n)
    return off


def _values(g, M, C):
    return torch.randint(-V_R, V_R + 1, (M, C), generator=g).to(F64)


def build_self(c):
    """the inputs of one self-attention case, float64 holding small integers: qkv [M, 3C], dout [M, C]; ``sets[(b, h)]`` = selected keys per query"""
    B, H, D, L = c["B"], c["H"], c["D"], c["L"]
    assert L <= 16 * 32 and D >= CODE_DIMS + 3 and D % 8 == 0
    lens = list(c["lens"] or [L] * B)
    rng, g = random.Random(case_seed(c)), torch.Generator().manual_seed(case_seed(c))
    C, off = H * D, _offsets(lens)
    M = off[-1]
    qkv, dout, sets = torch.zeros(M, 3 * C, dtype=F64), torch.zeros(M, C, dtype=F64), {}
    qkv[:, 2 * C:] = _values(g, M, C)
    for b in range(B):
        n, r0 = lens[b], off[b]
        for h in range(H):
            col = h * D
            last = {n - 1} if c["causal"] else {n - 1} | {rng.randrange(n) for _ in range(3)}  # queries that select the sequence's last key
            seam_of = {}  # uniform family: two queries per block seam whose sets hold the keys on both sides of it
            for m in seams_to_straddle(n, c["causal"]) if c["family"] == "uniform" else ():
                cand = (32 * m + 3, 32 * m + 40, 32 * m, n - 1) if c["causal"] else rng.sample(range(n), min(n, 6))
                for i in [i for i in cand if 32 * m <= i < n or not c["causal"]]:
                    if (i not in last or 32 * m == n - 1) and i not in seam_of and sum(1 for v in seam_of.values() if v == m) < 2:
                        seam_of[i] = m
            sel = []
            for i in range(n):
                vis_max = i if c["causal"] else n - 1
                decoy = i + 1 if c["causal"] and i + 1 < n and ((i + 1) % 32 == 0 or rng.random() < 0.5) else None
                A, Bs, S = choose_sets(rng, vis_max, c["family"], decoy, n - 1 if i in last else None, seam_of.get(i))
                qkv[r0 + i, col:col + D] = _query_row(D, A, Bs)
                qkv[r0 + i, C + col:C + col + D] = _key_row(D, i)
                sel.append(S)
            qkv[r0:r0 + n, col + SPARE + b % 3] = SPARE_ENTRY
            if b > 0:
                qkv[r0:r0 + n, C + col + SPARE + (b - 1) % 3] = SPARE_ENTRY
            uses = [0] * n  # uniform family: a key receives dS from at most two queries
            order = [n - 1, 0] + rng.sample(range(n), n)
            done = set()
            for i in order:
                if i in done or (c["family"] == "uniform" and any(uses[j] >= 2 for j in sel[i])):
                    continue
                done.add(i)
                for j in sel[i]:
                    uses[j] += 1
                dout[r0 + i, col:col + D] = _dout_row(rng, D)
            sets[(b, h)] = sel
    return {"case": c, "qkv": qkv, "dout": dout, "lens": lens, "off": off, "sets": sets, "M": M, "C": C}


def dense_twin(inp):
    """the dense batch that holds the rows of a packed causal case: sequence b's rows at b * L .., behind them filler tokens (each query selects its own
    key; no gradient), which the causal mask keeps away from the rows in front of them"""
    c = inp["case"]
    B, H, D, L, C = c["B"], c["H"], c["D"], c["L"], inp["C"]
    assert c["causal"] and c["lens"]
    g = torch.Generator().manual_seed(case_seed(c) + 1)
    qkv, dout = torch.zeros(B * L, 3 * C, dtype=F64), torch.zeros(B * L, C, dtype=F64)
    qkv[:, 2 * C:] = _values(g, B * L, C) + 2 * V_R + 1  # filler values in [3, 7]: distinct from every packed row
    for b in range(B):
        n, r0 = inp["lens"][b], inp["off"][b]
        for h in range(H):
            col = h * D
            for i in range(n, L):
                qkv[b * L + i, col:col + D] = _query_row(D, {i % 32}, {i // 32})
                qkv[b * L + i, C + col:C + col + D] = _key_row(D, i)
            qkv[b * L + n:(b + 1) * L, col + SPARE + b % 3] = SPARE_ENTRY
            if b > 0:
                qkv[b * L + n:(b + 1) * L, C + col + SPARE + (b - 1) % 3] = SPARE_ENTRY
        qkv[b * L:b * L + n] = inp["qkv"][r0:r0 + n]
        dout[b * L:b * L + n] = inp["dout"][r0:r0 + n]
    tc = dict(c, lens=None, bucketed=False)
    return {"case": tc, "qkv": qkv, "dout": dout, "lens": [L] * B, "off": _offsets([L] * B), "sets": None, "M": B * L, "C": C}


def build_pooled(c):
    """single-query case: q [B, C], kv [M, 2C] (K | V), dout [B, C], rows [B] (absolute row of the pooled token)"""
    B, H, D, L = c["B"], c["H"], c["D"], c["L"]
    lens = list(c["lens"] or [L] * B)
    rng, g = random.Random(case_seed(c)), torch.Generator().manual_seed(case_seed(c))
    C, off = H * D, _offsets(lens)
    M = off[-1]
    q, kv, dout = torch.zeros(B, C, dtype=F64), torch.zeros(M, 2 * C, dtype=F64), torch.zeros(B, C, dtype=F64)
    kv[:, C:] = _values(g, M, C)
    sets = {}
    for b in range(B):
        n, r0, qp = lens[b], off[b], c["qpos"][b]
        for h in range(H):
            col = h * D
            vis_max = qp if c["causal"] else n - 1
            A, Bs, S = choose_sets(rng, vis_max, c["family"], None, vis_max if h == 0 else None)
            q[b, col:col + D] = _query_row(D, A, Bs)
            q[b, col + SPARE + b % 3] = SPARE_ENTRY
            for j in range(n):  # rows behind the pooled token: decoys, copies of a selected key's code
                kv[r0 + j, col:col + D] = _key_row(D, j if j <= vis_max else S[j % len(S)])
            if b > 0:
                kv[r0:r0 + n, col + SPARE + (b - 1) % 3] = SPARE_ENTRY
            dout[b, col:col + D] = _dout_row(rng, D)
            sets[(b, h)] = [S]
    rows = torch.tensor([off[b] + c["qpos"][b] for b in range(B)], dtype=torch.int32)
    return {"case": c, "q": q, "kv": kv, "dout": dout, "rows": rows, "lens": lens, "off": off, "sets": sets, "M": M, "C": C}


# ---- float64 reference with the kernels' rounding points ---------------------------------------------------------------------------------------
def _rb(x, strict, what):
    """x through bf16; strict: the rounding must be lossless"""
    r = x.to(F32).to(BF16).to(F64)
    if strict:
        assert torch.equal(r, x), f"{what}: not representable in bf16 (max |loss| {float((r - x).abs().max()):.3e}): badly chosen case"
    return r


def _on_grid(x, g, what):
    assert g > 0 and math.log2(g) == round(math.log2(g))
    assert torch.equal((x / g).round() * g, x), f"{what}: not a multiple of the stated grid step {g}"
    assert float(x.abs().max()) / g < 2 ** 24  # (partial sums of such values are exact in fp32 in any order)


def head_reference(q, k, v, do, vis, scale=SCALE, strict=True):
    """one (sequence, head): q [nq, D], k, v [nk, D], do [nq, D] float64, vis [nq, nk] bool.  -> out, lse, dq, dk, dv, count and the analytic bound of
    the fp32 noise in dq / dk.  ``strict`` runs the guards (a badly chosen case fails here, on its own inputs); without it the same arithmetic serves
    the deliberately wrong references of tests/test_attn_exact.py."""
    s = (q @ k.t()) * scale
    m = torch.where(vis, s, torch.full_like(s, -math.inf)).max(-1).values
    assert torch.isfinite(m).all(), "a query that sees no key"
    live = vis & ((s - m[:, None]) * LOG2E > -150.0)  # fp32 exp2 of -150 or less is 0
    e = torch.where(live, torch.exp(s - m[:, None]), torch.zeros_like(s))
    count = live.sum(-1)
    if strict:
        assert torch.equal(m, torch.zeros_like(m)), "the winning score must be 0"
        assert torch.equal(live, vis & (s == 0)), "a visible key that neither scores 0 nor <= -150 / log2(e)"
        assert bool((s[vis & ~live] <= MASKED_MAX).all())
        assert bool(((count & (count - 1)) == 0).all()) and int(count.min()) >= 1, f"counts {sorted(set(count.tolist()))}: not powers of two"
    l = e.sum(-1)
    p = e / l[:, None]
    out = _rb((_rb(e, strict, "P") @ v) / l[:, None], strict, "out")
    dp = do @ v.t()
    delta = (do * out).sum(-1)
    ds = _rb(p * (dp - delta[:, None]) * scale, strict, "dS")
    dv = _rb(_rb(p, strict, "P / l").t() @ do, strict, "dV")
    dq = _rb(ds @ k, strict, "dQ")
    dk = _rb(ds.t() @ q, strict, "dK")
    w = p * (dp.abs() + delta.abs()[:, None]) * scale  # |dS| where the true value is 0 is at most P_REL * w
    noise = P_REL * max(float((w @ k.abs()).max()), float((w.t() @ q.abs()).max()))
    return {"out": out, "lse": m + torch.log(l), "dq": dq, "dk": dk, "dv": dv, "count": count, "noise": noise, "dp_max": float(dp.abs().max()),
            "entry_max": float(max(q.abs().max(), k.abs().max()))}


def _vis_self(n, causal, shift=0):
    i = torch.arange(n)
    return (i[None, :] <= i[:, None] + shift) if causal else torch.ones(n, n, dtype=torch.bool)


def _guard_noise(name, parts, L):
    """both bounds below g / 16: the one worked out per element (head_reference) and eps * max|dP| * scale * max entry * L"""
    noise = max(p["noise"] for p in parts)
    coarse = EPS32 * max(p["dp_max"] for p in parts) * SCALE * max(p["entry_max"] for p in parts) * L
    assert max(noise, coarse) < min(G_DQ, G_DK) / 16, f"{name}: fp32 noise bound {noise:.3e} / {coarse:.3e} not below g / 16"
    return max(noise, coarse)


def reference_self(inp, strict=True, causal_shift=0, dup_last_key=False):
    """-> {"out" [M, C], "dqkv" [M, 3C], "lse" [B, H, L] (NaN where a packed sequence has no row), "count", "noise"} in float64.  ``causal_shift`` and
    ``dup_last_key`` (the last key of every sequence counted once more, as a padded key that got weight would be) build WRONG references."""
    c = inp["case"]
    B, H, D, L, C = c["B"], c["H"], c["D"], c["L"], inp["C"]
    qkv, dout = inp["qkv"], inp["dout"]
    out, dqkv = torch.zeros(inp["M"], C, dtype=F64), torch.zeros(inp["M"], 3 * C, dtype=F64)
    lse, count, parts = torch.full((B, H, L), math.nan, dtype=F64), torch.zeros(B, H, L, dtype=torch.int64), []
    if strict:
        assert torch.unique(qkv[:, 2 * C:].reshape(-1, D), dim=0).shape[0] == inp["M"] * H, "V rows are not pairwise distinct"
    for b in range(B):
        n, r0 = inp["lens"][b], inp["off"][b]
        for h in range(H):
            col = h * D
            q, k, v = (qkv[r0:r0 + n, t * C + col:t * C + col + D] for t in range(3))
            vis = _vis_self(n, c["causal"], causal_shift)
            if dup_last_key:
                k, v, vis = torch.cat([k, k[-1:]]), torch.cat([v, v[-1:]]), torch.cat([vis, vis[:, -1:]], 1)
            r = head_reference(q, k, v, dout[r0:r0 + n, col:col + D], vis, strict=strict)
            if dup_last_key:
                for nm in ("dk", "dv"):
                    r[nm] = torch.cat([r[nm][:n - 1], r[nm][n - 1:n] + r[nm][n:]])
            out[r0:r0 + n, col:col + D] = r["out"]
            for t, nm in enumerate(("dq", "dk", "dv")):
                dqkv[r0:r0 + n, t * C + col:t * C + col + D] = r[nm]
            lse[b, h, :n], count[b, h, :n] = r["lse"], r["count"]
            parts.append(r)
    ref = {"out": out, "dqkv": dqkv, "lse": lse, "count": count, "noise": 0.0}
    if strict:
        _on_grid(out, G_OUT, "out"), _on_grid(dqkv[:, :C], G_DQ, "dQ"), _on_grid(dqkv[:, C:2 * C], G_DK, "dK"), _on_grid(dqkv[:, 2 * C:], G_DV, "dV")
        ref["noise"] = _guard_noise(case_id(c), parts, L)
    return ref


def reference_pooled(inp, strict=True):
    """-> {"out" [B, C], "lse" [B * H], "dq" [B, C], "dkv" [M, 2C], "zero_rows" (bool [M]: rows behind a pooled causal query)}"""
    c = inp["case"]
    B, H, D, C = c["B"], c["H"], c["D"], inp["C"]
    out, dq, dkv = torch.zeros(B, C, dtype=F64), torch.zeros(B, C, dtype=F64), torch.zeros(inp["M"], 2 * C, dtype=F64)
    lse, count, parts = torch.zeros(B, H, dtype=F64), torch.zeros(B, H, dtype=torch.int64), []
    zero_rows = torch.zeros(inp["M"], dtype=torch.bool)
    if strict:
        assert torch.unique(inp["kv"][:, C:].reshape(-1, D), dim=0).shape[0] == inp["M"] * H, "V rows are not pairwise distinct"
    for b in range(B):
        n, r0 = inp["lens"][b], inp["off"][b]
        vis_max = c["qpos"][b] if c["causal"] else n - 1
        zero_rows[r0 + vis_max + 1:r0 + n] = True
        for h in range(H):
            col = h * D
            k, v = inp["kv"][r0:r0 + n, col:col + D], inp["kv"][r0:r0 + n, C + col:C + col + D]
            r = head_reference(inp["q"][b:b + 1, col:col + D], k, v, inp["dout"][b:b + 1, col:col + D], (torch.arange(n) <= vis_max)[None, :], strict=strict)
            out[b, col:col + D], dq[b, col:col + D] = r["out"][0], r["dq"][0]
            dkv[r0:r0 + n, col:col + D], dkv[r0:r0 + n, C + col:C + col + D] = r["dk"], r["dv"]
            lse[b, h], count[b, h] = r["lse"][0], r["count"][0]
            parts.append(r)
    ref = {"out": out, "dq": dq, "dkv": dkv, "lse": lse.reshape(-1), "count": count.reshape(-1), "zero_rows": zero_rows, "noise": 0.0}
    if strict:
        _on_grid(out, G_OUT, "out"), _on_grid(dq, G_DQ, "dQ"), _on_grid(dkv[:, :C], G_DK, "dK"), _on_grid(dkv[:, C:], G_DV, "dV")
        assert float(dkv[zero_rows].abs().max() if zero_rows.any() else 0.0) == 0.0
        ref["noise"] = _guard_noise(case_id(c), parts, c["L"])
    return ref


# ---- comparison (the same code judges the kernels on the GPU and the deliberately wrong references on the CPU) ------------------------------------
def as_kernel_output(x, dtype=BF16):
    """a float64 reference in the dtype a kernel returns it"""
    return x.to(F32).to(dtype)


def embed_rows(t, dtype, device):
    """``t`` as a row slice of a larger allocation whose rows in front of and behind it are NaN: contiguous and 16-byte aligned, as the wrappers ask"""
    parent = torch.full((t.shape[0] + 2 * PAD_ROWS,) + tuple(t.shape[1:]), math.nan, dtype=dtype, device=device)
    parent[PAD_ROWS:PAD_ROWS + t.shape[0]] = t.to(dtype)
    view = parent[PAD_ROWS:PAD_ROWS + t.shape[0]]
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    return view


def _where(bad, cols_per_head):
    idx = bad.nonzero()
    return f"{idx.shape[0]} of {bad.numel()} elements; first (row, head, dim): {[(int(r), int(col) // cols_per_head, int(col) % cols_per_head) for r, col in idx[:6].tolist()]}"


def assert_exact(name, got, want, D):
    """bf16 output against a float64 reference that is representable in bf16: equal element for element"""
    assert got.dtype == BF16 and got.shape == want.shape, (name, got.dtype, got.shape, want.shape)
    g = got.to(F64).cpu()
    assert bool(torch.isfinite(g).all()), f"{name}: non-finite output (a NaN guard row or a neighbour read into a product?): {_where(~torch.isfinite(g), D)}"
    if not torch.equal(g, want):
        raise AssertionError(f"{name}: differs from the exact result in {_where(g != want, D)}; max |diff| {float((g - want).abs().max()):.4g}")


def assert_on_grid(name, got, want, g_step, D):
    """|got - want| <= g / 8: fp32 noise where the true dS is 0 stays below g / 16, a wrong, missing or extra key moves a value by >= g.  -> max |diff|"""
    assert got.dtype == BF16 and got.shape == want.shape, (name, got.dtype, got.shape, want.shape)
    g = got.to(F64).cpu()
    assert bool(torch.isfinite(g).all()), f"{name}: non-finite output: {_where(~torch.isfinite(g), D)}"
    diff = (g - want).abs()
    mx = float(diff.max()) if diff.numel() else 0.0
    if mx > g_step / 8:
        raise AssertionError(f"{name}: off the grid (step {g_step}) in {_where(diff > g_step / 8, D)}; max |diff| {mx:.4g}")
    return mx


def assert_lse(name, got, want, count):
    """fp32 lse within 8 ulps of max(1, |ln count|); a wrong count moves it by at least ln(9 / 8).  NaN in ``want``: no such row"""
    assert got.dtype == F32 and got.numel() == want.numel(), (name, got.dtype, got.shape, want.shape)
    g, w, valid = got.to(F64).cpu().reshape(-1), want.reshape(-1), ~torch.isnan(want.reshape(-1))
    assert torch.allclose(w[valid], torch.log(count.reshape(-1)[valid].double()), rtol=0, atol=1e-15)
    mag = w[valid].abs().clamp_min(1.0)
    tol = 8 * torch.exp2(torch.floor(torch.log2(mag)) - 23)
    err = (g[valid] - w[valid]).abs()
    bad = ~(err <= tol)  # (a NaN is bad)
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} of {int(valid.sum())} values beyond 8 fp32 ulps; first (index, got, want): " \
                                f"{[(int(i), float(g[valid][i]), float(w[valid][i])) for i in bad.nonzero()[:6, 0].tolist()]}"
    return float(err.max())


def check_self(name, got, ref, inp):
    """got: {"out" bf16 [M, C], "dqkv" bf16 [M, 3C], "lse" fp32 [B * H * L]} -> measured (max |dQ - ref|, max |dK - ref|)"""
    C, D = inp["C"], inp["case"]["D"]
    assert_exact(name + " out", got["out"], ref["out"], D)
    assert_lse(name + " lse", got["lse"], ref["lse"], ref["count"])
    assert_exact(name + " dV", got["dqkv"][:, 2 * C:], ref["dqkv"][:, 2 * C:], D)
    return (assert_on_grid(name + " dQ", got["dqkv"][:, :C], ref["dqkv"][:, :C], G_DQ, D),
            assert_on_grid(name + " dK", got["dqkv"][:, C:2 * C], ref["dqkv"][:, C:2 * C], G_DK, D))


def check_pooled(name, got, ref, inp):
    """got: {"out", "dq" bf16 [B, C], "dkv" bf16 [M, 2C], "lse" fp32 [B * H]} -> measured (max |dq - ref|, max |dK - ref|)"""
    C, D = inp["C"], inp["case"]["D"]
    assert_exact(name + " out", got["out"], ref["out"], D)
    assert_lse(name + " lse", got["lse"], ref["lse"], ref["count"])
    assert_exact(name + " dV", got["dkv"][:, C:], ref["dkv"][:, C:], D)
    z = ref["zero_rows"]
    assert float(got["dkv"].cpu()[z].float().abs().max() if z.any() else 0.0) == 0.0, f"{name}: dK / dV rows behind the pooled token are not exact zeros"
    return assert_on_grid(name + " dq", got["dq"], ref["dq"], G_DQ, D), assert_on_grid(name + " dK", got["dkv"][:, :C], ref["dkv"][:, :C], G_DK, D)


def bucket_layout(lens, L):
    """(order, counts) as ocn_seq_bucket_plan gives them: sequence ids grouped by ceil(len / 32) ascending, one count per block count"""
    nb = torch.tensor([(n + 31) // 32 for n in lens])
    return torch.sort(nb, stable=True).indices.to(torch.int32), torch.bincount(nb - 1, minlength=(L + 31) // 32).tolist()
