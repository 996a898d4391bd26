"""MI355X: NativeMuon and its kernels against the float64 oracle of tests/muon_util.py.

The batched GEMM is checked in exact arithmetic (integer operands: bit-equal, no tolerance).  Everything that goes through the Newton-Schulz iteration
is judged per matrix by   err(native, oracle) <= 2 * err(emulation, oracle) + 2^-9   (relative Frobenius error; the emulation stores X, A and B in
bf16 -- the coarsest legal storage; the factor 2 covers another legal choice of rounding points; the right-hand side is computed per input)."""
import itertools
import math

import pytest
import torch

from open_clip_amd.configs import get_model_config
from open_clip_amd.synth import init_state_dict, synthetic_batch
from tests import gemm_exact as X
from tests import muon_util as U

pytestmark = pytest.mark.gpu
BACKENDS = ("batched", "per_matrix")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


# ---- 1. the batched GEMM in exact arithmetic ---------------------------------------------------------------------------------------------
def _stack_in_parent(t, fill, col_off, extra_cols):
    """t [batch, rows, cols] as a strided view inside a ``fill``-ed parent [batch, 8 + rows + 8, col_off + cols + extra_cols]"""
    b, rows, cols = t.shape
    ld = (col_off + cols + extra_cols + 7) // 8 * 8
    parent = torch.full((b, rows + 2 * X.PAD_ROWS, ld), fill, dtype=t.dtype, device=t.device)
    view = parent[:, X.PAD_ROWS:X.PAD_ROWS + rows, col_off:col_off + cols]
    view.copy_(t)
    return parent, view


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("with_r", [False, True])
@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (0.5, 2.0)])
def test_gemm_nt_batched_exact(dev, batch, with_r, alpha, beta):
    from open_clip_amd import ops
    nan = float("nan")
    for M, N, K in itertools.product((32, 96, 160, 288), (32, 96, 160, 288), (32, 96, 352)):
        g = torch.Generator().manual_seed(M * 7 + N * 3 + K + batch)
        a = X.int_operand((batch, M, K), X.R_NT, g, dev)
        b = X.int_operand((batch, N, K), X.R_NT, g, dev)
        r = X.int_operand((batch, M, N), X.BIAS_R, g, dev)
        pa, va = _stack_in_parent(a, nan, 8, 16)
        pb, vb = _stack_in_parent(b, nan, 16, 8)
        pr, vr = _stack_in_parent(r, nan, 8, 8)
        po, vo = _stack_in_parent(torch.full((batch, M, N), nan, dtype=torch.bfloat16, device=dev), X.SENTINEL, 24, 8)
        pt, vt = _stack_in_parent(torch.full((batch, N, M), nan, dtype=torch.bfloat16, device=dev), X.SENTINEL, 3, 5)  # any 2-byte alignment
        ops.gemm_nt_batched(va, vb, vo, resid=vr if with_r else None, out_t=vt, alpha=alpha, beta=beta)
        name = f"gemm_nt_batched {batch} x ({M}, {N}, {K}) R={with_r} alpha={alpha} beta={beta}"
        for i in range(batch):
            ref = X.exact_ref(a[i], b[i], "nt", alpha, (beta * r[i].double()) if with_r else None)
            want = X.rne_bf16(X.f32_exact(ref))
            X.assert_bit_equal(name, vo[i], want)
            X.assert_bit_equal(name + " (transposed)", vt[i], want.t())
            X.assert_outside_untouched(po[i], vo[i], X.SENTINEL, name)
            X.assert_outside_untouched(pt[i], vt[i], X.SENTINEL, name + " (transposed)")
            if not with_r:  # where both apply: the one-problem GEMM with the same epilogue
                single = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
                ops.gemm_nt(ops.EPI_BF16, va[i], vb[i], single, alpha=alpha)
                X.assert_bit_equal(name + " vs ocn_gemm_nt", vo[i].contiguous(), single)


def test_gemm_nt_batched_in_place_and_argument_checks(dev):
    from open_clip_amd import _lib, ops
    g = torch.Generator().manual_seed(1)
    a, b = X.int_operand((2, 96, 64), 8, g, dev), X.int_operand((2, 160, 64), 8, g, dev)
    r = X.int_operand((2, 96, 160), 64, g, dev)
    want = torch.stack([X.rne_bf16(X.f32_exact(X.exact_ref(a[i], b[i], "nt", 1.0, 0.5 * r[i].double()))) for i in range(2)])
    out = r.clone()
    ops.gemm_nt_batched(a, b, out, resid=out, beta=0.5)  # C aliases R
    X.assert_bit_equal("in place", out.reshape(-1, 160), want.reshape(-1, 160))
    with pytest.raises(RuntimeError, match="K=48 must be a multiple of 32"):
        _lib.call("ocn_gemm_nt_batched", 4096, 48, 0, 4096, 48, 0, 4096, 64, 0, 0, 0, 0, 0, 0, 0, 16, 64, 48, 1, 1.0, 0.0, 0)
    with pytest.raises(RuntimeError, match="row strides must be multiples of 8"):
        _lib.call("ocn_gemm_nt_batched", 4096, 36, 0, 4096, 32, 0, 4096, 64, 0, 0, 0, 0, 0, 0, 0, 16, 64, 32, 1, 1.0, 0.0, 0)


# ---- the iteration through the optimizer's public interface -------------------------------------------------------------------------------
def _orthogonalize(mats, backend, ns_steps=5):
    """X of every matrix, float64, from ONE optimizer step on zero weights: momentum 0 makes u = grad, lr = 1 and adjust_lr "original" make
    w = -sqrt(max(1, r / c)) * X"""
    from open_clip_amd.optim import NativeMuon
    params = [torch.nn.Parameter(torch.zeros_like(m)) for m in mats]
    for p, m in zip(params, mats):
        p.grad = m.clone()
    NativeMuon(params, lr=1.0, momentum=0.0, ns_steps=ns_steps, adjust_lr="original", _backend=backend).step()
    torch.cuda.synchronize()
    return [-p.detach().double() / U.lr_scale("original", p.shape[0], p[0].numel()) for p in params]


def _assert_parity(name, native, grad, others=()):
    """the bound of this module for one matrix; ``others``: further native results that must lie within the same bound of ``native``"""
    exact, emu = U.newton_schulz(grad.double()), U.newton_schulz(grad.double(), emulate=True)
    e_emu, e_nat = U.rel_err(emu, exact), U.rel_err(native, exact)
    msg = f"{name}: native vs oracle {e_nat:.4%}, emulation vs oracle {e_emu:.4%}, bound {U.bound(e_emu):.4%}"
    print(msg)
    assert e_nat <= U.bound(e_emu), msg
    for o in others:
        e = U.rel_err(o, native)
        assert e <= U.bound(e_emu), f"{name}: backends differ by {e:.4%}, bound {U.bound(e_emu):.4%}"


# ---- 2. parity ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", U.PARITY_KINDS)
@pytest.mark.parametrize("shape", U.PARITY_SHAPES)
def test_newton_schulz_parity(dev, shape, kind):
    """three different matrices of one shape in one call (one batched launch per product), both backends"""
    mats = [U.parity_input(shape, kind, seed=100 * i + shape[0] + shape[1], device=dev) for i in range(3)]
    got = {b: _orthogonalize(mats, b) for b in BACKENDS}
    for i, m in enumerate(mats):
        _assert_parity(f"{shape} {kind} [{i}] batched", got["batched"][i], m, others=[got["per_matrix"][i]])
        _assert_parity(f"{shape} {kind} [{i}] per_matrix", got["per_matrix"][i], m)


@pytest.mark.parametrize("backend", BACKENDS)
def test_newton_schulz_two_shapes_in_one_step(dev, backend):
    shapes = [(64, 192), (352, 588), (192, 64), (352, 588), (64, 192), (40, 72)]  # (64, 192) and (192, 64) share a workspace group
    mats = [U.parity_input(s, U.PARITY_KINDS[i % 2], seed=11 + i, device=dev) for i, s in enumerate(shapes)]
    for i, (m, x) in enumerate(zip(mats, _orthogonalize(mats, backend))):
        _assert_parity(f"mixed {shapes[i]} [{i}] {backend}", x, m)


# ---- 3. structure that rounding cannot blur ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shape", [(64, 192), (192, 64)])
def test_partial_permutations(dev, shape, backend):
    ks = (1, 7, 33, 64)
    mats = [U.partial_permutation(shape, k, seed=k, scale=0.37 * (i + 1), device=dev) for i, k in enumerate(ks)]
    for k, m, x in zip(ks, mats, _orthogonalize(mats, backend)):
        assert torch.equal(x == 0, m == 0), f"k={k}: nonzeros moved (tile edge, padding, transposition or cross-batch mix-up)"
        nz = x[m != 0]
        assert nz.numel() == k and bool((nz == nz[0]).all()), f"k={k}: the nonzeros differ from each other: {nz.unique().tolist()}"
        want = U.scalar_recursion(k)
        assert abs(float(nz[0]) / want - 1.0) <= 2.0 ** -5, f"k={k}: {float(nz[0])} vs the scalar recursion {want}"


# ---- 4. degenerate inputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_zero_gradient_moves_the_weight_by_its_decay_only(dev, backend):
    from open_clip_amd.optim import NativeMuon
    g = torch.Generator().manual_seed(3)
    ws = [torch.randn(s, generator=g).to(dev) for s in ((64, 192), (192, 64), (40, 72))]
    params = [torch.nn.Parameter(w.clone()) for w in ws]
    for p in params:
        p.grad = torch.zeros_like(p)
    opt = NativeMuon(params, lr=0.05, weight_decay=0.2, _backend=backend)
    opt.step()
    for p, w in zip(params, ws):
        assert torch.equal(p.detach(), w * torch.tensor(1.0 - 0.05 * 0.2, dtype=torch.float32)), tuple(p.shape)  # X is exactly 0
        assert not bool(opt.state[p]["momentum_buffer"].any())


@pytest.mark.parametrize("backend", BACKENDS)
def test_rank_deficient_gradient(dev, backend):
    mats = [U.low_rank_input(s, 4, seed=5 + i, device=dev) for i, s in enumerate(((64, 192), (192, 64)))]
    for m, x in zip(mats, _orthogonalize(mats, backend)):
        assert bool(torch.isfinite(x).all())
        emu = U.newton_schulz(m.double(), emulate=True)
        s_nat, s_emu = float(torch.linalg.matrix_norm(x, 2)), float(torch.linalg.matrix_norm(emu, 2))
        assert abs(s_nat / s_emu - 1.0) <= 0.05, (tuple(m.shape), s_nat, s_emu)


# ---- 5. the whole update ------------------------------------------------------------------------------------------------------------------
UPDATE_SHAPES = ((128, 128), (384, 128), (128, 512), (352, 3, 14, 14), (128,), ())
FALLBACK_MATRIX = (64, 32)  # a matrix in a use_fallback group
LR, FB_SCALE, BETAS, EPS, MOMENTUM = 0.02, 0.5, (0.9, 0.95), 1e-8, 0.95


def _update_inputs(dev):
    g = torch.Generator().manual_seed(17)
    shapes = UPDATE_SHAPES + (FALLBACK_MATRIX,)
    ws = [(0.05 * torch.randn(s, generator=g)).to(dev) for s in shapes]
    grads = [[(torch.randn(s, generator=g) * (0.3 + step)).to(dev) for s in shapes] for step in range(3)]
    return ws, grads


@pytest.mark.parametrize("clip", [None, 1.0])
@pytest.mark.parametrize("wd", [0.0, 0.2])
@pytest.mark.parametrize("adjust_lr", ["match_rms_adamw", "original"])
@pytest.mark.parametrize("nesterov", [True, False])
def test_whole_update_three_steps(dev, nesterov, adjust_lr, wd, clip):
    from open_clip_amd.optim import NativeAdamW, NativeMuon
    ws, grads = _update_inputs(dev)
    P = [torch.nn.Parameter(w.clone()) for w in ws]
    Q = [torch.nn.Parameter(w.clone()) for w in ws]  # NativeAdamW steps clones of ALL tensors, so that its global norm is the same
    opt = NativeMuon([{"params": P[:-1]}, {"params": P[-1:], "use_fallback": True, "group_name": "wd/fallback"}], lr=LR, weight_decay=wd,
                     momentum=MOMENTUM, nesterov=nesterov, adjust_lr=adjust_lr, betas=BETAS, eps=EPS, fallback_lr_scale=FB_SCALE, grad_clip_norm=clip)
    ref = NativeAdamW([{"params": Q[:-1]}, {"params": Q[-1:]}], lr=LR * FB_SCALE, betas=BETAS, eps=EPS, weight_decay=wd, grad_clip_norm=clip,
                      deterministic=True)
    bufs = [torch.zeros(w.shape, dtype=torch.float64, device=dev) for w in ws]
    for step in range(3):
        before = [p.detach().clone() for p in P]
        for p, q, gr in zip(P, Q, grads[step]):
            p.grad, q.grad = gr.clone(), gr.clone()
        opt.step()
        ref.step()
        coef = U.clip_coef(grads[step], clip)
        for i, (p, gr) in enumerate(zip(P, grads[step])):
            assert torch.equal(p.grad, gr), "`.grad` must stay unscaled"
            if p.ndim >= 2 and i < len(P) - 1:
                w0 = before[i].double()
                kw = dict(lr=LR, weight_decay=wd, momentum=MOMENTUM, nesterov=nesterov, ns_steps=5, adjust_lr=adjust_lr, clip_coef=coef)
                exact, buf = U.muon_update(w0, gr, bufs[i], **kw)
                emu, _ = U.muon_update(w0, gr, bufs[i], emulate=True, **kw)
                bufs[i] = buf
                e_emu, e_nat = U.rel_err(emu - w0, exact - w0), U.rel_err(p.detach().double() - w0, exact - w0)
                msg = f"step {step} {tuple(p.shape)}: dw native vs oracle {e_nat:.4%}, emulation vs oracle {e_emu:.4%}, bound {U.bound(e_emu):.4%}"
                print(msg)
                assert e_nat <= U.bound(e_emu), msg
                got = opt.state[p]["momentum_buffer"].double()
                # fp32 rounding: per step one rounding of the buffer and, scaled by 1 - momentum, two of gradient-sized terms -- under two roundings'
                # worth of the largest element, carried (x momentum) over three steps: 8 * 2^-24 of it is a safe ceiling
                assert float((got - buf).abs().max()) <= 8 * 2.0 ** -24 * float(buf.abs().max()), f"momentum buffer, step {step} {tuple(p.shape)}"
            else:
                assert torch.equal(p.detach(), Q[i].detach()), f"fallback parameter {tuple(p.shape)} differs from NativeAdamW at step {step}"
                assert "momentum_buffer" not in opt.state[p]


# ---- 6 - 9 on the model -------------------------------------------------------------------------------------------------------------------
def _model(dev, seed=5, batch_size=8):
    from open_clip_amd.model import NativeCLIP
    cfg = get_model_config("tiny-test")
    m = NativeCLIP(cfg["embed_dim"], cfg["vision_cfg"], cfg["text_cfg"], output_dict=True)
    m.load_state_dict(init_state_dict(cfg, seed=seed, perturb=True), strict=True)
    batch = {k: v.to(dev) for k, v in synthetic_batch(cfg, batch_size, seed=seed + 1).items()}
    return m.to(dev).train(), batch


def _backward(model, batch):
    from open_clip_amd.loss import NativeClipLoss
    model.zero_grad(set_to_none=True)
    out = model(image=batch["image"], text=batch["text"])
    loss = NativeClipLoss()(**out)
    loss.backward()
    return out, loss


def test_operand_copies_are_rewritten_by_the_step(dev):
    from open_clip_amd.optim import NativeMuon, muon_param_groups, takes_muon, weight_caches_of
    model, batch = _model(dev)
    caches = weight_caches_of(model)
    _backward(model, batch)
    groups = muon_param_groups(model, 0.2)
    held = {}
    for g in groups:
        for p in g["params"]:
            if p.ndim in (2, 4):
                kinds = {k: next((c.peek(p, k) for c in caches if c.peek(p, k) is not None), None) for k in "nt"}
                if any(v is not None for v in kinds.values()):
                    held[p] = (kinds, takes_muon(g, p))
    assert sum(muon for _, muon in held.values()) >= 8, "the towers' GEMM weights must have cached operand copies after a forward / backward"
    NativeMuon(groups, lr=0.02, weight_caches=caches).step()
    for p, (kinds, muon) in held.items():
        w2 = p.detach().reshape(p.shape[0], -1)
        tileable = w2.shape[0] % 64 == 0 and w2.shape[1] % 64 == 0
        for kind, t in kinds.items():
            if t is None or (kind == "t" and not (muon and tileable)):
                continue
            fresh = next(c for c in caches if c.peek(p, kind) is t).get(p, kind)
            assert fresh is t, f"{tuple(p.shape)} '{kind}': the copy was re-cast (a cache miss) instead of rewritten by the optimizer"
            assert torch.equal(t, (w2 if kind == "n" else w2.t().contiguous()).to(torch.bfloat16)), (tuple(p.shape), kind)
    with torch.no_grad():
        a = model(image=batch["image"], text=batch["text"])
        model.invalidate_weight_caches()
        b = model(image=batch["image"], text=batch["text"])
    for k in ("image_features", "text_features"):
        assert torch.equal(a[k], b[k]), k


def _snapshot(model, opt):
    return ([p.detach().clone() for p in model.parameters()],
            [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state[p].items()} for p in model.parameters()])


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and \
        all(sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) if torch.is_tensor(sa[k]) else sa[k] == sb[k] for k in sa) for sa, sb in zip(a[1], b[1]))


_GRADS = []


def _run(dev, steps, lrs=None, reload_after=None, grad_clip_norm=1.0):
    """``steps`` optimizer steps on tiny-test from one fixed state with the gradients of one fixed batch at the INITIAL weights (inputs, not a trajectory)"""
    from open_clip_amd.optim import NativeMuon, muon_param_groups
    model, batch = _model(dev)
    if not _GRADS:  # computed once: the model's backward sums its weight gradients with fp32 atomics, so two backward passes differ in the last bits
        _backward(model, batch)
        _GRADS.extend(None if p.grad is None else p.grad.clone() for p in model.parameters())
    for p, g in zip(model.parameters(), _GRADS):
        p.grad = None if g is None else g.clone()
    opt = NativeMuon(muon_param_groups(model, 0.2), lr=0.02, grad_clip_norm=grad_clip_norm)
    for s in range(steps):
        if lrs is not None:
            for g in opt.param_groups:
                g["lr"] = lrs[s]
        if reload_after == s:
            sd = opt.state_dict()
            opt = NativeMuon(muon_param_groups(model, 0.2), lr=123.0, grad_clip_norm=grad_clip_norm)
            opt.load_state_dict(sd)
        opt.step()
    torch.cuda.synchronize()
    return _snapshot(model, opt)


def test_step_is_reproducible_and_state_round_trips(dev):
    base = _run(dev, 2)
    assert _same(base, _run(dev, 2)), "two runs of the same steps differ"
    assert _same(base, _run(dev, 2, reload_after=1)), "state_dict() -> new optimizer -> load_state_dict() does not continue bit-identically"
    assert any("momentum_buffer" in st for st in base[1]) and any("exp_avg" in st for st in base[1])


def test_group_lr_changed_between_steps_takes_effect(dev):
    base, changed = _run(dev, 2, lrs=[0.02, 0.02]), _run(dev, 2, lrs=[0.02, 0.0])
    one = _run(dev, 1)
    assert not _same(base, changed)
    # lr = 0 in the second step: the weights stay where the first step left them (decay and update both scale with lr), the state still advances
    assert all(torch.equal(x, y) for x, y in zip(changed[0], one[0]))
    assert not _same(changed, one)


def test_training_sanity(dev):
    from open_clip_amd.optim import NativeMuon, muon_param_groups, takes_muon, weight_caches_of
    # 160 pairs: the last block of either tower sees ONE token per sample, so fewer samples than the width (128) would make its weight gradients
    # rank-deficient -- no parity inputs (tests/test_muon.py)
    model, batch = _model(dev, seed=9, batch_size=160)
    groups = muon_param_groups(model, 0.2)
    opt = NativeMuon(groups, lr=0.02, fallback_lr_scale=0.05, grad_clip_norm=1.0, weight_caches=weight_caches_of(model))
    losses = []
    for step in range(10):
        _, loss = _backward(model, batch)
        losses.append(float(loss))
        assert math.isfinite(losses[-1]), losses
        if step == 0:
            before = {p: (p.detach().clone(), p.grad.clone()) for g in groups for p in g["params"] if p.grad is not None}
        opt.step()
        if step == 0:
            coef = U.clip_coef([g for _, g in before.values()], 1.0)
            for g in groups:
                for p in g["params"]:
                    if not takes_muon(g, p) or p not in before:
                        continue
                    w0, gr = before[p][0].double(), before[p][1]
                    kw = dict(lr=0.02, weight_decay=g["weight_decay"], momentum=0.95, nesterov=True, ns_steps=5, adjust_lr="match_rms_adamw", clip_coef=coef)
                    zeros = torch.zeros_like(w0)
                    exact, emu = U.muon_update(w0, gr, zeros, **kw)[0], U.muon_update(w0, gr, zeros, emulate=True, **kw)[0]
                    e_emu, e_nat = U.rel_err(emu - w0, exact - w0), U.rel_err(p.detach().double() - w0, exact - w0)
                    assert e_nat <= U.bound(e_emu), f"{tuple(p.shape)}: dw native vs oracle {e_nat:.4%}, emulation {e_emu:.4%}, bound {U.bound(e_emu):.4%}"
    print("losses", [f"{v:.4f}" for v in losses])
    assert losses[-1] < losses[0], losses
