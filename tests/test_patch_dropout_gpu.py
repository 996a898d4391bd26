"""Patch dropout of the image tower on a real MI355X (reference transformer.py:17-58, :658, :804): the keep-plan kernel, the ``keep`` forms of
the patchify / assemble kernels against plain torch statements of the same gathers, and the whole training step against the reference's own
step with the same kept patches (tests/golden/small_patch_dropout.npz).  Bounds are written next to each check."""
import math

import numpy as np
import pytest
import torch

from tests.golden_util import check_grad, grad_keys
from tests.patch_dropout_util import fixture, inputs
from tests.test_kernels_gpu import _report, dev  # noqa: F401  (dev: module fixture)

pytestmark = pytest.mark.gpu

I32 = torch.int32


def _random_keep(B, G, K, dev, seed, never=None):
    """int32 [B, K]: K distinct patch indices per image in random (unsorted) order; patch ``never`` is kept by no image"""
    gen = torch.Generator().manual_seed(seed)
    pool = [g for g in range(G) if g != never]
    rows = [[pool[i] for i in torch.randperm(len(pool), generator=gen)[:K].tolist()] for _ in range(B)]
    return torch.tensor(rows, dtype=I32).to(dev)


# ---- the plan kernel ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,G,K", [(7, 36, 18), (3, 4, 1), (2, 36, 35), (2, 729, 364)])
def test_keep_plan(dev, B, G, K):
    from open_clip_amd import ops
    plans = []
    for seed in range(9):
        keep, inv = ops.patch_keep_plan(1000 + seed, B, G, K, dev)
        keep2, inv2 = ops.patch_keep_plan(1000 + seed, B, G, K, dev)
        assert torch.equal(keep, keep2) and torch.equal(inv, inv2), "the same seed must give the same bits"
        k = keep.cpu().long()
        assert keep.dtype == I32 and tuple(keep.shape) == (B, K) and inv.dtype == I32 and tuple(inv.shape) == (B, G)
        assert int(k.min()) >= 0 and int(k.max()) < G
        assert bool((k[:, 1:] > k[:, :-1]).all()), "every row strictly ascending"
        want = torch.full((B, G), -1, dtype=torch.long)
        want.scatter_(1, k, torch.arange(K).expand(B, K))
        assert torch.equal(inv.cpu().long(), want), "inv is the exact inverse, -1 elsewhere"
        plans.append(k)
    # Another seed / another image gives another subset.  A row is one of C(G, K) subsets: where that space is large (>= 1e6: a chance collision among
    # the few draws here has probability < 1e-4) EVERY pair must differ; in the two tiny spaces (4 and 36 subsets) chance collisions are likely, and
    # what a kernel that ignored the seed or the image index would show -- the same rows for all 9 seeds / in every plan -- must not happen
    # (by chance: <= (1/4)^8 for the seeds, (1/4)^9 for the rows).
    big = math.comb(G, K) >= 10 ** 6
    other_seed_differs = [not torch.equal(plans[0], p) for p in plans[1:]]
    rows_differ = [all(not torch.equal(p[a], p[b]) for a in range(B) for b in range(a + 1, B)) for p in plans]
    rows_not_all_equal = [any(not torch.equal(p[0], p[b]) for b in range(1, B)) for p in plans]
    if big:
        assert all(other_seed_differs) and all(rows_differ)
    else:
        assert any(other_seed_differs) and any(rows_not_all_equal)


def test_keep_plan_is_uniform(dev):
    """fixed seed, B = 4096 images, G = 49 (7 x 7), K = 24: every patch's keep frequency within 5 sigma of K / G, every horizontally adjacent
    pair's joint frequency within 5 sigma of K (K - 1) / (G (G - 1)) (correlated keys of neighbouring patches would show there);
    sigma = sqrt(p (1 - p) / B) of the respective p"""
    from open_clip_amd import ops
    B, G, K = 4096, 49, 24
    _, inv = ops.patch_keep_plan(20240607, B, G, K, dev)
    kept = (inv.cpu() >= 0).double()  # [B, G]
    assert bool((kept.sum(1) == K).all())
    p1 = K / G
    s1 = math.sqrt(p1 * (1 - p1) / B)
    f1 = kept.mean(0)
    p2 = K * (K - 1) / (G * (G - 1))
    s2 = math.sqrt(p2 * (1 - p2) / B)
    grid = kept.view(B, 7, 7)
    f2 = (grid[:, :, :-1] * grid[:, :, 1:]).mean(0)  # 42 pairs
    _report(f"patch_keep_plan uniformity: single max dev {float((f1 - p1).abs().max()) / s1:.2f} sigma, adjacent pair max dev {float((f2 - p2).abs().max()) / s2:.2f} sigma")
    assert float((f1 - p1).abs().max()) <= 5 * s1
    assert float((f2 - p2).abs().max()) <= 5 * s2


def test_keep_inverse(dev):
    from open_clip_amd import ops
    B, G, K = 5, 36, 18
    keep = _random_keep(B, G, K, dev, 3)
    inv = ops.patch_keep_inverse(keep, G).cpu().long()
    want = torch.full((B, G), -1, dtype=torch.long)
    want.scatter_(1, keep.cpu().long(), torch.arange(K).expand(B, K))
    assert torch.equal(inv, want)


# ---- patchify with keep ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,P", [(96, 16), (112, 14)])
@pytest.mark.parametrize("kind", ["fp32", "bf16", "u8_chw", "u8_hwc"])
def test_patchify_keep_is_a_row_gather_of_the_full_patchify(dev, size, P, kind):
    """bit-identical; unsorted keep; 112 px / patch 14 has Kpad = 640 > 3 P^2 = 588 (zero-padded columns) and takes the generic uint8 kernel,
    96 px / patch 16 in HWC order the LDS fast path"""
    from open_clip_amd import ops
    B, G = 3, (size // P) ** 2
    K = G // 2 - 1
    Kpad = (3 * P * P + 63) // 64 * 64
    keep = _random_keep(B, G, K, dev, 11)
    assert not bool((keep[:, 1:] > keep[:, :-1]).all())
    gen = torch.Generator().manual_seed(5)
    if kind in ("fp32", "bf16"):
        img = torch.randn(B, 3, size, size, generator=gen).to(dev)
        img = img.bfloat16() if kind == "bf16" else img
        full, got = ops.patchify(img, P, Kpad), ops.patchify(img, P, Kpad, keep=keep)
    else:
        hwc = kind == "u8_hwc"
        img = torch.randint(0, 256, (B, size, size, 3) if hwc else (B, 3, size, size), generator=gen, dtype=torch.uint8).to(dev)
        mean, std = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
        full, got = ops.patchify_u8(img, P, Kpad, mean, std, hwc), ops.patchify_u8(img, P, Kpad, mean, std, hwc, keep=keep)
    want = full.view(B, G, Kpad)[torch.arange(B, device=dev)[:, None], keep.long()].reshape(B * K, Kpad)
    assert tuple(got.shape) == (B * K, Kpad) and got.dtype == torch.bfloat16
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    if Kpad > 3 * P * P:
        assert float(got[:, 3 * P * P:].float().abs().max()) == 0.0


# ---- assemble ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,K", [(128, 18), (256, 1), (256, 35)])
def test_assemble_keep_fwd(dev, C, K):
    """one fp32 add per element: bit-identical to the torch expression"""
    from open_clip_amd import ops
    B, G = 5, 36
    gen = torch.Generator().manual_seed(C + K)
    po, cls, pos = torch.randn(B * K, C, generator=gen).to(dev), torch.randn(C, generator=gen).to(dev), torch.randn(G + 1, C, generator=gen).to(dev)
    keep = _random_keep(B, G, K, dev, 17)
    emb = ops.embed_assemble_fwd(po, cls, pos, B, G, C, keep=keep)
    want = torch.cat([(cls + pos[0]).expand(B, 1, C), po.view(B, K, C) + pos[1 + keep.long()]], dim=1).reshape(B * (K + 1), C)
    assert torch.equal(emb, want)


@pytest.mark.parametrize("C", [128, 256])
@pytest.mark.parametrize("K", [18, 1, 35])
def test_assemble_keep_bwd(dev, C, K):
    """dpatch: the bf16 rounding of the gathered rows, bit-identical.  dpos / dcls against a float64 sum: every element within
    B * 2^-24 * sum |terms| (fp32 summation of at most B terms, any order).  The deterministic form gives the same bits twice; a position no
    image kept gets exactly 0."""
    from open_clip_amd import ops
    B, G = 64, 36
    never = 35 if C == 128 else 0
    keep = _random_keep(B, G, K, dev, 100 + K, never=never)
    inv = ops.patch_keep_inverse(keep, G)
    demb = torch.randn(B * (K + 1), C, generator=torch.Generator().manual_seed(K)).to(dev)
    d3 = demb.view(B, K + 1, C).double()
    idx = (1 + keep.long()).reshape(-1)  # position of every kept row
    rows = d3[:, 1:].reshape(B * K, C)
    ref = torch.zeros(G + 1, C, dtype=torch.float64, device=dev).index_add_(0, idx, rows)
    mag = torch.zeros(G + 1, C, dtype=torch.float64, device=dev).index_add_(0, idx, rows.abs())
    ref[0], mag[0] = d3[:, 0].sum(0), d3[:, 0].abs().sum(0)
    bound = B * 2.0 ** -24 * mag
    results = []
    for det in (False, True, True):
        dpos, dcls = torch.zeros(G + 1, C, device=dev), torch.zeros(C, device=dev)
        dpatch = ops.embed_assemble_bwd(demb, dpos, dcls, B, G, C, deterministic=det, inv=inv, K=K)
        assert torch.equal(dpatch.view(torch.int16), demb.view(B, K + 1, C)[:, 1:].reshape(B * K, C).bfloat16().view(torch.int16))
        e_pos, e_cls = (dpos.double() - ref).abs(), (dcls.double() - ref[0]).abs()
        _report(f"embed_assemble_bwd with inv C={C} K={K} det={int(det)}: dpos max err/bound {float((e_pos / bound.clamp_min(1e-300)).max()):.3f} dcls {float((e_cls / bound[0]).max()):.3f}")
        assert bool((e_pos <= bound).all()) and bool((e_cls <= bound[0]).all())
        assert float(dpos[1 + never].abs().max()) == 0.0
        results.append((dpos, dcls))
    assert torch.equal(results[1][0], results[2][0]) and torch.equal(results[1][1], results[2][1])


# ---- keep = None is the identity keep ----------------------------------------------------------------------------------------------------
def _identity(B, G, dev):
    return torch.arange(G, dtype=I32, device=dev).expand(B, G).contiguous()


@pytest.mark.parametrize("size,P", [(96, 16), (112, 14)])
@pytest.mark.parametrize("kind", ["fp32", "bf16", "u8_chw", "u8_hwc"])
def test_patchify_identity_keep_is_the_dense_call(dev, size, P, kind):
    """keep[b] = arange(G) against keep = None, bit for bit (the geometries of the row-gather test above: LDS fast path / generic uint8 kernel with padding)"""
    from open_clip_amd import ops
    B, G = 3, (size // P) ** 2
    Kpad = (3 * P * P + 63) // 64 * 64
    keep = _identity(B, G, dev)
    gen = torch.Generator().manual_seed(6)
    if kind in ("fp32", "bf16"):
        img = torch.randn(B, 3, size, size, generator=gen).to(dev)
        img = img.bfloat16() if kind == "bf16" else img
        dense, got = ops.patchify(img, P, Kpad), ops.patchify(img, P, Kpad, keep=keep)
    else:
        hwc = kind == "u8_hwc"
        img = torch.randint(0, 256, (B, size, size, 3) if hwc else (B, 3, size, size), generator=gen, dtype=torch.uint8).to(dev)
        mean, std = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
        dense, got = ops.patchify_u8(img, P, Kpad, mean, std, hwc), ops.patchify_u8(img, P, Kpad, mean, std, hwc, keep=keep)
    assert tuple(dense.shape) == tuple(got.shape) == (B * G, Kpad)
    assert float(dense.float().abs().max()) > 0.0
    assert torch.equal(got.view(torch.int16), dense.view(torch.int16))


def test_assemble_fwd_identity_keep_is_the_dense_call(dev):
    from open_clip_amd import ops
    B, G, C = 5, 36, 128
    gen = torch.Generator().manual_seed(31)
    po, cls, pos = torch.randn(B * G, C, generator=gen).to(dev), torch.randn(C, generator=gen).to(dev), torch.randn(G + 1, C, generator=gen).to(dev)
    dense = ops.embed_assemble_fwd(po, cls, pos, B, G, C)
    got = ops.embed_assemble_fwd(po, cls, pos, B, G, C, keep=_identity(B, G, dev))
    assert tuple(dense.shape) == (B * (G + 1), C) and torch.equal(got, dense)


def test_assemble_bwd_identity_inv_is_the_dense_call(dev):
    """B = 40: two batch chunks of the atomic form, the second ragged (8 images).  dpatch bit-equal in both modes; dpos / dcls bit-equal in the
    deterministic form (a single writer in batch order); with atomics the two chunk sums arrive in either order, so each result is held to the
    file's bound B * 2^-24 * sum |terms| around the float64 sum, and the two results to the same bound of each other."""
    from open_clip_amd import ops
    B, G, C = 40, 36, 128
    inv = _identity(B, G, dev)
    demb = torch.randn(B * (G + 1), C, generator=torch.Generator().manual_seed(41)).to(dev)
    d3 = demb.view(B, G + 1, C).double()
    ref, bound = d3.sum(0), B * 2.0 ** -24 * d3.abs().sum(0)
    for det in (False, True):
        out = []
        for use_inv in (None, inv):
            dpos, dcls = torch.zeros(G + 1, C, device=dev), torch.zeros(C, device=dev)
            dpatch = ops.embed_assemble_bwd(demb, dpos, dcls, B, G, C, deterministic=det, inv=use_inv, K=G)
            out.append((dpatch, dpos, dcls))
        (p0, pos0, cls0), (p1, pos1, cls1) = out
        assert torch.equal(p0.view(torch.int16), p1.view(torch.int16))
        assert torch.equal(p0.view(torch.int16), demb.view(B, G + 1, C)[:, 1:].reshape(B * G, C).bfloat16().view(torch.int16))
        if det:
            assert torch.equal(pos0, pos1) and torch.equal(cls0, cls1)
        for dpos, dcls in ((pos0, cls0), (pos1, cls1)):
            assert bool(((dpos.double() - ref).abs() <= bound).all()) and bool(((dcls.double() - ref[0]).abs() <= bound[0]).all())
        d_pos, d_cls = (pos0.double() - pos1.double()).abs(), (cls0.double() - cls1.double()).abs()
        _report(f"embed_assemble_bwd identity inv vs dense det={int(det)}: dpos max diff/bound {float((d_pos / bound).max()):.3f} dcls {float((d_cls / bound[0]).max()):.3f}")
        assert bool((d_pos <= bound).all()) and bool((d_cls <= bound[0]).all())


# ---- the whole step ----------------------------------------------------------------------------------------------------------------------
def _build(cfg, state, prob, **kw):
    from open_clip_amd.model import NativeCLIP
    vision = dict(cfg["vision_cfg"], patch_dropout=prob) if prob is not None else cfg["vision_cfg"]
    m = NativeCLIP(cfg["embed_dim"], vision, cfg["text_cfg"], output_dict=True, **kw)
    m.load_state_dict(state, strict=True)
    return m.cuda().train()


@pytest.mark.parametrize("image_stream,pooled,recompute", [("fp32", True, False), ("fp32", False, False), ("fp32", True, True),
                                                           ("bf16", True, False), ("bf16", False, False), ("bf16", True, True)])
def test_step_against_reference_fixture(image_stream, pooled, recompute):
    """'small-test', B = 6, training mode, ``patch_keep`` = the indices the reference's PatchDropout drew (its own topk order), NativeClipLoss:
    features, loss and every gradient within the small-batch bounds of tests/test_model_gpu.py (features 4e-3, loss 2e-2, gradient rel-L2
    3.5e-2 matrices / 5e-2 1-D / 0.12 small)"""
    from open_clip_amd.loss import NativeClipLoss
    from tests.test_model_gpu import FEAT_TOL, LOSS_TOL, _grad_tol
    g, cfg, state, batch, keep = fixture()
    model = _build(cfg, state, 0.5, image_stream=image_stream, pooled_last_block=pooled)
    model.set_grad_checkpointing(recompute)
    out = model(image=batch["image"].cuda(), text=batch["text"].cuda(), patch_keep=keep.cuda())
    loss = NativeClipLoss()(**out)
    loss.backward()
    torch.cuda.synchronize()
    tag = f"patch_dropout step [{image_stream}, pooled={int(pooled)}, recompute={int(recompute)}]"
    fi = float((out["image_features"].float().cpu() - torch.from_numpy(g["out/image_features"])).abs().max())
    ft = float((out["text_features"].float().cpu() - torch.from_numpy(g["out/text_features"])).abs().max())
    dl = abs(float(loss.detach()) - float(g["out/loss"]))
    grads = {k: p.grad for k, p in model.named_parameters()}
    gmax = max(float(g["gnorm/" + k]) for k in grad_keys(g))
    worst = sorted(((check_grad(g, k, grads[k], 0)[0], k, float(g["gnorm/" + k])) for k in grad_keys(g)), reverse=True)
    _report(f"{tag}: image_features max_abs={fi:.3e} text_features max_abs={ft:.3e} loss={float(loss.detach()):.6f} ref={float(g['out/loss']):.6f}")
    for rel, k, n in worst[:8]:
        _report(f"{tag}:   grad rel_l2={rel:.3e} tol={_grad_tol(n, gmax, grads[k].ndim):.2e} |g|={n:.3e} {k}")
    assert fi <= FEAT_TOL and ft <= FEAT_TOL, (fi, ft)
    assert dl <= LOSS_TOL, dl
    for rel, k, n in worst:
        assert rel <= _grad_tol(n, gmax, grads[k].ndim), (k, rel, n)


def test_random_plan_is_governed_by_torch_manual_seed():
    cfg, state, batch = inputs()
    image, text = batch["image"].cuda(), batch["text"].cuda()
    model = _build(cfg, state, 0.5)
    feats, keeps = [], []
    with torch.no_grad():
        for seed in (5, 5, 6):
            torch.manual_seed(seed)
            feats.append(model.encode_image(image, normalize=True).clone())
            keeps.append(model.visual.patch_dropout.last_keep.clone())
        again = model.encode_image(image, normalize=True, keep=keeps[0])
    assert tuple(keeps[0].shape) == (6, 18) and keeps[0].dtype == I32
    assert torch.equal(keeps[0], keeps[1]) and torch.equal(feats[0], feats[1])
    assert not torch.equal(keeps[0], keeps[2])
    assert torch.equal(again, feats[0])


def test_random_step_is_bit_reproducible_when_deterministic():
    from open_clip_amd.loss import NativeClipLoss
    cfg, state, batch = inputs()
    image, text = batch["image"].cuda(), batch["text"].cuda()

    def run():
        model = _build(cfg, state, 0.5, deterministic=True)
        torch.manual_seed(77)
        loss = NativeClipLoss(deterministic=True)(**model(image=image, text=text))
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}

    (l1, g1), (l2, g2) = run(), run()
    assert torch.equal(l1, l2)
    diff = [k for k in g1 if not torch.equal(g1[k], g2[k])]
    assert not diff, diff[:6]


def test_switch_off_paths_are_bit_identical():
    """eval mode with patch_dropout = 0.5 runs every token: the bits of a model without the option.  Training with patch_dropout = 0 is the path
    of a model built without the key (deterministic step: the same bits for the loss and every gradient)."""
    from open_clip_amd.loss import NativeClipLoss
    cfg, state, batch = inputs()
    image, text = batch["image"].cuda(), batch["text"].cuda()
    half, none = _build(cfg, state, 0.5).eval(), _build(cfg, state, None).eval()
    with torch.no_grad():
        a, b = half(image=image, text=text), none(image=image, text=text)
    assert torch.equal(a["image_features"], b["image_features"]) and torch.equal(a["text_features"], b["text_features"])

    def run(prob):
        model = _build(cfg, state, prob, deterministic=True)
        out = model(image=image, text=text)
        loss = NativeClipLoss(deterministic=True)(**out)
        loss.backward()
        torch.cuda.synchronize()
        return out["image_features"].detach().clone(), loss.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}

    (f0, l0, g0), (f1, l1, g1) = run(0.0), run(None)
    assert torch.equal(f0, f1) and torch.equal(l0, l1)
    assert not [k for k in g0 if not torch.equal(g0[k], g1[k])]


def test_bad_keep_is_refused():
    cfg, state, batch = inputs()
    model = _build(cfg, state, 0.5)
    image = batch["image"].cuda()
    keep = _random_keep(6, 36, 18, "cuda", 1)
    with pytest.raises(ValueError):
        model.encode_image(image, keep=keep.long())
    with pytest.raises(ValueError):
        model.encode_image(image, keep=keep[:3])


# ---- the keep argument at the model boundary ---------------------------------------------------------------------------------------------
def test_keep_is_honoured_in_eval_mode():
    """eval mode draws nothing, but a ``keep`` passed to the call is followed there too: the same arithmetic as in training mode (no layer of
    the tower depends on the mode), so the same bits; not the full forward; the stored random plan is left alone"""
    cfg, state, batch = inputs()
    image = batch["image"].cuda()
    keep = _random_keep(6, 36, 18, "cuda", 21)
    model = _build(cfg, state, 0.5)
    with torch.no_grad():
        train = model.encode_image(image, normalize=True, keep=keep)
        model.eval()
        full = model.encode_image(image, normalize=True)
        evaluated = model.encode_image(image, normalize=True, keep=keep)
        plain = _build(cfg, state, None).eval().encode_image(image, normalize=True, keep=keep)  # a model without the option takes keep as well
    assert model.visual.patch_dropout.last_keep is None
    assert torch.equal(evaluated, train) and torch.equal(plain, train)
    assert not torch.equal(evaluated, full)


def test_keep_of_another_length_than_the_plan():
    """K' != num_keep(G) = 18 through encode_image and forward.  K' = G in ascending order is the full forward: the same rows in the same
    order through the same kernels at the same shapes, so the same bits.  K' = 7 (unsorted) through NativeCLIP.forward in training mode: image
    features against the fp32 CPU statement of the dropped forward (tests/test_patch_dropout.py) within the feature bound of
    tests/test_model_gpu.py for that comparison; the positional gradient is exactly 0 at every patch no image kept, and not at the kept ones."""
    from open_clip_amd.loss import NativeClipLoss
    from tests.test_model_gpu import FEAT_TOL
    from tests.test_patch_dropout import _dropped_encode_image
    cfg, state, batch = inputs()
    image, text = batch["image"].cuda(), batch["text"].cuda()
    model = _build(cfg, state, 0.5)
    every = torch.arange(36, dtype=I32, device="cuda").expand(6, 36).contiguous()
    with torch.no_grad():
        all_kept = model.encode_image(image, normalize=True, keep=every)
        full = model.eval().encode_image(image, normalize=True)
    assert torch.equal(all_kept, full)
    model.train()
    keep = _random_keep(6, 36, 7, "cuda", 23)
    out = model(image=image, text=text, patch_keep=keep)
    NativeClipLoss()(**out).backward()
    torch.cuda.synchronize()
    with torch.no_grad():
        want = _dropped_encode_image(batch["image"], state, cfg, keep.cpu())
    err = float((out["image_features"].float().cpu() - want).abs().max())
    _report(f"patch_keep of 7 through forward: image_features max_abs={err:.3e}")
    assert tuple(out["image_features"].shape) == tuple(want.shape) and err <= FEAT_TOL
    dpos = model.visual.positional_embedding.grad.cpu()
    kept = sorted(set(keep.cpu().reshape(-1).tolist()))
    never = sorted(set(range(36)) - set(kept))
    assert never and all(float(dpos[1 + n].abs().max()) == 0.0 for n in never)
    assert all(float(dpos[1 + k].abs().max()) > 0.0 for k in kept) and float(dpos[0].abs().max()) > 0.0
    assert model.visual.patch_dropout.last_keep is None, "a caller's keep is not the random plan"


def test_uint8_image_with_keep():
    """decoded pixels with ``keep`` (normalisation inside the keep patchify): [B,H,W,3] and [B,3,H,W] give the same bits, and the features of
    the normalised float image within the 2e-3 that tests/test_model_gpu.py::test_uint8_image_input_equals_normalised_float_input allows the
    same pair without keep; a training step on them runs and leaves finite gradients"""
    cfg, state, _ = inputs()
    model = _build(cfg, state, 0.5)
    S = cfg["vision_cfg"]["image_size"]
    u8 = torch.randint(0, 256, (5, S, S, 3), generator=torch.Generator().manual_seed(8), dtype=torch.uint8)
    mean = torch.tensor(model.visual.image_mean).view(1, 3, 1, 1)
    std = torch.tensor(model.visual.image_std).view(1, 3, 1, 1)
    f = (u8.permute(0, 3, 1, 2).float() / 255.0 - mean) / std
    keep = _random_keep(5, 36, 11, "cuda", 29)
    with torch.no_grad():
        a = model.encode_image(u8.cuda(), normalize=True, keep=keep)
        b = model.encode_image(u8.permute(0, 3, 1, 2).contiguous().cuda(), normalize=True, keep=keep)
        c = model.encode_image(f.cuda(), normalize=True, keep=keep)
    assert torch.equal(a, b)
    assert float((a - c).abs().max()) <= 2e-3
    feats = model.encode_image(u8.cuda(), normalize=True, keep=keep)
    (feats * torch.randn(feats.shape, generator=torch.Generator().manual_seed(9)).cuda()).sum().backward()
    torch.cuda.synchronize()
    grads = [p.grad for p in model.visual.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert float(model.visual.conv1.weight.grad.abs().max()) > 0.0
