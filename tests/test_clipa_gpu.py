"""The CLIPA model shape on a real MI355X: the mean-pooling kernels and the widening cast in exact arithmetic and against float64, single-query
attention without a mask at a query row that is not the first, and the whole training step of ``tiny-clipa-test`` against the reference's own step
(tests/golden/tiny_clipa.npz).  Bounds are written next to each check; measured values go to the parity report of tests/test_kernels_gpu.py (``_report``)."""
import pytest
import torch

from tests import clipa_util as U
from tests.golden_util import check_grad, grad_keys
from tests.test_kernels_gpu import _report, bf, check, dev  # noqa: F401  (dev: module fixture)

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
# (B, T, C): one patch and less than a wave of columns; 20 lanes of a bf16 row and T - 1 = 5; the parity twin's head; several column slabs and more
# tokens than waves; more than 512 tokens with C no multiple of 256 (the last slab of either dtype is ragged)
POOL_SHAPES = [(3, 2, 128), (1, 6, 160), (2, 17, 128), (5, 257, 1024), (2, 577, 1664)]
SENTINEL = 12345.0


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _pool_fwd(x, B, T, skip, C):
    """ocn_mean_pool_fwd into a buffer with a sentinel behind the result -> (out [B, C], the tail)"""
    from open_clip_amd import _lib
    buf = torch.full((B * C + 256,), SENTINEL, dtype=F32, device=x.device)
    _lib.call("ocn_mean_pool_fwd", x.data_ptr(), int(x.dtype == BF16), buf.data_ptr(), B, T, skip, C, _stream())
    return buf[:B * C].view(B, C), buf[B * C:]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("skip", [1, 0])
@pytest.mark.parametrize("B,T,C", POOL_SHAPES)
def test_mean_pool_fwd_is_exact_on_integers(dev, B, T, C, skip, dtype):
    """|v| <= 8: every partial sum is an integer below 2^24, exact in fp32 in any order, and ONE correctly rounded fp32 division of an exact sum rounds
    like the float64 quotient rounded once (53 >= 2 * 24 + 2 bits): bit-equal.  NaN in the class rows must not be read when they are skipped."""
    g = torch.Generator().manual_seed(B * 1000 + T + C + skip)
    x = torch.randint(-8, 9, (B, T, C), generator=g).to(dtype)
    want = (x[:, skip:].double().sum(1) / (T - skip)).float()
    if skip:
        x[:, :skip] = float("nan")
    xd = x.reshape(B * T, C).to(dev)
    out, tail = _pool_fwd(xd, B, T, skip, C)
    out2, _ = _pool_fwd(xd, B, T, skip, C)
    assert torch.equal(_bits(out.cpu()), _bits(want)), f"{int((_bits(out.cpu()) != _bits(want)).sum())} of {B * C} elements differ"
    assert torch.equal(_bits(out), _bits(out2)), "two runs must give the same bits"
    assert bool((tail == SENTINEL).all()), "store behind the result"


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,T,C", POOL_SHAPES)
def test_mean_pool_fwd_real_data(dev, B, T, C, dtype):
    """randn against the float64 mean: per element |err| <= 2^-24 * ((n - 1) / n * sum_t |x_t| + |mean|), n = T - skip -- the fp32 summation bound of
    n terms in any order ((n - 1) roundings, each at most 2^-24 of a partial sum <= sum |x_t|, to first order) plus the division's rounding"""
    from open_clip_amd import ops
    g = torch.Generator().manual_seed(B + T + C)
    x = torch.randn(B, T, C, generator=g).to(dtype)
    n = T - 1
    xs = x[:, 1:].double()
    mean = xs.sum(1) / n
    bound = 2.0 ** -24 * ((n - 1) / n * xs.abs().sum(1) + mean.abs())
    out = ops.mean_pool_fwd(x.reshape(B * T, C).to(dev), B, T, skip=1)
    err = (out.cpu().double() - mean).abs()
    _report(f"mean_pool_fwd[{B}x{T}x{C} {'bf16' if dtype == BF16 else 'fp32'}]: max err/bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert out.dtype == F32 and tuple(out.shape) == (B, C)
    assert bool((err <= bound).all())


@pytest.mark.parametrize("outputs", ["f32", "bf16", "both"])
@pytest.mark.parametrize("skip", [1, 0])
@pytest.mark.parametrize("B,T,C", POOL_SHAPES)
def test_mean_pool_bwd(dev, B, T, C, skip, outputs):
    """outputs prefilled with NaN: every row written, class rows exactly 0, the others bit-equal to the fp32 quotient dpooled / (T - skip) (torch's
    CPU division, itself checked against the once-rounded float64 quotient), the bf16 output to its round-to-nearest-even; a sentinel behind each"""
    from open_clip_amd import _lib
    g = torch.Generator().manual_seed(B + 3 * T + C + skip)
    dp = torch.randn(B, C, generator=g)
    want = dp / torch.tensor(float(T - skip))
    assert torch.equal(_bits(want), _bits((dp.double() / (T - skip)).float()))
    want = want[:, None, :].expand(B, T, C).clone()
    want[:, :skip] = 0.0
    n = B * T * C
    b32 = torch.full((n + 256,), float("nan"), dtype=F32, device=dev) if outputs != "bf16" else None
    b16 = torch.full((n + 256,), float("nan"), dtype=BF16, device=dev) if outputs != "f32" else None
    for buf in (b32, b16):
        if buf is not None:
            buf[n:] = SENTINEL
    _lib.call("ocn_mean_pool_bwd", dp.to(dev).data_ptr(), 0 if b32 is None else b32.data_ptr(), 0 if b16 is None else b16.data_ptr(), B, T, skip, C, _stream())
    torch.cuda.synchronize()
    if b32 is not None:
        got = b32[:n].view(B, T, C).cpu()
        assert bool(torch.isfinite(got).all()), "unwritten rows"
        assert torch.equal(_bits(got), _bits(want)) and float(got[:, :skip].abs().sum()) == 0.0
        assert bool((b32[n:] == SENTINEL).all())
    if b16 is not None:
        got = b16[:n].view(B, T, C).cpu()
        assert bool(torch.isfinite(got.float()).all()), "unwritten rows"
        assert torch.equal(_bits(got), _bits(want.bfloat16())) and float(got[:, :skip].float().abs().sum()) == 0.0
        assert bool((b16[n:] == torch.tensor(SENTINEL).bfloat16()).all())  # the sentinel as bf16 holds it


def test_mean_pool_ops_wrappers(dev):
    """ops.mean_pool_fwd / mean_pool_bwd: shapes, dtypes, the three output selections, and the refusal of a matrix that is not [B*T, C]"""
    from open_clip_amd import ops
    B, T, C = 2, 17, 128
    x = torch.randn(B * T, C, device=dev)
    assert torch.equal(ops.mean_pool_fwd(x, B, T), ops.mean_pool_fwd(x.clone(), B, T, skip=1))
    d = torch.randn(B, C, device=dev)
    dx, dx16 = ops.mean_pool_bwd(d, B, T)
    assert dx.dtype == F32 and dx16.dtype == BF16 and tuple(dx.shape) == tuple(dx16.shape) == (B * T, C)
    assert torch.equal(_bits(dx16), _bits(dx.bfloat16()))
    only16 = ops.mean_pool_bwd(d, B, T, want_f32=False)
    assert only16[0] is None and torch.equal(_bits(only16[1]), _bits(dx16))
    with pytest.raises(RuntimeError, match="mean_pool_fwd"):
        ops.mean_pool_fwd(x, B, T + 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.mean_pool_fwd(x.cpu(), B, T)


@pytest.mark.parametrize("n", [1, 7, 8 * 1024 + 3])
def test_cast_bf16_f32(dev, n):
    from open_clip_amd import _lib, ops
    g = torch.Generator().manual_seed(n)
    src = torch.randn(n, generator=g)
    src[0] = float("inf") if n > 1 else -0.0
    src[-1] = -0.0
    if n > 4:
        src[3] = 1e-40  # a bf16 subnormal
    src16 = src.bfloat16().to(dev)
    buf = torch.full((n + 64,), SENTINEL, dtype=F32, device=dev)
    _lib.call("ocn_cast_bf16_f32", src16.data_ptr(), buf.data_ptr(), n, _stream())
    assert torch.equal(_bits(buf[:n]), _bits(src16.float())) and bool((buf[n:] == SENTINEL).all())
    assert torch.equal(_bits(ops.cast_f32(src16)), _bits(src16.float()))


@pytest.mark.parametrize("L,qrow", [(16, 15), (32, 31), (77, 76), (32, 13)])
def test_single_query_attention_without_a_mask_at_a_later_row(dev, L, qrow):
    """ocn_attn_pooled_fwd / _bwd with causal = 0 and the query at row L - 1 (the 'last' text pooling) or in the middle: the query sees ALL L keys
    whatever its row is.  Against fp32 torch over all keys, tolerances of tests/test_kernels_gpu.py::test_attention_pooled_single_query."""
    from open_clip_amd import ops
    g = torch.Generator().manual_seed(L * 100 + qrow)
    B, H = 6, 3
    C = H * 64
    kv = bf(torch.randn(B * L, 2 * C, generator=g) * 1.5).to(dev)
    q = bf(torch.randn(B, C, generator=g) * 1.5).to(dev)
    dout = bf(torch.randn(B, C, generator=g)).to(dev)
    rows = (torch.arange(B, dtype=torch.int32) * L + qrow).to(dev)
    out, lse = ops.attn_pooled_fwd(q, kv, rows, B, L, H, False, 0.125)
    dq, dkv = ops.attn_pooled_bwd(q, kv, out, dout, lse, rows, B, L, H, False, 0.125)
    qf, kvf = q.float().requires_grad_(True), kv.float().requires_grad_(True)
    k = kvf[:, :C].reshape(B, L, H, 64).permute(0, 2, 1, 3)  # [B, H, L, 64]
    v = kvf[:, C:].reshape(B, L, H, 64).permute(0, 2, 1, 3)
    s = (k @ qf.reshape(B, H, 64, 1)).squeeze(-1) * 0.125   # [B, H, L]: every key
    ref_out = (torch.softmax(s, dim=-1).unsqueeze(2) @ v).reshape(B, C)
    ref_out.backward(dout.float())
    tag = f"attn_pooled[no mask, L={L}, query row {qrow}]"
    check(tag + " out", out, ref_out.detach(), rel=4e-3)
    check(tag + " lse", lse, torch.logsumexp(s, dim=-1).reshape(-1).detach(), rel=1e-5)
    check(tag + " dq", dq, qf.grad, rel=1e-2)
    check(tag + " dkv", dkv, kvf.grad, rel=1e-2)
    assert bool(torch.isfinite(dkv.float()).all())
    assert bool((dkv.float().abs().sum(1) > 0).all()), "every key row carries gradient without a mask"


# ---- the whole step ----------------------------------------------------------------------------------------------------------------------
def _build(cfg, state, vision=None, **kw):
    from open_clip_amd.model import NativeCLIP
    m = NativeCLIP(cfg["embed_dim"], dict(cfg["vision_cfg"], **(vision or {})), cfg["text_cfg"], output_dict=True, **kw)
    m.load_state_dict(state, strict=True)
    return m.cuda().train()


def _grad_bound(g, key, ndim, stream):
    """DESIGN section 2, small batches: rel-L2 <= 3.5e-2 (matrices, embeddings) / 5e-2 (1-D) on the fp32 stream, 6e-2 / 7e-2 on the bf16 stream
    (tests/test_bf16_stream_gpu.py); on the bf16 stream a gradient may exceed its bound where the reference's own autocast policy does on this very
    step (``policy/<key>`` of the fixture), no further than that and never beyond twice the bound (tests/test_parity_at_size_gpu.py::stream_bound)"""
    if stream == "fp32":
        return 3.5e-2 if ndim >= 2 else 5e-2
    tol = 6e-2 if ndim >= 2 else 7e-2
    return max(tol, min(2.0 * tol, float(g["policy/" + key]))) if "policy/" + key in g else tol


@pytest.mark.parametrize("image_stream,recompute", [("fp32", False), ("bf16", False), ("fp32", True), ("bf16", True)])
def test_step_against_reference_fixture(image_stream, recompute):
    """'tiny-clipa-test', B = 6, training mode, NativeClipLoss against the reference's own CLIPTask step: features max-abs <= 4e-3, loss <= 2e-2,
    every gradient inside ``_grad_bound``"""
    from open_clip_amd.loss import NativeClipLoss
    g, cfg, state, batch = U.fixture()
    model = _build(cfg, state, image_stream=image_stream)
    assert not model.pack_text and model.attn_mask is None
    model.set_grad_checkpointing(recompute)
    out = model(image=batch["image"].cuda(), text=batch["text"].cuda())
    loss = NativeClipLoss()(**out)
    loss.backward()
    torch.cuda.synchronize()
    tag = f"clipa step [{image_stream}, recompute={int(recompute)}]"
    fi = float((out["image_features"].float().cpu() - torch.from_numpy(g["out/image_features"])).abs().max())
    ft = float((out["text_features"].float().cpu() - torch.from_numpy(g["out/text_features"])).abs().max())
    dl = abs(float(loss.detach()) - float(g["out/loss"]))
    grads = {k: p.grad for k, p in model.named_parameters()}
    assert set(grads) == set(grad_keys(g)) and all(v is not None for v in grads.values())
    rows = sorted(((check_grad(g, k, grads[k], 0)[0], k) for k in grad_keys(g)), reverse=True)
    _report(f"{tag}: image_features max_abs={fi:.3e} text_features max_abs={ft:.3e} loss={float(loss.detach()):.6f} ref={float(g['out/loss']):.6f}")
    for rel, k in rows[:8]:
        _report(f"{tag}:   grad rel_l2={rel:.3e} bound={_grad_bound(g, k, grads[k].ndim, image_stream):.2e} |g|={float(g['gnorm/' + k]):.3e} {k}")
    assert fi <= 4e-3 and ft <= 4e-3, (fi, ft)
    assert dl <= 2e-2, dl
    bad = [(k, rel, _grad_bound(g, k, grads[k].ndim, image_stream)) for rel, k in rows if not rel <= _grad_bound(g, k, grads[k].ndim, image_stream)]
    assert not bad, bad


@pytest.mark.parametrize("image_stream", ["fp32", "bf16"])
def test_deterministic_step_gives_the_same_bits_twice(image_stream):
    from open_clip_amd.loss import NativeClipLoss
    cfg, state, batch = U.inputs()
    image, text = batch["image"].cuda(), batch["text"].cuda()

    def run():
        model = _build(cfg, state, image_stream=image_stream, deterministic=True)
        loss = NativeClipLoss(deterministic=True)(**model(image=image, text=text))
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}

    (l1, g1), (l2, g2) = run(), run()
    assert torch.equal(l1, l2)
    diff = [k for k in g1 if not torch.equal(g1[k], g2[k])]
    assert not diff, diff[:6]


def test_padding_is_visible_without_a_mask_and_invisible_behind_one():
    """one token changed at a padding position: the bidirectional CLIPA tower's feature of that caption moves by more than 1e-3 (a packed text tower
    would be wrong for it); on 'tiny-test' (causal mask, argmax pooling) the features keep their bits"""
    from open_clip_amd.configs import get_model_config
    from open_clip_amd.synth import init_state_dict, synthetic_batch
    cfg, state, batch = U.inputs()
    text = batch["text"].cuda()
    b = int((text[:, -2] == 0).nonzero()[0])
    text2 = text.clone()
    text2[b, -2] = 7
    model = _build(cfg, state).eval()
    with torch.no_grad():
        a, c = model.encode_text(text, normalize=True), model.encode_text(text2, normalize=True)
    moved = float((a[b] - c[b]).abs().max())
    _report(f"clipa padding token changed: text feature moves by {moved:.3e}")
    assert moved > 1e-3
    others = [i for i in range(text.shape[0]) if i != b]
    assert torch.equal(a[others], c[others])
    tcfg = get_model_config("tiny-test")
    tstate = init_state_dict(tcfg, seed=5, perturb=True)
    ttext = synthetic_batch(tcfg, 6, seed=141)["text"].cuda()
    tb = int((ttext[:, -2] == 0).nonzero()[0])
    ttext2 = ttext.clone()
    ttext2[tb, -2] = 7
    for pack in (True, False):
        tm = _build(tcfg, tstate, pack_text=pack).eval()
        assert tm.pack_text is pack
        with torch.no_grad():
            assert torch.equal(tm.encode_text(ttext, normalize=True), tm.encode_text(ttext2, normalize=True))


def test_mean_runs_over_the_kept_patches():
    """``keep`` with K' = 5 of the 16 patches in unsorted order: the mean is over those 5 tokens (features within 4e-3 of the elementary forward with
    the same keep).  A training step with patch_dropout = 0.5 leaves finite gradients, and exactly 0 for the position of a patch nobody kept."""
    from open_clip_amd.loss import NativeClipLoss
    cfg, state, batch = U.inputs()
    image, text = batch["image"].cuda(), batch["text"].cuda()
    gen = torch.Generator().manual_seed(9)
    keep = torch.stack([torch.randperm(16, generator=gen)[:5] for _ in range(image.shape[0])]).to(torch.int32)
    assert not bool((keep[:, 1:] > keep[:, :-1]).all())
    model = _build(cfg, state).eval()
    with torch.no_grad():
        got = model.encode_image(image, normalize=True, keep=keep.cuda())
        full = model.encode_image(image, normalize=True)
        want = U.encode_image(batch["image"], state, cfg, keep=keep)
    err = float((got.float().cpu() - want).abs().max())
    _report(f"clipa encode_image with keep of 5: max_abs={err:.3e}")
    assert err <= 4e-3 and not torch.equal(got, full)
    # training mode, random plan: two images, so that some patch is kept by neither (the seed is chosen for that; the plan follows torch.manual_seed)
    model = _build(cfg, state, vision={"patch_dropout": 0.5})
    never = []
    for seed in range(16):
        torch.manual_seed(seed)
        with torch.no_grad():
            model.encode_image(image[:2], normalize=True)
        plan = model.visual.patch_dropout.last_keep.clone()
        never = sorted(set(range(16)) - set(plan.cpu().reshape(-1).tolist()))
        if never:
            break
    assert never and tuple(plan.shape) == (2, 8)
    torch.manual_seed(seed)
    out = model(image=image[:2], text=text[:2])
    assert torch.equal(model.visual.patch_dropout.last_keep, plan)
    NativeClipLoss()(**out).backward()
    torch.cuda.synchronize()
    grads = {k: p.grad for k, p in model.named_parameters()}
    assert all(v is not None and bool(torch.isfinite(v).all()) for v in grads.values())
    dpos = model.visual.positional_embedding.grad.cpu()
    assert all(float(dpos[1 + n].abs().max()) == 0.0 for n in never)
    kept = sorted(set(plan.cpu().reshape(-1).tolist()))
    assert all(float(dpos[1 + k].abs().max()) > 0.0 for k in kept)
