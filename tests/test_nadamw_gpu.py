"""MI355X: ``ocn_nadamw_multi`` / ``NativeNAdamW`` against torch.optim.NAdam(decoupled_weight_decay=True) on the device, and training steps through
``open_clip_amd.create_optimizer``.  Bounds: fp32 elementwise arithmetic in the same order as torch's single-tensor form -- parameters and both moments
rel-L2 <= 1e-6 (the AdamW kernel's bound, tests/test_kernels_gpu.py), the gradient norm <= 1e-5 (an fp32 sum in another order); operand copies and
everything said to be reproducible: equal bits."""
import pytest
import torch

from open_clip_amd.configs import get_model_config
from open_clip_amd.synth import init_state_dict, synthetic_batch
from tests.test_kernels_gpu import _report, check, dev  # noqa: F401  (dev: the module fixture that loads the library)

pytestmark = pytest.mark.gpu

# tile mode with both copies | the same, one tile | vector path | 0-d | 2-D that is not 64-divisible (transposed copy re-cast) | vector path with a tail,
# more than one chunk | 4-D weight as [192, 192] | scalar path (odd size behind a 4-byte offset)
SHAPES = [(128, 192), (64, 64), (768,), (), (50, 768), (100003,), (192, 3, 8, 8), (24577,)]
HYPER = dict(betas=(0.9, 0.98), eps=1e-6)


def _groups(params):
    return [{"params": [p], "weight_decay": 0.0 if p.ndim <= 1 else 0.2, "lr": 1e-2 * (1 + i % 2)} for i, p in enumerate(params)]


def _three_steps(dev, deterministic, reference):
    """three NativeNAdamW steps on SHAPES (gradients scaled 0.1 + step, two of them views at a 4-byte offset, clip at 0.7); ``reference``: also step
    torch.optim.NAdam on twins and compare after every step"""
    from open_clip_amd.model import _WeightCache
    from open_clip_amd.optim import NativeNAdamW
    g = torch.Generator().manual_seed(5)
    ws = [torch.randn(sh, generator=g).to(dev) for sh in SHAPES]
    P = [torch.nn.Parameter(w.clone()) for w in ws]
    cache = _WeightCache()
    for p in P:
        if p.ndim in (2, 4):
            cache.get(p, "n"), cache.get(p, "t")
    held = {id(p): (cache.peek(p, "n"), cache.peek(p, "t")) for p in P}
    opt = NativeNAdamW(_groups(P), lr=1e-2, grad_clip_norm=0.7, weight_caches=[cache], deterministic=deterministic, **HYPER)
    if reference:
        R = [torch.nn.Parameter(w.clone()) for w in ws]
        ref = torch.optim.NAdam(_groups(R), lr=1e-2, decoupled_weight_decay=True, foreach=False, **HYPER)
    for step in range(3):
        for i, p in enumerate(P):
            gr = torch.randn(p.shape, generator=g).to(dev) * (0.1 + step)
            if i in (0, 5):  # gradient views at a 4-byte offset (DDP bucket views): unaligned tile path / scalar path
                buf = torch.empty(gr.numel() + 1, device=dev)
                buf[1:].copy_(gr.flatten())
                p.grad = buf[1:].view(p.shape)
            else:
                p.grad = gr.clone()
            if reference:
                R[i].grad = gr.clone()
        opt.step()
        if not reference:
            continue
        total = torch.nn.utils.clip_grad_norm_(R, 0.7)
        ref.step()
        check(f"nadamw_multi grad-norm step {step}", opt.last_grad_norm_sq.sqrt(), total.reshape(1), rel=1e-5)
        assert float(total) > 0.7  # the clip is active in every step
        for p, r in zip(P, R):
            tag = f"nadamw_multi step {step} {tuple(p.shape)}"
            check(tag + " param", p.detach().reshape(-1), r.detach().reshape(-1), rel=1e-6)
            check(tag + " exp_avg", opt.state[p]["exp_avg"].reshape(-1), ref.state[r]["exp_avg"].reshape(-1), rel=1e-6)
            check(tag + " exp_avg_sq", opt.state[p]["exp_avg_sq"].reshape(-1), ref.state[r]["exp_avg_sq"].reshape(-1), rel=1e-6)
            assert opt.state[p]["step"] == step + 1 and opt.state[p]["mu_product"] == pytest.approx(float(ref.state[r]["mu_product"]), rel=1e-6)
    return P, ws, cache, held


def test_kernel_against_torch_nadam(dev):  # noqa: F811
    P, ws, cache, held = _three_steps(dev, deterministic=False, reference=True)
    for p, w in zip(P, ws):
        if p.ndim >= 1:  # three steps at lr 1e-2 / 2e-2 move a weight by percent: 1e-6 of the weight resolves 1e-4 of the update
            assert float((p.detach() - w).norm() / w.norm()) > 1e-2, tuple(p.shape)
        if p.ndim in (2, 4):
            n16, t16 = cache.get(p, "n"), cache.get(p, "t")
            assert n16 is held[id(p)][0], "the optimizer must refresh the cached copy in place"
            tileable = p.shape[0] % 64 == 0 and (p.numel() // p.shape[0]) % 64 == 0
            assert (t16 is held[id(p)][1]) == tileable, "transposed copies of 64-divisible weights are refreshed in place, others re-cast"
            w2 = p.detach().reshape(p.shape[0], -1)
            assert torch.equal(n16, w2.to(torch.bfloat16)), tuple(p.shape)
            assert torch.equal(t16, w2.t().contiguous().to(torch.bfloat16)), tuple(p.shape)


def test_deterministic_steps_are_bit_reproducible(dev):  # noqa: F811
    a = _three_steps(dev, deterministic=True, reference=False)[0]
    b = _three_steps(dev, deterministic=True, reference=False)[0]
    for p, q in zip(a, b):
        assert torch.equal(p.detach(), q.detach()), tuple(p.shape)


def test_groups_must_share_the_kernel_arguments(dev):  # noqa: F811
    from open_clip_amd.optim import NativeNAdamW
    for key, other in (("betas", (0.9, 0.99)), ("eps", 1e-5), ("momentum_decay", 1e-3)):
        P = [torch.nn.Parameter(torch.ones(8, device=dev)) for _ in range(2)]
        opt = NativeNAdamW([{"params": [P[0]]}, {"params": [P[1]], key: other}])
        for p in P:
            p.grad = torch.ones_like(p)
        with pytest.raises(RuntimeError, match="NativeNAdamW: all param groups must share betas, eps and momentum_decay"):
            opt.step()


def _tiny(state, cfg):
    from open_clip_amd.model import NativeCLIP
    m = NativeCLIP(cfg["embed_dim"], cfg["vision_cfg"], cfg["text_cfg"], output_dict=True, deterministic=True)
    m.load_state_dict(state, strict=True)
    return m.cuda().train()


@pytest.fixture(scope="module")
def tiny(dev):  # noqa: F811
    cfg = get_model_config("tiny-test")
    return cfg, init_state_dict(cfg, seed=4, perturb=True), synthetic_batch(cfg, 8, seed=12, device="cuda")


def _forward_backward(model, batch):
    from open_clip_amd.loss import NativeClipLoss
    model.zero_grad(set_to_none=True)
    out = model(image=batch["image"], text=batch["text"])
    NativeClipLoss(deterministic=True)(**out).backward()
    return out


def test_training_steps_with_the_factory(tiny):
    """create_optimizer(opt="nadamw") with layer decay on both towers and the fused clip, against clip_grad_norm_ + torch.optim.NAdam over the same
    groups on twin parameters fed the model's gradients; and the operand copies the kernel rewrote are the casts of the new weights: the next forward
    equals, to the bit, that of a fresh model loaded from the stepped one's state_dict()"""
    from open_clip_amd import NativeNAdamW, OptimizerCfg, create_optimizer
    cfg, state, batch = tiny
    model = _tiny(state, cfg)
    opt = create_optimizer(model, OptimizerCfg(opt="nadamw", lr=1e-3, beta1=0.9, beta2=0.98, eps=1e-6, text_layer_decay=0.75, image_layer_decay=0.65),
                           grad_clip_norm=1.0, deterministic=True)
    assert type(opt) is NativeNAdamW and len(opt.param_groups) == 14 and len({g["lr"] for g in opt.param_groups}) == 7
    names = {id(p): n for n, p in model.named_parameters()}
    twin = {id(p): torch.nn.Parameter(p.detach().clone()) for p in model.parameters()}
    ref = torch.optim.NAdam([{"params": [twin[id(p)] for p in g["params"]], "weight_decay": g["weight_decay"], "lr": g["lr"]} for g in opt.param_groups],
                            lr=1e-3, betas=(0.9, 0.98), eps=1e-6, decoupled_weight_decay=True, foreach=False)
    _forward_backward(model, batch)
    for step in range(3):
        for p in model.parameters():
            twin[id(p)].grad = p.grad.detach().clone()
        total = torch.nn.utils.clip_grad_norm_(list(twin.values()), 1.0)
        ref.step()
        opt.step()
        assert abs(float(opt.last_grad_norm_sq.sqrt()) / float(total) - 1.0) <= 1e-5 and float(total) > 1.0
        worst = max((float((p.detach().double() - twin[id(p)].detach().double()).norm() / twin[id(p)].detach().double().norm()), names[id(p)])
                    for p in model.parameters())
        _report(f"create_optimizer(nadamw) training step {step}: worst parameter rel_l2 {worst[0]:.3e} ({worst[1]}), grad norm {float(total):.4f}")
        assert worst[0] <= 1e-6, worst
        out = _forward_backward(model, batch)  # the next forward, on the copies the optimizer rewrote
        fresh = _tiny(model.state_dict(), cfg)
        with torch.no_grad():
            want = fresh(image=batch["image"], text=batch["text"])
        for k in ("image_features", "text_features"):
            assert torch.equal(out[k].detach(), want[k]), (step, k)


@pytest.mark.parametrize("opt_name", ["adamw", "muon"])
def test_the_factory_changes_nothing_for_adamw_and_muon(tiny, opt_name):
    """without layer decay the factory's optimizer is the hand-built one over ``param_groups_like_reference`` / ``muon_param_groups``: two training steps
    leave the same bits in every parameter"""
    from open_clip_amd import OptimizerCfg, create_optimizer
    from open_clip_amd.optim import NativeAdamW, NativeMuon, muon_param_groups, param_groups_like_reference, weight_caches_of
    cfg, state, batch = tiny
    a, b = _tiny(state, cfg), _tiny(state, cfg)
    made = create_optimizer(a, OptimizerCfg(opt=opt_name, lr=1e-3, weight_decay=0.2, beta1=0.9, beta2=0.98, eps=1e-6), grad_clip_norm=1.0, deterministic=True)
    if opt_name == "adamw":
        hand = NativeAdamW(param_groups_like_reference(b, 0.2), lr=1e-3, betas=(0.9, 0.98), eps=1e-6, grad_clip_norm=1.0,
                           weight_caches=weight_caches_of(b), deterministic=True)
    else:
        hand = NativeMuon(muon_param_groups(b, 0.2), lr=1e-3, betas=(0.9, 0.98), eps=1e-6, grad_clip_norm=1.0, weight_caches=weight_caches_of(b))
    assert type(made) is type(hand)
    before = {k: p.detach().clone() for k, p in a.named_parameters()}
    for step in range(2):
        for model, opt in ((a, made), (b, hand)):
            _forward_backward(model, batch)
            opt.step()
        assert torch.equal(made.last_grad_norm_sq, hand.last_grad_norm_sq)
        diff = [k for (k, p), q in zip(a.named_parameters(), b.parameters()) if not torch.equal(p.detach(), q.detach())]
        assert not diff, (step, diff[:6])
    assert all(not torch.equal(p.detach(), before[k]) for k, p in a.named_parameters() if p.ndim >= 2)  # and the steps were steps
