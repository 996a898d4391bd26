"""CPU: ``open_clip_amd.create_optimizer`` -- the reference's parameter groups restated natively (against tests/golden/optimizer_groups.json, written by
tools/make_optimizer_groups_golden.py from the reference's own builders on its own CLIP, and against those builders run on the NativeCLIP itself), the
dispatch and every refusal -- and the host side of NativeNAdamW: its momentum schedule against torch.optim.NAdam, its checkpoints, and the argument
checks of ``ocn_nadamw_multi``."""
import fnmatch
import json
import os
import types

import pytest
import torch

from open_clip_amd.configs import get_model_config
from oracle.ref_shim import import_reference, reference_available

needs_reference = pytest.mark.skipif(not reference_available(), reason="reference tree not present")
GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optimizer_groups.json")))
MODELS, CASES = sorted(GOLDEN["groups"]), sorted(GOLDEN["cases"])


def _model(name="tiny-test"):
    from open_clip_amd.model import NativeCLIP
    cfg = get_model_config(name)
    return NativeCLIP(cfg["embed_dim"], cfg["vision_cfg"], cfg["text_cfg"], output_dict=True)


def _cfg(case, opt="adamw", **more):
    """the OptimizerCfg of a fixture case; a case with a fallback predicate is a Muon configuration (the only native optimizer that takes one)"""
    from open_clip_amd import OptimizerCfg
    fields = {k: v for k, v in GOLDEN["cases"][case].items() if k != "fallback"}
    if GOLDEN["cases"][case].get("fallback"):
        opt, fields["fallback_list"] = "muon", list(GOLDEN["fallback_list"])
    return OptimizerCfg(opt=opt, lr=GOLDEN["lr"], weight_decay=GOLDEN["weight_decay"], **fields, **more)


def _described(model, groups):
    names = {id(p): n for n, p in model.named_parameters()}
    return [{"group_name": g["group_name"], "weight_decay": g["weight_decay"], "lr_scale": g.get("lr_scale"), "use_fallback": bool(g.get("use_fallback", False)),
             "lr": g["lr"], "params": sorted(names[id(p)] for p in g["params"])} for g in groups]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("name", MODELS)
def test_groups_equal_the_fixture(name, case):
    """group order, names, weight decay, lr_scale, members and the initial lr, for every optimizer the case can be built with"""
    from open_clip_amd import create_optimizer
    model = _model(name)
    assert sorted(n for n, _ in model.named_parameters()) == GOLDEN["names"][name]
    want = [dict(g, params=[GOLDEN["names"][name][i] for i in g["params"]]) for g in GOLDEN["groups"][name][case]]
    for opt in (("muon",) if GOLDEN["cases"][case].get("fallback") else ("adamw", "nadamw")):
        got = _described(model, create_optimizer(model, _cfg(case, opt)).param_groups)
        assert [g["group_name"] for g in got] == [g["group_name"] for g in want]
        for g, w in zip(got, want):
            assert g["params"] == w["params"], g["group_name"]
            assert g["weight_decay"] == w["weight_decay"] and g["use_fallback"] == w["use_fallback"], g["group_name"]
            assert g["lr_scale"] == w["lr_scale"] and g["lr"] == w["lr"], g["group_name"]  # the same float expressions: equal to the bit
        assert sum(len(g["params"]) for g in got) == len(GOLDEN["names"][name])


@needs_reference
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("name", MODELS)
def test_reference_builders_on_the_native_model(name, case):
    """the reference's own builders run on the NativeCLIP: the same parameter OBJECTS, group by group, as the native builders give"""
    import_reference()
    from open_clip_train import optim as R
    from open_clip_amd import optim as N
    model = _model(name)
    c = _cfg(case)
    fallback_fn = (lambda n: any(fnmatch.fnmatchcase(n, pat) for pat in c.fallback_list)) if c.fallback_list else None
    args = (c.text_layer_decay, c.image_layer_decay)
    if any(args):
        want = R.layer_decay_param_groups(model, 0.2, *args, None, c.pooler_in_head, R.make_wd_exclude(model, c.wd_exclude_patterns), fallback_fn)
        got = N.layer_decay_param_groups(model, 0.2, *args, c.pooler_in_head, N.make_wd_exclude(model, c.wd_exclude_patterns), N.make_fallback_fn(c.fallback_list))
    else:
        want = R.wd_param_groups(model, 0.2, R.make_wd_exclude(model, c.wd_exclude_patterns), fallback_fn)
        got = N.wd_param_groups(model, 0.2, N.make_wd_exclude(model, c.wd_exclude_patterns), N.make_fallback_fn(c.fallback_list))
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert {k: v for k, v in g.items() if k != "params"} == {k: v for k, v in w.items() if k != "params"}
        assert [id(p) for p in g["params"]] == [id(p) for p in w["params"]], g["group_name"]


def test_dispatch_and_wiring():
    from open_clip_amd import NativeAdamW, NativeMuon, NativeNAdamW, OptimizerCfg, create_optimizer
    from open_clip_amd.optim import DEFAULT_FALLBACK
    model = _model()
    for opt, cls in (("adamw", NativeAdamW), ("NAdamW", NativeNAdamW), ("muon", NativeMuon)):
        o = create_optimizer(model, OptimizerCfg(opt=opt, lr=1e-3, beta1=0.9, beta2=0.95, eps=1e-7), grad_clip_norm=0.5, deterministic=True)
        assert type(o) is cls
        assert len(o.weight_caches) == 2 and o.weight_caches[0] is model._cache and o.weight_caches[1] is model.visual._cache
        assert o.grad_clip_norm == 0.5
        assert all(g["lr"] == 1e-3 and g["betas"] == (0.9, 0.95) and g["eps"] == 1e-7 for g in o.param_groups)
        if cls is not NativeMuon:
            assert o.deterministic is True
    # the optimizers' own defaults when the configuration sets neither betas nor eps
    o = create_optimizer(model, OptimizerCfg(opt="nadamw"))
    assert o.grad_clip_norm is None and o.deterministic is False
    assert all(g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8 and g["momentum_decay"] == 4e-3 and g["lr"] == 5e-4 for g in o.param_groups)
    assert [g["group_name"] for g in o.param_groups] == ["no_wd", "wd"] and [g["weight_decay"] for g in o.param_groups] == [0.0, 0.2]
    # Muon: the default fallback list, momentum when set, opt_kwargs merged last (they win over the typed fields)
    o = create_optimizer(model, OptimizerCfg(opt="muon", momentum=0.9, eps=1e-7, opt_kwargs={"fallback_lr_scale": 0.5, "eps": 1e-5}))
    names = {id(p): n for n, p in model.named_parameters()}
    listed = {names[id(p)] for g in o.param_groups if g.get("use_fallback") for p in g["params"]}
    assert listed == set(DEFAULT_FALLBACK) - {"logit_bias"}
    assert all(g["momentum"] == 0.9 and g["fallback_lr_scale"] == 0.5 and g["eps"] == 1e-5 for g in o.param_groups)
    o = create_optimizer(model, OptimizerCfg(opt="muon", opt_kwargs={"fallback_list": ["visual.*"]}))  # the reference's opt_kwargs spelling
    assert all(names[id(p)].startswith("visual.") == bool(g.get("use_fallback")) for g in o.param_groups for p in g["params"])
    assert create_optimizer(model, OptimizerCfg(opt="muon")).param_groups[0]["momentum"] == 0.95
    # DDP-like and torch.compile-like wrappers are unwrapped; any object with the fields serves as cfg
    wrapped = types.SimpleNamespace(module=types.SimpleNamespace(_orig_mod=model))
    o = create_optimizer(wrapped, types.SimpleNamespace(opt="adamw", lr=2e-3, weight_decay=0.1, beta1=None, beta2=None, eps=None), None, False)
    assert type(o) is NativeAdamW and sum(len(g["params"]) for g in o.param_groups) == len(list(model.parameters()))
    assert o.weight_caches[0] is model._cache and [g["weight_decay"] for g in o.param_groups] == [0.0, 0.1]


@needs_reference
def test_the_references_own_cfg_instance():
    import_reference()
    from open_clip_train.optim import OptimizerCfg as RefCfg
    from open_clip_amd import NativeNAdamW, OptimizerCfg, create_optimizer
    import dataclasses
    assert [(f.name, f.default) for f in dataclasses.fields(OptimizerCfg) if f.default is not dataclasses.MISSING] == \
        [(f.name, f.default) for f in dataclasses.fields(RefCfg) if f.default is not dataclasses.MISSING]
    assert [f.name for f in dataclasses.fields(OptimizerCfg)] == [f.name for f in dataclasses.fields(RefCfg)]
    model = _model()
    o = create_optimizer(model, RefCfg(opt="nadamw", lr=1e-3, text_layer_decay=0.75, image_layer_decay=0.65, pooler_in_head=False))
    want = GOLDEN["groups"]["tiny-test"]["both_decays"]
    assert type(o) is NativeNAdamW and [g["group_name"] for g in o.param_groups] == [g["group_name"] for g in want]
    assert [g["lr"] for g in o.param_groups] == [g["lr"] for g in want]


def test_refusals():
    from open_clip_amd import NativeNAdamW, OptimizerCfg, create_optimizer
    model = _model()
    with pytest.raises(TypeError, match="NativeCLIP.*Linear"):
        create_optimizer(torch.nn.Linear(2, 2), OptimizerCfg())
    with pytest.raises(NotImplementedError, match="tensorize"):
        create_optimizer(model, OptimizerCfg(), torch.device("cpu"), True)
    with pytest.raises(NotImplementedError, match=r"timm/lamb.*open_clip_train\.optim\.create_optimizer"):
        create_optimizer(model, OptimizerCfg(opt="timm/lamb"))
    with pytest.raises(NotImplementedError, match="timm/nadamuon"):
        create_optimizer(model, OptimizerCfg(opt="timm/nadamuon", fallback_list=["logit_scale"]))
    with pytest.raises(ValueError, match="Unknown optimizer sgd"):
        create_optimizer(model, OptimizerCfg(opt="SGD"))
    for key in ("text", "image", "audio"):
        for bad in (0.0, -0.5, 1.5):
            with pytest.raises(ValueError, match=rf"--{key}-layer-decay must be in \(0, 1\], got {bad}"):
                create_optimizer(model, OptimizerCfg(**{key + "_layer_decay": bad}))
    with pytest.raises(ValueError, match="audio_layer_decay=0.5.*no audio tower"):
        create_optimizer(model, OptimizerCfg(audio_layer_decay=0.5))
    for off in (None, 1.0):  # "off" for every tower, the absent one included
        o = create_optimizer(model, OptimizerCfg(text_layer_decay=off, image_layer_decay=off, audio_layer_decay=off))
        assert [g["group_name"] for g in o.param_groups] == ["no_wd", "wd"] and "lr_scale" not in o.param_groups[0]
    for opt in ("adamw", "nadamw"):
        with pytest.raises(ValueError, match=f"fallback_list.*{opt}"):
            create_optimizer(model, OptimizerCfg(opt=opt, fallback_list=["logit_scale"]))
        with pytest.raises(ValueError, match="fallback_list"):
            create_optimizer(model, OptimizerCfg(opt=opt, opt_kwargs={"fallback_list": ["logit_scale"]}))
        with pytest.raises(ValueError, match="BOTH beta1 and beta2"):
            create_optimizer(model, OptimizerCfg(opt=opt, beta1=0.9))
    with pytest.raises(ValueError, match="decoupled_weight_decay"):
        NativeNAdamW(list(model.parameters()), decoupled_weight_decay=False)
    with pytest.raises(ValueError, match="decoupled_weight_decay"):
        create_optimizer(model, OptimizerCfg(opt="nadamw", opt_kwargs={"decoupled_weight_decay": False}))
    with pytest.raises(ValueError, match="momentum_decay"):
        NativeNAdamW(list(model.parameters()), momentum_decay=-1.0)


@pytest.mark.parametrize("case", ["defaults", "both_decays", "fallback_both_decays"])
def test_frozen_parameters_are_in_no_group(case):
    from open_clip_amd import create_optimizer
    model = _model()
    model.lock_image_tower(unlocked_groups=1)
    frozen = {id(p) for p in model.parameters() if not p.requires_grad}
    assert frozen and len(frozen) < len(list(model.parameters()))
    o = create_optimizer(model, _cfg(case))
    members = [id(p) for g in o.param_groups for p in g["params"]]
    assert not frozen & set(members) and len(members) == len(set(members))
    assert set(members) == {id(p) for p in model.parameters() if p.requires_grad}
    assert all(g["params"] for g in o.param_groups)


def test_the_two_fixed_shape_builders_return_what_they_returned():
    """``param_groups_like_reference`` / ``muon_param_groups`` against a literal restatement of what they were before they shared the builders"""
    from open_clip_amd.optim import DEFAULT_FALLBACK, muon_param_groups, param_groups_like_reference

    def two_groups(model, weight_decay):
        skip = set(model.no_weight_decay())
        decay, no_decay = [], []
        for n, p in model.named_parameters():
            if p.requires_grad:
                (no_decay if (p.ndim <= 1 or n in skip) else decay).append(p)
        return [{"params": no_decay, "weight_decay": 0.0}, {"params": decay, "weight_decay": weight_decay}]

    def four_groups(model, weight_decay, patterns):
        skip = set(model.no_weight_decay())
        buckets = {}
        for n, p in model.named_parameters():
            if not p.requires_grad:
                continue
            no_wd, fb = p.ndim <= 1 or n in skip, any(fnmatch.fnmatchcase(n, pat) for pat in patterns)
            if (no_wd, fb) not in buckets:
                buckets[(no_wd, fb)] = {"params": [], "weight_decay": 0.0 if no_wd else weight_decay,
                                        "group_name": ("no_wd" if no_wd else "wd") + ("/fallback" if fb else "")}
                if fb:
                    buckets[(no_wd, fb)]["use_fallback"] = True
            buckets[(no_wd, fb)]["params"].append(p)
        return list(buckets.values())

    def same(got, want):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert list(g) == list(w) and {k: v for k, v in g.items() if k != "params"} == {k: v for k, v in w.items() if k != "params"}
            assert [id(p) for p in g["params"]] == [id(p) for p in w["params"]]

    for name in MODELS:
        for lock in (False, True):
            model = _model(name)
            if lock:
                model.lock_text_tower(unlocked_layers=1)
            same(param_groups_like_reference(model, 0.3), two_groups(model, 0.3))
            same(param_groups_like_reference(types.SimpleNamespace(module=model)), two_groups(model, 0.2))
            for patterns in (DEFAULT_FALLBACK, ("*.bias", "visual.*"), ()):
                same(muon_param_groups(model, 0.2, patterns), four_groups(model, 0.2, patterns))
            same(muon_param_groups(model, 0.1), four_groups(model, 0.1, DEFAULT_FALLBACK))


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_nadam_schedule_against_torch():
    """the host coefficients (``nadam_schedule``: c_g, c_m, bc2, mu_product) put through the update formula of ocn_nadamw_multi in float64, against
    torch.optim.NAdam(decoupled_weight_decay=True) on float64 CPU parameters and the same gradients, five steps.  Bound: rel-L2 <= 1e-6 (the bound of
    the AdamW kernel test); torch keeps mu_product in fp32, which moves 1 - mu_product by <= 1e-7 relative, everything else is the same arithmetic."""
    from open_clip_amd.optim import nadam_schedule
    g = torch.Generator().manual_seed(3)
    lr, wd, (b1, b2), eps, md = 1e-2, 0.2, (0.9, 0.98), 1e-6, 4e-3
    w0 = torch.randn(257, 33, generator=g, dtype=torch.float64)
    ref = torch.nn.Parameter(w0.clone())
    opt = torch.optim.NAdam([ref], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, momentum_decay=md, decoupled_weight_decay=True, foreach=False)
    p, m, v, mu_product = w0.clone(), torch.zeros_like(w0), torch.zeros_like(w0), 1.0
    for step in range(1, 6):
        grad = torch.randn(w0.shape, generator=g, dtype=torch.float64) * (0.1 + step)
        ref.grad = grad.clone()
        opt.step()
        mu_product, c_g, c_m, bc2 = nadam_schedule(step, mu_product, lr, b1, b2, md)
        p = p * (1 - lr * wd)
        m = m + (grad - m) * (1 - b1)
        v = v * b2 + grad * grad * (1 - b2)
        den = (v / bc2).sqrt() + eps
        p = p - (c_g * grad / den + c_m * m / den)
        st = opt.state[ref]
        errs = (_rel(p, ref.detach()), _rel(m, st["exp_avg"]), _rel(v, st["exp_avg_sq"]), abs(mu_product / float(st["mu_product"]) - 1.0))
        print(f"step {step}: rel-L2 param {errs[0]:.2e} exp_avg {errs[1]:.2e} exp_avg_sq {errs[2]:.2e}; mu_product rel {errs[3]:.2e}")
        assert max(errs) <= 1e-6, (step, errs)
    assert _rel(p, w0) > 1e-2  # five steps at lr 1e-2 moved the weights by percent: the bound resolves the update itself


def test_nadamw_checkpoints():
    """a torch.optim.NAdam checkpoint (``step`` and ``mu_product`` are 0-d tensors) loads; native -> native round-trips"""
    from open_clip_amd import NativeNAdamW
    from open_clip_amd.optim import nadam_schedule
    g = torch.Generator().manual_seed(4)
    params = [torch.nn.Parameter(torch.randn(5, 3, generator=g)), torch.nn.Parameter(torch.randn(7, generator=g))]
    groups = lambda ps: [{"params": [ps[0]], "weight_decay": 0.2, "group_name": "wd", "lr_scale": 0.75}, {"params": [ps[1]], "weight_decay": 0.0}]
    ref = torch.optim.NAdam(groups(params), lr=1e-2, betas=(0.9, 0.98), eps=1e-6, decoupled_weight_decay=True)
    for _ in range(2):
        for p in params:
            p.grad = torch.randn(p.shape, generator=g)
        ref.step()
    blob = ref.state_dict()
    assert torch.is_tensor(blob["state"][0]["step"]) and torch.is_tensor(blob["state"][0]["mu_product"])
    opt = NativeNAdamW(groups(params), lr=5e-4)
    assert opt.param_groups[0]["betas"] == (0.9, 0.999) and opt.param_groups[0]["momentum_decay"] == 4e-3  # torch's defaults
    opt.load_state_dict(blob)
    mu = nadam_schedule(2, nadam_schedule(1, 1.0, 1e-2, 0.9, 0.98, 4e-3)[0], 1e-2, 0.9, 0.98, 4e-3)[0]
    for p in params:
        st = opt.state[p]
        assert list(st) == ["step", "mu_product", "exp_avg", "exp_avg_sq"] == list(ref.state[p])
        assert type(st["step"]) is int and st["step"] == 2 and type(st["mu_product"]) is float and st["mu_product"] == pytest.approx(mu, rel=1e-6)
        assert torch.equal(st["exp_avg"], ref.state[p]["exp_avg"]) and torch.equal(st["exp_avg_sq"], ref.state[p]["exp_avg_sq"])
    g0 = opt.param_groups[0]
    assert (g0["lr"], g0["betas"], g0["eps"], g0["group_name"], g0["lr_scale"]) == (1e-2, (0.9, 0.98), 1e-6, "wd", 0.75)
    opt2 = NativeNAdamW(groups(params))
    opt2.load_state_dict(opt.state_dict())
    for p in params:
        a, b = opt.state[p], opt2.state[p]
        assert (a["step"], a["mu_product"]) == (b["step"], b["mu_product"]) and type(b["step"]) is int and type(b["mu_product"]) is float
        assert torch.equal(a["exp_avg"], b["exp_avg"]) and torch.equal(a["exp_avg_sq"], b["exp_avg_sq"])
    assert opt2.state_dict()["param_groups"] == opt.state_dict()["param_groups"]


def test_nadamw_multi_refuses_bad_arguments_before_any_launch():
    """host-side validation only: the fake device pointers are never dereferenced (as tests/test_cabi.py does)"""
    from open_clip_amd import _lib, build
    build.build()
    p = 4096
    with pytest.raises(RuntimeError, match=r"ocn_nadamw_multi failed \(-1\): ocn_nadamw_multi: null entry / chunk table"):
        _lib.call("ocn_nadamw_multi", None, p, 1, 0.1, 0.999, 0.001, 1e-8, None, 0.0, None)
    with pytest.raises(RuntimeError, match=r"ocn_nadamw_multi failed \(-1\): ocn_nadamw_multi: null entry / chunk table"):
        _lib.call("ocn_nadamw_multi", p, None, 1, 0.1, 0.999, 0.001, 1e-8, None, 0.0, None)
    for n in (0, -3):
        with pytest.raises(RuntimeError, match=r"ocn_nadamw_multi failed \(-1\): ocn_nadamw_multi: n_chunks must be positive"):
            _lib.call("ocn_nadamw_multi", p, p, n, 0.1, 0.999, 0.001, 1e-8, None, 0.0, None)
