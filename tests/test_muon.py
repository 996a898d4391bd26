"""CPU: the host side of NativeMuon -- parameter grouping against the reference's ``wd_param_groups``, the routing rule, constructor validation --
and the yardsticks of tests/test_muon_gpu.py: the bf16-storage emulation's own distance from the float64 oracle (tests/muon_util.py) on the parity
inputs, and the scalar recursion that a partial permutation follows."""
import fnmatch

import pytest
import torch

from open_clip_amd.configs import get_model_config
from oracle.ref_shim import import_reference, reference_available
from tests import muon_util as U

needs_reference = pytest.mark.skipif(not reference_available(), reason="reference tree not present")


def _tiny(name="tiny-test"):
    from open_clip_amd.model import NativeCLIP
    cfg = get_model_config(name)
    return NativeCLIP(cfg["embed_dim"], cfg["vision_cfg"], cfg["text_cfg"], output_dict=True)


def _described(model, groups):
    names = {id(p): n for n, p in model.named_parameters()}
    return [({k: v for k, v in g.items() if k != "params"}, [names[id(p)] for p in g["params"]]) for g in groups]


@needs_reference
@pytest.mark.parametrize("fallback", ["default", ("*.bias", "visual.*"), ()])
def test_groups_equal_the_reference(fallback):
    import_reference()
    from open_clip_train.optim import wd_param_groups
    from open_clip_amd.optim import DEFAULT_FALLBACK, muon_param_groups
    model = _tiny()
    pats = DEFAULT_FALLBACK if fallback == "default" else fallback
    fallback_fn = (lambda name: any(fnmatch.fnmatchcase(name, pat) for pat in pats)) if pats else None  # optim.py:392-394
    want = _described(model, wd_param_groups(model, 0.2, None, fallback_fn))
    got = _described(model, muon_param_groups(model, 0.2, pats))
    assert got == want
    assert sum(len(names) for _, names in got) == len(list(model.parameters()))
    if fallback == "default":
        assert [m["group_name"] for m, _ in got] == [m["group_name"] for m, _ in want] and len(got) == 4
        assert all(m.get("use_fallback", False) == m["group_name"].endswith("/fallback") for m, _ in got)


def test_default_fallback_names_exist_and_route():
    """which of tiny-test's parameters take Muon: a table by name"""
    from open_clip_amd.optim import DEFAULT_FALLBACK, muon_param_groups, takes_muon
    model = _tiny()
    names = {id(p): n for n, p in model.named_parameters()}
    route = {names[id(p)]: takes_muon(g, p) for g in muon_param_groups(model, 0.2) for p in g["params"]}
    shapes = {n: tuple(p.shape) for n, p in model.named_parameters()}
    assert set(route) == set(shapes)
    expected = {
        "visual.conv1.weight": True,  # 4-D, used as [width, 3 * patch * patch]
        "visual.transformer.resblocks.0.attn.in_proj_weight": True,  # one [3C, C] matrix
        "visual.transformer.resblocks.0.attn.out_proj.weight": True,
        "visual.transformer.resblocks.0.mlp.c_fc.weight": True,
        "transformer.resblocks.0.mlp.c_proj.weight": True,
        "visual.proj": True,
        "text_projection": True,
        "visual.transformer.resblocks.0.ln_1.weight": False,  # 1-D gains and biases
        "visual.transformer.resblocks.0.attn.in_proj_bias": False,
        "transformer.resblocks.0.mlp.c_fc.bias": False,
        "ln_final.bias": False,
        "logit_scale": False,  # scalar (and on the list)
        "token_embedding.weight": False,  # the DEFAULT_FALLBACK names
        "positional_embedding": False,
        "visual.positional_embedding": False,
        "visual.class_embedding": False,
    }
    assert len(shapes["visual.conv1.weight"]) == 4 and shapes["logit_scale"] == ()
    for n, want in expected.items():
        assert route[n] == want, n
    for n, muon in route.items():  # and the rule itself for every parameter
        listed = any(fnmatch.fnmatchcase(n, pat) for pat in DEFAULT_FALLBACK)
        assert muon == (len(shapes[n]) >= 2 and not listed), n
    present = [pat for pat in DEFAULT_FALLBACK if pat in shapes]
    assert set(DEFAULT_FALLBACK) - set(present) == {"logit_bias"}  # tiny-test (a CLIP-loss model) has no logit_bias; every other name exists
    # a Muon group's parameters with ndim < 2 fall back; a fallback group's matrices do too
    p1, p2 = torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(4, 4))
    assert not takes_muon({}, p1) and takes_muon({}, p2) and takes_muon({"use_fallback": False}, p2) and not takes_muon({"use_fallback": True}, p2)


def test_constructor_validation_and_defaults():
    from open_clip_amd.optim import NativeMuon
    p = [torch.nn.Parameter(torch.zeros(8, 8))]
    with pytest.raises(ValueError, match="adjust_lr"):
        NativeMuon(p, adjust_lr="rms")
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="ns_steps"):
            NativeMuon(p, ns_steps=bad)
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError, match="momentum"):
            NativeMuon(p, momentum=bad)
    with pytest.raises(ValueError, match="backend"):
        NativeMuon(p, _backend="eager")
    opt = NativeMuon([{"params": p, "group_name": "wd", "lr_scale": 0.5}], momentum=0.0)
    g = opt.param_groups[0]
    assert (g["lr"], g["weight_decay"], g["momentum"], g["nesterov"], g["ns_steps"], g["adjust_lr"], g["betas"], g["eps"], g["fallback_lr_scale"]) == \
        (0.02, 0.0, 0.0, True, 5, "match_rms_adamw", (0.9, 0.95), 1e-8, 1.0)
    assert g["group_name"] == "wd" and g["lr_scale"] == 0.5  # carried, never read
    sd = opt.state_dict()
    assert sd["param_groups"][0]["group_name"] == "wd"


def test_lr_scale_rule():
    from open_clip_amd.optim import muon_lr_scale
    for r, c in ((64, 64), (64, 192), (192, 64), (352, 588)):
        for mode in ("match_rms_adamw", "original"):
            assert muon_lr_scale(mode, r, c) == pytest.approx(U.lr_scale(mode, r, c), rel=1e-15)
    assert U.lr_scale("original", 192, 64) == pytest.approx(3 ** 0.5) and U.lr_scale("original", 64, 192) == 1.0
    assert U.lr_scale("match_rms_adamw", 64, 192) == pytest.approx(0.2 * 192 ** 0.5)


@pytest.mark.parametrize("shape", U.PARITY_SHAPES)
@pytest.mark.parametrize("kind", U.PARITY_KINDS)
def test_emulation_error_on_parity_inputs(shape, kind):
    """bf16 storage of X, A and B costs about one percent on full-rank inputs (0.8 - 1.4 % when the yardstick was written): the bound of the GPU
    parity tests, 2 * this + 2^-9, is therefore a few percent, and the oracle orthogonalises (singular values in Muon's band around 1)"""
    u = U.parity_input(shape, kind, seed=7).double()
    exact, emu = U.newton_schulz(u), U.newton_schulz(u, emulate=True)
    err = U.rel_err(emu, exact)
    s = torch.linalg.svdvals(exact)
    print(f"{shape} {kind}: emulation vs oracle {err:.4%}; oracle singular values in [{float(s.min()):.3f}, {float(s.max()):.3f}]")
    assert 0.002 <= err <= 0.02
    assert exact.shape == u.shape and float(s.max()) < 1.3


def test_rank_deficient_inputs_are_no_parity_inputs():
    """on a rank-4 input the directions with (numerically) zero singular value are amplified rounding noise: the emulation is tens of percent from the
    oracle, which is why tests/test_muon_gpu.py only asks for a finite update of the right spectral norm there"""
    u = U.low_rank_input((64, 192), 4, seed=3).double()
    err = U.rel_err(U.newton_schulz(u, emulate=True), U.newton_schulz(u))
    print(f"rank 4: emulation vs oracle {err:.1%}")
    assert err > 0.1


def test_scalar_recursion_under_bf16_storage():
    """s P / ||s P|| has k singular values 1 / sqrt(k); with bf16 rounding at every stored quantity (X, A and B) the recursion stays within 2.1 % of
    the float64 one for the k of the GPU test, which allows 2^-5 = 3.1 %.  (Not for every k: the map amplifies an early rounding where it is steep,
    and over k = 1 .. 257 the deviation reaches 7.7 %, at k = 4 -- printed below; the GPU test's k were chosen away from those.)"""
    dev = {k: abs(U.scalar_recursion(k, emulate=True) / U.scalar_recursion(k) - 1.0) for k in range(1, 258)}
    worst = max(dev, key=dev.get)
    print(f"k = 1, 7, 33, 64: {[f'{dev[k]:.3%}' for k in (1, 7, 33, 64)]}; worst over 1 .. 257: {dev[worst]:.3%} at k = {worst}")
    assert max(dev[k] for k in (1, 7, 33, 64)) <= 0.021
    # and the matrix oracle follows the scalar recursion exactly
    for k in (1, 7, 33, 64):
        p = U.partial_permutation((64, 192), k, seed=k, scale=0.37).double()
        x = U.newton_schulz(p)
        assert torch.equal(x == 0, p == 0)
        assert float((x[p != 0] - U.scalar_recursion(k)).abs().max()) <= 1e-6 * U.scalar_recursion(k)
