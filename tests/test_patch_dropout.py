"""CPU: patch dropout of the image tower (reference transformer.py:17-58, :658, :804; model.py:48; factory.py:460-461) -- configuration plumbing,
the keep count, executed FLOPs, and the fixture tests/golden/small_patch_dropout.npz pinned by the CPU oracle's public pieces."""
import numpy as np
import pytest
import torch

from oracle import clip_oracle as O
from open_clip_amd.configs import forward_gflops_per_pair, get_model_config, vision_tokens
from tests.golden_util import check_grad, grad_keys
from tests.patch_dropout_util import fixture

TOL = 2e-5  # fp32 CPU vs fp32 CPU (tests/test_oracle_golden.py): summation order only


def _native(cfg, **vision):
    from open_clip_amd.model import NativeCLIP
    return NativeCLIP(cfg["embed_dim"], dict(cfg["vision_cfg"], **vision), cfg["text_cfg"])


def test_config_with_patch_dropout_constructs():
    from open_clip_amd.model import PatchDropout
    cfg = get_model_config("tiny-test")
    m = _native(cfg, patch_dropout=0.5)
    pd = m.visual.patch_dropout
    assert isinstance(pd, PatchDropout) and pd.prob == 0.5 and pd.exclude_first_token is True and pd.last_keep is None
    assert not list(pd.parameters()) and not list(pd.buffers())


@pytest.mark.parametrize("prob", [1.0, -0.1, 1.5])
def test_probability_outside_range_raises(prob):
    from open_clip_amd.model import PatchDropout
    with pytest.raises(ValueError):
        _native(get_model_config("tiny-test"), patch_dropout=prob)
    with pytest.raises(ValueError):
        PatchDropout(prob)


def test_create_model_force_patch_dropout():
    from open_clip_amd.model import create_model
    m = create_model("ViT-B-32", device="meta", force_patch_dropout=0.5)
    assert m.visual.patch_dropout.prob == 0.5
    assert isinstance(create_model("ViT-B-32", device="meta").visual.patch_dropout, torch.nn.Identity)
    # the override wins over a value in the config (factory.py:460-461)
    m = create_model("tiny-test", device="meta", vision_cfg=dict(get_model_config("tiny-test")["vision_cfg"], patch_dropout=0.25), force_patch_dropout=0.75)
    assert m.visual.patch_dropout.prob == 0.75


def test_state_dict_is_unchanged():
    cfg = get_model_config("tiny-test")
    base, zero, half = _native(cfg), _native(cfg, patch_dropout=0.0), _native(cfg, patch_dropout=0.5)
    assert isinstance(zero.visual.patch_dropout, torch.nn.Identity)  # transformer.py:658
    assert list(base.state_dict()) == list(zero.state_dict()) == list(half.state_dict())
    half.load_state_dict(base.state_dict(), strict=True)


@pytest.mark.parametrize("G,prob,K", [(49, 0.5, 24), (196, 0.75, 49), (256, 0.5, 128), (36, 0.5, 18), (36, 0.01, 35), (4, 0.9, 1)])
def test_num_keep_is_the_reference_formula(G, prob, K):
    from open_clip_amd.model import PatchDropout
    assert PatchDropout(prob).num_keep(G) == K == max(1, int(G * (1 - prob)))  # transformer.py:47-48


def test_live_tokens_and_memory_plan_follow_the_mode():
    cfg = get_model_config("small-test")
    m, full = _native(cfg, patch_dropout=0.5), _native(cfg)
    assert m.train().visual.live_tokens() == 19 and m.eval().visual.live_tokens() == 37 == full.train().visual.live_tokens()
    bv_train, bt = m.train().activation_bytes_per_block(8)
    bv_eval, _ = m.eval().activation_bytes_per_block(8)
    assert (bv_eval, bt) == full.activation_bytes_per_block(8) and bv_train * 37 == bv_eval * 19


def test_executed_flops():
    cfg = get_model_config("ViT-B-32")
    base = forward_gflops_per_pair(cfg)
    assert forward_gflops_per_pair(cfg, patch_dropout=None) == base == forward_gflops_per_pair(cfg, patch_dropout=0)
    assert forward_gflops_per_pair(cfg, patch_dropout=0.75) < forward_gflops_per_pair(cfg, patch_dropout=0.5) < base
    assert (vision_tokens(cfg), vision_tokens(cfg, 0.5), vision_tokens(cfg, 0.75), vision_tokens(cfg, 0)) == (50, 25, 13, 50)


def _dropped_encode_image(image, p, cfg, keep):
    """VisionTransformer.forward with PatchDropout active (transformer.py:793-808 with :48-56 at :804), from the oracle's public pieces:
    patch dot product, class token and positions, gather by ``keep``, ln_pre, transformer, ln_post, proj, normalize"""
    v = cfg["vision_cfg"]
    ps, width = v["patch_size"], v["width"]
    B, Cin, H, W = image.shape
    gh, gw = H // ps, W // ps
    w = p["visual.conv1.weight"].reshape(width, Cin * ps * ps)
    patches = image.reshape(B, Cin, gh, ps, gw, ps).permute(0, 2, 4, 1, 3, 5).reshape(B, gh * gw, Cin * ps * ps)
    x = torch.cat([p["visual.class_embedding"].reshape(1, 1, width).expand(B, 1, width), patches @ w.t()], dim=1) + p["visual.positional_embedding"]
    x = torch.cat([x[:, :1], x[:, 1:][torch.arange(B)[:, None], keep.long()]], dim=1)
    x = O.layer_norm(x, p["visual.ln_pre.weight"], p["visual.ln_pre.bias"])
    x = O.transformer(x, p, "visual.transformer.", v["layers"], width // v.get("head_width", 64), causal=False)
    x = O.layer_norm(x, p["visual.ln_post.weight"], p["visual.ln_post.bias"])
    return O.l2_normalize(x[:, 0] @ p["visual.proj"])


def test_fixture_is_pinned_by_the_oracle():
    g, cfg, state, batch, keep = fixture()
    assert g["keep"].dtype == np.int32 and g["keep"].shape == (6, 18) and float(g["patch_dropout"]) == 0.5
    assert all(len(set(r)) == 18 and min(r) >= 0 and max(r) < 36 for r in g["keep"].tolist())
    p = {k: v.detach().clone().float().requires_grad_(True) for k, v in state.items()}
    fi = _dropped_encode_image(batch["image"], p, cfg, keep)
    ft = O.encode_text(batch["text"], p, cfg)
    scale = p["logit_scale"].exp()
    loss = O.clip_loss(fi, ft, scale)
    loss.backward()
    d_i = float((fi.detach() - torch.from_numpy(g["out/image_features"])).abs().max())
    d_t = float((ft.detach() - torch.from_numpy(g["out/text_features"])).abs().max())
    d_l = abs(float(loss.detach()) - float(g["out/loss"]))
    worst = max(max(check_grad(g, k, p[k].grad, 0)) for k in grad_keys(g))
    print(f"features {d_i:.3e} / {d_t:.3e}  loss {d_l:.3e}  worst grad rel-L2 {worst:.3e}")
    assert d_i <= TOL and d_t <= TOL
    assert d_l <= TOL * max(1.0, abs(float(g["out/loss"])))
    assert abs(float(scale) - float(g["out/logit_scale_exp"])) <= TOL * float(g["out/logit_scale_exp"])
    assert set(grad_keys(g)) == set(p)
    for k in grad_keys(g):
        rel, nrel = check_grad(g, k, p[k].grad, 0)
        assert rel <= TOL and nrel <= TOL, (k, rel, nrel)
    # every patch no image kept has a zero positional gradient in the reference, too
    never = sorted(set(range(36)) - set(g["keep"].reshape(-1).tolist()))
    assert all(float(p["visual.positional_embedding"].grad[1 + n].abs().max()) == 0.0 for n in never)


@pytest.mark.parametrize("name,args", [
    # keep / inv = 0 means every patch in grid order: K must then be G.  Operands are non-null dummies: the refusal comes before any launch or read.
    ("ocn_embed_assemble_fwd", (64, 64, 64, 0, 64, 2, 36, 18, 128, 0)),            # K = 18, G = 36
    ("ocn_embed_assemble_bwd", (64, 0, 64, 64, 64, 2, 36, 18, 128, 0, 0)),         # K = 18, G = 36
    ("ocn_patchify", (64, 0, 0, 18, 64, 2, 96, 96, 16, 768, 0)),                   # K = 18, (96 / 16)^2 = 36
])
def test_dense_call_with_another_k_is_refused_on_the_host(name, args):
    """argument validation happens before any launch (tests/test_cabi.py): safe without a GPU"""
    from open_clip_amd import _lib, build
    build.build()
    with pytest.raises(RuntimeError, match=name + r": K=18 with G=36"):
        _lib.call(name, *args)
