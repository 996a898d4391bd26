"""CPU: the CLIPA model shape (reference model_configs/ViT-*-CLIPA*.json) -- registry, option check, state-dict layout against the reference's own
``CLIP``, the host-side argument checks of the pooling entry points, and the fixture tests/golden/tiny_clipa.npz pinned by an elementary-torch forward
(tests/clipa_util.py)."""
import pytest
import torch

from open_clip_amd.configs import get_model_config, list_models
from oracle.ref_shim import import_reference, reference_available
from tests import clipa_util as U

needs_reference = pytest.mark.skipif(not reference_available(), reason="reference tree not present")
TOL = 2e-5  # fp32 CPU vs fp32 CPU (tests/test_oracle_golden.py): summation order only
CLIPA = ("ViT-L-14-CLIPA", "ViT-L-14-CLIPA-336", "ViT-H-14-CLIPA", "ViT-H-14-CLIPA-336", "ViT-bigG-14-CLIPA", "ViT-bigG-14-CLIPA-336")


def test_fixture_is_pinned_by_the_elementary_forward():
    g, cfg, state, batch = U.fixture()
    with torch.no_grad():
        fi, ft = U.encode_image(batch["image"], state, cfg), U.encode_text(batch["text"], state, cfg)
    d_i = float((fi - torch.from_numpy(g["out/image_features"])).abs().max())
    d_t = float((ft - torch.from_numpy(g["out/text_features"])).abs().max())
    print(f"features {d_i:.3e} / {d_t:.3e}")
    assert d_i <= TOL and d_t <= TOL
    assert not any(k.startswith("visual.ln_pre") for k in state)
    # the last position of most captions is padding: this fixture does exercise a pooled padding row
    assert int((batch["text"][:, -1] == 0).sum()) >= 1


def test_synth_state_of_other_configs_is_unchanged_by_the_dropped_ln_pre():
    """a `no_ln_pre` config draws ln_pre's values and drops them: every other tensor equals the one of the same config WITH ln_pre"""
    from open_clip_amd.synth import init_state_dict
    cfg = get_model_config("tiny-clipa-test")
    with_ln = dict(cfg, vision_cfg={k: v for k, v in cfg["vision_cfg"].items() if k != "no_ln_pre"})
    a, b = init_state_dict(cfg, seed=3, perturb=True), init_state_dict(with_ln, seed=3, perturb=True)
    assert set(b) - set(a) == {"visual.ln_pre.weight", "visual.ln_pre.bias"} and not set(a) - set(b)
    assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("name", CLIPA + ("tiny-clipa-test",))
def test_registry(name):
    from open_clip_amd.model import _pooled_last_block_ok, create_model
    assert name in list_models()
    m = create_model(name, device="meta")
    assert m.pack_text is False and m.attn_mask is None and m.text_pool_type == "last" and m.text_eos_id is None
    m.pack_text = True  # whatever is assigned: the packed layout is invalid without a causal mask
    assert m.pack_text is False
    assert not any(k.startswith("visual.ln_pre") for k in m.state_dict())
    assert isinstance(m.visual.ln_pre, torch.nn.Identity) and m.visual.pool_type == "avg" and m.visual.final_ln_after_pool is True
    assert not _pooled_last_block_ok(m.visual)
    m.visual.pooled_last_block = True
    assert not _pooled_last_block_ok(m.visual)
    assert m.context_length == get_model_config(name)["text_cfg"]["context_length"]
    # lock / layer_groups with the parameter-less ln_pre
    groups = m.visual.layer_groups()
    assert groups[0][0] == "embeddings" and m.visual.ln_pre in groups[0][1]
    m.lock_image_tower(unlocked_groups=1)
    assert [n for n, p in m.visual.named_parameters() if p.requires_grad] == ["proj"]


def _native(vision=None, text=None):
    from open_clip_amd.model import NativeCLIP
    cfg = get_model_config("tiny-test")
    return NativeCLIP(cfg["embed_dim"], dict(cfg["vision_cfg"], **(vision or {})), dict(cfg["text_cfg"], **(text or {})))


@pytest.mark.parametrize("vision,text", [
    ({"no_ln_pre": True}, {}), ({"no_ln_pre": False}, {}),
    ({"final_ln_after_pool": True}, {}), ({"final_ln_after_pool": False, "pool_type": "tok"}, {}),
    ({"pool_type": "avg", "final_ln_after_pool": True}, {}), ({"pool_type": "avg", "final_ln_after_pool": True, "no_ln_pre": True}, {}),
    ({}, {"pool_type": "argmax"}), ({}, {"pool_type": "last"}), ({}, {"pool_type": "last", "no_causal_mask": True}), ({}, {"no_causal_mask": False}),
    ({}, {"hf_tokenizer_name": "bert-base-uncased", "tokenizer_kwargs": {"strip_sep_token": True}, "tokenizer_mode": "clips"}),
])
def test_accepted_options_construct(vision, text):
    m = _native(vision, text)
    assert isinstance(m.visual.ln_pre, torch.nn.Identity) == bool(vision.get("no_ln_pre"))
    assert m.visual.pool_type == vision.get("pool_type", "tok") and m.text_pool_type == text.get("pool_type", "argmax")
    assert (m.attn_mask is None) == bool(text.get("no_causal_mask"))
    # the packed text layout only behind a causal mask with argmax pooling
    assert m.pack_text == (m.text_pool_type == "argmax")


@pytest.mark.parametrize("vision,text,key", [
    ({"pool_type": "avg"}, {}, "pool_type"),
    ({"pool_type": "avg", "final_ln_after_pool": False}, {}, "pool_type"),
    ({"pool_type": "none"}, {}, "pool_type"),
    ({}, {"no_causal_mask": True}, "no_causal_mask"),
    ({}, {"no_causal_mask": True, "pool_type": "argmax"}, "no_causal_mask"),
    ({}, {"pool_type": "first"}, "pool_type"),
    ({}, {"pool_type": "eos", "eos_id": 2}, "pool_type|eos_id"),
    ({"ls_init_value": 1e-5}, {}, "ls_init_value"),
    ({"attentional_pool": True}, {}, "attentional_pool"),
    ({}, {"hf_model_name": "roberta-base"}, "hf_model_name"),
])
def test_rejected_options_name_their_key(vision, text, key):
    with pytest.raises(NotImplementedError, match=key):
        _native(vision, text)


@needs_reference
def test_state_dict_and_layer_groups_equal_the_reference():
    import_reference()
    from open_clip.model import CLIP
    from open_clip.transformer import _text_layer_groups
    from open_clip_amd.model import NativeCLIP
    cfg = get_model_config("tiny-clipa-test")
    v = {k: w for k, w in cfg["vision_cfg"].items()}
    ref = CLIP(embed_dim=cfg["embed_dim"], vision_cfg=v, text_cfg=dict(cfg["text_cfg"]), output_dict=True)
    native = NativeCLIP(cfg["embed_dim"], cfg["vision_cfg"], cfg["text_cfg"], output_dict=True)
    rs, ns = ref.state_dict(), native.state_dict()
    assert list(rs) == list(ns) or set(rs) == set(ns)
    assert {k: tuple(w.shape) for k, w in rs.items()} == {k: tuple(w.shape) for k, w in ns.items()}
    assert not any(k.startswith("visual.ln_pre") for k in rs)
    assert ref.attn_mask is None and native.attn_mask is None and ref.text_pool_type == native.text_pool_type == "last"
    assert ref.text_eos_id is None and native.text_eos_id is None
    # both directions, strict
    missing, unexpected = native.load_state_dict(rs, strict=True)
    assert not missing and not unexpected
    assert all(torch.equal(ns2, rs[k]) for k, ns2 in native.state_dict().items())
    state = U.inputs()[1]
    missing, unexpected = native.load_state_dict(state, strict=True)
    assert not missing and not unexpected
    missing, unexpected = ref.load_state_dict(native.state_dict(), strict=True)
    assert not missing and not unexpected
    assert all(torch.equal(w, state[k]) for k, w in ref.state_dict().items())

    def names_by_group(model, groups):
        ids = {id(p): n for n, p in model.named_parameters()}
        out = []
        for gname, members in groups:
            ps = []
            for m in members:
                ps += [m] if isinstance(m, torch.nn.Parameter) else list(m.parameters())
            out.append((gname, sorted(ids[id(p)] for p in ps)))
        return out
    assert names_by_group(native, native.visual.layer_groups()) == names_by_group(ref, ref.visual.layer_groups())
    assert names_by_group(native, native.text_layer_groups()) == names_by_group(ref, _text_layer_groups(ref))
    for k in (0, 1, 3):
        ref.lock_image_tower(unlocked_groups=k)
        native.lock_image_tower(unlocked_groups=k)
        assert {n for n, p in ref.named_parameters() if p.requires_grad} == {n for n, p in native.named_parameters() if p.requires_grad}, k


@needs_reference
def test_elementary_forward_equals_the_reference_model_with_keep_free_inputs():
    """the util's forward against the reference's own eval forward on the fixture's inputs (fp32 CPU: summation order only)"""
    import_reference()
    from open_clip.model import CLIP
    cfg, state, batch = U.inputs()
    ref = CLIP(embed_dim=cfg["embed_dim"], vision_cfg=dict(cfg["vision_cfg"]), text_cfg=dict(cfg["text_cfg"]), output_dict=True)
    ref.load_state_dict(state, strict=True)
    ref = ref.float().eval()
    with torch.no_grad():
        out = ref(image=batch["image"], text=batch["text"])
        fi, ft = U.encode_image(batch["image"], state, cfg), U.encode_text(batch["text"], state, cfg)
        # a token changed at a padding position moves the reference's text features: the tower is bidirectional
        text2 = batch["text"].clone()
        b = int((text2[:, -2] == 0).nonzero()[0])
        text2[b, -2] = 7
        moved = float((ref.encode_text(text2, normalize=True)[b] - out["text_features"][b]).abs().max())
    assert float((fi - out["image_features"]).abs().max()) <= TOL and float((ft - out["text_features"]).abs().max()) <= TOL
    assert moved > 1e-3


# operands are non-null dummies (64): every refusal comes before any launch or read
@pytest.mark.parametrize("name,args,msg", [
    ("ocn_mean_pool_fwd", (0, 0, 64, 2, 17, 1, 128, 0), "null operand"),
    ("ocn_mean_pool_fwd", (64, 0, 0, 2, 17, 1, 128, 0), "null operand"),
    ("ocn_mean_pool_fwd", (64, 0, 64, 2, 17, 17, 128, 0), r"skip=17 must satisfy 0 <= skip < T=17"),
    ("ocn_mean_pool_fwd", (64, 1, 64, 2, 17, -1, 128, 0), r"skip=-1 must satisfy"),
    ("ocn_mean_pool_fwd", (64, 0, 64, 2, 17, 1, 124, 0), r"C=124 must be a multiple of 8"),
    ("ocn_mean_pool_fwd", (64, 0, 64, 0, 17, 1, 128, 0), r"B=0"),
    ("ocn_mean_pool_bwd", (0, 64, 64, 2, 17, 1, 128, 0), "null operand"),
    ("ocn_mean_pool_bwd", (64, 0, 0, 2, 17, 1, 128, 0), "null operand"),
    ("ocn_mean_pool_bwd", (64, 64, 0, 2, 17, 18, 128, 0), r"skip=18 must satisfy 0 <= skip < T=17"),
    ("ocn_mean_pool_bwd", (64, 0, 64, 2, 17, 1, 132, 0), r"C=132 must be a multiple of 8"),
    ("ocn_cast_bf16_f32", (0, 64, 8, 0), "null operand"),
    ("ocn_cast_bf16_f32", (64, 0, 8, 0), "null operand"),
    ("ocn_cast_bf16_f32", (64, 64, 0, 0), r"n=0 must be positive"),
])
def test_pool_entry_points_refuse_bad_arguments_on_the_host(name, args, msg):
    """argument validation happens before any launch (tests/test_cabi.py): safe without a GPU"""
    from open_clip_amd import _lib, build
    build.build()
    with pytest.raises(RuntimeError, match=name + r" failed \(-1\): " + name + ": " + msg):
        _lib.call(name, *args)
