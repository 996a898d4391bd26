"""The recipe of tests/golden/tiny_clipa.npz (tools/make_clipa_golden.py), restated for the tests that read it -- the fixture stores checksums of its
weights and image, both are regenerated here -- and the CLIPA forward in elementary torch from oracle.clip_oracle's public pieces: image tower without
ln_pre, mean over the patch tokens, then ln_post (transformer.py:660, :783-785, :826-828); text tower without a mask, pooled at its last position
(:1649, :939-940)."""
import torch

from oracle import clip_oracle as O
from open_clip_amd.configs import get_model_config
from open_clip_amd.synth import init_state_dict, synthetic_batch
from tests.golden_util import load

NAME = "tiny_clipa.npz"
CFG, BATCH, WEIGHT_SEED, BATCH_SEED = "tiny-clipa-test", 6, 41, 141

_cache = {}


def inputs():
    """(cfg, state, batch) of the recipe: fp16-rounded weights and image, built once per process; reads no fixture"""
    if "inputs" not in _cache:
        cfg = get_model_config(CFG)
        state = {k: (v.half().float() if v.dtype.is_floating_point else v) for k, v in init_state_dict(cfg, seed=WEIGHT_SEED, perturb=True).items()}
        batch = synthetic_batch(cfg, BATCH, seed=BATCH_SEED)
        batch["image"] = batch["image"].half().float()
        _cache["inputs"] = (cfg, state, batch)
    return _cache["inputs"]


def fixture():
    """(golden dict, cfg, state, batch).  The regenerated weights, image and text must be the ones the fixture was made from: a checksum that does not
    match FAILS (a changed init_state_dict / synthetic_batch / recipe constant means the fixture has to be regenerated)."""
    cfg, state, batch = inputs()
    if "golden" not in _cache:
        _cache["golden"] = load(NAME)
    g = _cache["golden"]
    got, want = float(batch["image"].double().sum()), float(g["image_checksum"])
    assert abs(got - want) <= 1e-6 * batch["image"].numel() ** 0.5, f"image checksum {got!r} != fixture's {want!r}"
    names = [k[len("wsum/"):] for k in g if k.startswith("wsum/")]
    assert names and set(names) <= set(state)
    for k in names:
        got, want = float(state[k].double().sum()), float(g["wsum/" + k])
        assert abs(got - want) <= 1e-6 * state[k].numel() ** 0.5, f"weight checksum of {k}: {got!r} != fixture's {want!r}"
    assert bool((batch["text"].numpy() == g["text"]).all()), "text ids differ from the fixture's"
    return g, cfg, state, batch


def encode_image(image, p, cfg, keep=None, normalize=True):
    """patch dot product, class token and positions, (gather by ``keep`` [B, K] if given), NO ln_pre, transformer, mean over the patch tokens, ln_post
    on the pooled row, proj"""
    v = cfg["vision_cfg"]
    ps, width = v["patch_size"], v["width"]
    B, Cin, H, W = image.shape
    gh, gw = H // ps, W // ps
    w = p["visual.conv1.weight"].reshape(width, Cin * ps * ps)
    patches = image.reshape(B, Cin, gh, ps, gw, ps).permute(0, 2, 4, 1, 3, 5).reshape(B, gh * gw, Cin * ps * ps)
    x = torch.cat([p["visual.class_embedding"].reshape(1, 1, width).expand(B, 1, width), patches @ w.t()], dim=1) + p["visual.positional_embedding"]
    if keep is not None:
        x = torch.cat([x[:, :1], x[:, 1:][torch.arange(B)[:, None], keep.long()]], dim=1)
    x = O.transformer(x, p, "visual.transformer.", v["layers"], width // v.get("head_width", 64), causal=False)
    pooled = x[:, 1:].sum(dim=1) / (x.shape[1] - 1)
    pooled = O.layer_norm(pooled, p["visual.ln_post.weight"], p["visual.ln_post.bias"]) @ p["visual.proj"]
    return O.l2_normalize(pooled) if normalize else pooled


def encode_text(text, p, cfg, normalize=True):
    """token + positional embedding, transformer WITHOUT a mask, ln_final, the last position, text_projection"""
    t = cfg["text_cfg"]
    x = p["token_embedding.weight"][text] + p["positional_embedding"]
    x = O.transformer(x, p, "transformer.", t["layers"], t["heads"], causal=False)
    x = O.layer_norm(x, p["ln_final.weight"], p["ln_final.bias"])
    pooled = x[:, -1] @ p["text_projection"]
    return O.l2_normalize(pooled) if normalize else pooled
