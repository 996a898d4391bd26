"""The recipe of tests/golden/small_patch_dropout.npz (tools/make_patch_dropout_golden.py), restated for the tests that read it: the fixture
stores checksums of its weights and image, both are regenerated here."""
import torch

from open_clip_amd.configs import get_model_config
from open_clip_amd.synth import init_state_dict, synthetic_batch
from tests.golden_util import load

NAME = "small_patch_dropout.npz"
CFG, PROB, BATCH, WEIGHT_SEED, BATCH_SEED = "small-test", 0.5, 6, 31, 131

_cache = {}


def inputs():
    """(cfg WITHOUT patch_dropout, state, batch) of the recipe: fp16-rounded weights and image, built once per process; reads no fixture"""
    if "inputs" not in _cache:
        cfg = get_model_config(CFG)
        state = {k: (v.half().float() if v.dtype.is_floating_point else v) for k, v in init_state_dict(cfg, seed=WEIGHT_SEED, perturb=True).items()}
        batch = synthetic_batch(cfg, BATCH, seed=BATCH_SEED)
        batch["image"] = batch["image"].half().float()
        _cache["inputs"] = (cfg, state, batch)
    return _cache["inputs"]


def fixture():
    """(golden dict, cfg WITHOUT patch_dropout, state, batch, keep int32 [6, 18] in the reference's topk order).  The regenerated weights, image and
    text must be the ones the fixture was made from: a checksum that does not match FAILS (a changed init_state_dict / synthetic_batch / recipe
    constant means the fixture has to be regenerated, not that the parity tests may be passed over)."""
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
    return g, cfg, state, batch, torch.from_numpy(g["keep"])
