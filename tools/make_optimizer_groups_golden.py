"""Generates ``tests/golden/optimizer_groups.json``: the parameter groups the REFERENCE builds for its own ``CLIP`` -- names and numbers only -- which
tests/test_create_optimizer.py asks of ``open_clip_amd.create_optimizer`` on the ``NativeCLIP`` of the same configuration.  TEST INFRASTRUCTURE ONLY;
run where the reference can be imported (see oracle/ref_shim.py):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_optimizer_groups_golden.py

Models: the reference's ``CLIP`` from 'tiny-test' and from 'tiny-clipa-test' (no ln_pre: its image ``embeddings`` layer group differs).
Cases (``CASES``; the keys are ``OptimizerCfg`` fields, ``fallback`` marks the ones built with a fallback predicate):
    defaults | wd_exclude (two --wd-exclude patterns) | text_decay (0.75) | both_decays (text 0.75, image 0.65, pooler_in_head=False)
    fallback (predicate = open_clip_amd.optim.DEFAULT_FALLBACK) | fallback_both_decays
Builders: the reference's ``create_optimizer(model, OptimizerCfg(opt="adamw", lr=1e-3, ...))`` for the cases without a fallback predicate; with one (the
reference accepts it for timm's hybrid optimizers only) its ``wd_param_groups`` / ``layer_decay_param_groups`` with that predicate, a torch AdamW over the
groups and its ``assign_learning_rate`` -- the same three steps create_optimizer takes.
Layout: ``names/<model>`` the sorted parameter names; ``groups/<model>/<case>`` the groups in the optimizer's order, each with ``group_name``,
``weight_decay``, ``lr_scale`` (null without layer decay), ``use_fallback``, the ``lr`` after construction and ``params``: its members as ascending
indices into the model's name list."""
import fnmatch
import json
import os
import sys

import torch

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.ref_shim import import_reference  # noqa: E402
from open_clip_amd.configs import get_model_config  # noqa: E402
from open_clip_amd.optim import DEFAULT_FALLBACK  # noqa: E402

NAME = "optimizer_groups.json"
MODELS = ("tiny-test", "tiny-clipa-test")
LR, WEIGHT_DECAY = 1e-3, 0.2
BOTH = {"text_layer_decay": 0.75, "image_layer_decay": 0.65, "pooler_in_head": False}
CASES = {
    "defaults": {},
    "wd_exclude": {"wd_exclude_patterns": ["visual.proj", "*.c_fc.weight"]},
    "text_decay": {"text_layer_decay": 0.75},
    "both_decays": BOTH,
    "fallback": {"fallback": True},
    "fallback_both_decays": dict(BOTH, fallback=True),
}
VISION_KEYS = ("image_size", "layers", "width", "patch_size", "head_width", "mlp_ratio", "no_ln_pre", "pool_type", "final_ln_after_pool")
TEXT_KEYS = ("context_length", "vocab_size", "width", "heads", "layers", "pool_type", "no_causal_mask")


def reference_model(name):
    from open_clip.model import CLIP
    cfg = get_model_config(name)
    v = {k: cfg["vision_cfg"][k] for k in VISION_KEYS if k in cfg["vision_cfg"]}
    t = {k: cfg["text_cfg"][k] for k in TEXT_KEYS if k in cfg["text_cfg"]}
    return CLIP(embed_dim=cfg["embed_dim"], vision_cfg=v, text_cfg=t, output_dict=True)


def reference_optimizer(model, case):
    from open_clip_train import optim as R
    from open_clip_train.scheduler import assign_learning_rate
    fields = {k: v for k, v in case.items() if k != "fallback"}
    if not case.get("fallback"):
        return R.create_optimizer(model, R.OptimizerCfg(opt="adamw", lr=LR, weight_decay=WEIGHT_DECAY, **fields))
    fallback_fn = lambda name: any(fnmatch.fnmatchcase(name, pat) for pat in DEFAULT_FALLBACK)
    exclude_fn = R.make_wd_exclude(model, fields.get("wd_exclude_patterns"))
    if "text_layer_decay" in fields or "image_layer_decay" in fields:
        groups = R.layer_decay_param_groups(model, WEIGHT_DECAY, fields.get("text_layer_decay"), fields.get("image_layer_decay"), None,
                                            fields.get("pooler_in_head", True), exclude_fn, fallback_fn)
    else:
        groups = R.wd_param_groups(model, WEIGHT_DECAY, exclude_fn, fallback_fn)
    optimizer = torch.optim.AdamW(groups, lr=LR)
    assign_learning_rate(optimizer, LR)
    return optimizer


def describe(model, optimizer):
    index = {id(p): i for i, (_, p) in enumerate(sorted(model.named_parameters(), key=lambda np_: np_[0]))}
    return [{"group_name": g["group_name"], "weight_decay": g["weight_decay"], "lr_scale": g.get("lr_scale"), "use_fallback": bool(g.get("use_fallback", False)),
             "lr": g["lr"], "params": sorted(index[id(p)] for p in g["params"])} for g in optimizer.param_groups]


def main():
    import_reference()
    out = {"lr": LR, "weight_decay": WEIGHT_DECAY, "fallback_list": list(DEFAULT_FALLBACK), "cases": CASES, "names": {}, "groups": {}}
    for name in MODELS:
        model = reference_model(name)
        out["names"][name] = sorted(n for n, _ in model.named_parameters())
        out["groups"][name] = {key: describe(model, reference_optimizer(model, case)) for key, case in CASES.items()}
        print(name, {key: len(groups) for key, groups in out["groups"][name].items()})
    path = os.path.join(ROOT, "tests", "golden", NAME)
    with open(path, "w") as fh:
        json.dump(out, fh, sort_keys=True)
        fh.write("\n")
    print(NAME, "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
