"""Generates ``tests/golden/pos_resize.npz``: the REFERENCE's ``resize_pos_embed`` / ``resize_text_pos_embed`` (model.py:790-854) on seeded tables, and
one TRAINING step of the reference at another image size and context length than its weights were made for.  TEST INFRASTRUCTURE ONLY; run where the
reference can be imported (see oracle/ref_shim.py):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_pos_resize_golden.py

Recipe (restated in tests/pos_resample_util.py, which the tests use to regenerate every input: the fixture stores checksums only): 'small-test' (96 px,
patch 16: a 6 x 6 grid; context 77), weights = ``init_state_dict(cfg, seed=51, perturb=True)`` rounded to fp16.
(a) ``resize/<name>``: the reference's two functions on the state's own [6*6 + 1, 256] table -> 10 x 10 and -> 3 x 3 (bicubic, antialiased: the
    defaults), on its [77, 192] table -> 32 and on a seeded [32, 192] table -> 77 (linear: the defaults); ``refdev/<name>``: the reference's own largest
    deviation from the float64 restatement of tests/pos_resample_util.py (fp32 ATen against float64).
(b) the reference ``CLIP`` built at image 160 (10 x 10) and context 32, its state dict the seeded 96 / 77 one passed through those two functions;
    B = 6, image = ``synthetic_batch(cfg at 160 / 32, 6, seed=151)`` rounded to fp16; CPU, fp32, ``torch.use_deterministic_algorithms(True)``, through the
    reference's ``CLIPTask``.  ``out/*`` results, ``gnorm/ gsum/ grad/ gsample/`` gradients as oracle/make_golden.py packs them, and ``fullgrad/``: the
    whole gradient of the two position tables.
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.make_golden import GOLD, pack_grads  # noqa: E402
from oracle.ref_shim import import_reference  # noqa: E402
from tests import pos_resample_util as U  # noqa: E402

CHECKSUM_KEYS = ("visual.conv1.weight", "visual.positional_embedding", "positional_embedding", "token_embedding.weight", "visual.proj")


class _Shape:
    """what the reference's two functions read of a model: ``visual.grid_size`` and ``positional_embedding``"""

    def __init__(self, grid, num_pos, width):
        self.visual = type("V", (), {"grid_size": grid})()
        self.positional_embedding = torch.empty(num_pos, width)


def resizes(out):
    from open_clip.model import resize_pos_embed, resize_text_pos_embed
    for name, (_, prefix, src_hw, dst_hw, interpolation, antialias) in U.RESIZES.items():
        table = U.resize_source(name)
        if prefix:
            sd = {"visual.positional_embedding": table.clone()}
            resize_pos_embed(sd, _Shape(dst_hw, 1, table.shape[1]), interpolation, antialias)
            got = sd["visual.positional_embedding"]
        else:
            sd = {"positional_embedding": table.clone()}
            resize_text_pos_embed(sd, _Shape((1, 1), dst_hw[1], table.shape[1]), interpolation, antialias)
            got = sd["positional_embedding"]
        want = U.resample64(table.numpy(), prefix, src_hw, dst_hw, interpolation, antialias)
        assert tuple(got.shape) == want.shape and got.dtype == torch.float32
        out["resize/" + name] = got.numpy()
        out["refdev/" + name] = np.float64(np.abs(got.double().numpy() - want).max())
        print(name, tuple(got.shape), "reference max deviation from float64", float(out["refdev/" + name]))


def step(big, state, batch):
    """the reference at IMAGE / CONTEXT on the 96 / 77 state: its own resize functions, strict load, one training step"""
    from open_clip.model import CLIP, resize_pos_embed, resize_text_pos_embed
    from open_clip.task import CLIPTask
    v = {k: big["vision_cfg"][k] for k in ("image_size", "layers", "width", "patch_size") if k in big["vision_cfg"]}
    t = {k: big["text_cfg"][k] for k in ("context_length", "vocab_size", "width", "heads", "layers")}
    model = CLIP(embed_dim=big["embed_dim"], vision_cfg=v, text_cfg=t, output_dict=True)
    sd = {k: w.clone() for k, w in state.items()}
    resize_pos_embed(sd, model)
    resize_text_pos_embed(sd, model)
    assert tuple(sd["visual.positional_embedding"].shape) == (101, 256) and tuple(sd["positional_embedding"].shape) == (U.CONTEXT, 192)
    model.load_state_dict(sd, strict=True)
    model = model.float().train()
    seen = {}
    model.register_forward_hook(lambda m, a, o: seen.__setitem__("out", {k: w.detach().float().clone() for k, w in o.items()}))
    task = CLIPTask(model, rank=0, world_size=1)
    task.train()
    losses, _ = task({"image": batch["image"], "text": batch["text"]})
    losses["loss"].backward()
    return seen["out"], losses["loss"].detach().float(), {k: p.grad.detach().float() for k, p in model.named_parameters()}


def main():
    torch.manual_seed(0)
    torch.use_deterministic_algorithms(True)
    import_reference()
    cfg, big, state, batch, text32 = U.inputs()
    out = {"text": batch["text"].numpy(), "image_checksum": np.float64(batch["image"].double().sum()), "wsum/text32": np.float64(text32.double().sum())}
    for k in CHECKSUM_KEYS:
        out["wsum/" + k] = np.float64(state[k].double().sum())
    resizes(out)
    mo, loss, grads = step(big, state, batch)
    out["out/image_features"] = mo["image_features"].numpy()
    out["out/text_features"] = mo["text_features"].numpy()
    out["out/loss"] = loss.numpy()
    out["out/logit_scale_exp"] = mo["logit_scale"].numpy()
    pack_grads(out, grads)
    for k in ("visual.positional_embedding", "positional_embedding"):
        out["fullgrad/" + k] = grads[k].numpy()
    path = os.path.join(GOLD, U.NAME)
    np.savez_compressed(path, **out)
    print(U.NAME, "loss", float(loss), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
