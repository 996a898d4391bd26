"""Times the NAdamW optimizer step on one MI355X and writes profiles/nadamw_step.json.

    python tools/nadamw_step.py [--steps 20] [--out profiles/nadamw_step.json]

ViT-B-32 at the bench's configuration (local batch 4096, bf16 image stream).  One forward / backward leaves gradients in place; then the OPTIMIZER STEP
ALONE is timed for three configurations over the same parameters, gradients and groups (``create_optimizer``'s default two):
    adamw         NativeAdamW (one launch: the yardstick -- ocn_nadamw_multi moves the same bytes, 28 B per parameter plus the operand copies)
    nadamw        NativeNAdamW (one launch)
    torch_nadam   torch.optim.NAdam(decoupled_weight_decay=True) (foreach) followed by what the next forward then has to redo: the casts of every GEMM
                  weight -- an emptied ``_WeightCache`` + one ``cache.get`` per operand copy the model holds (a cache of the tool's own, so that the
                  model's copies, which the two native optimizers rewrite in place and whose identity is part of their plan, stay where they are)
Method (tools/muon_step.py): HIP events around every single step; every configuration is warmed up (3 steps) before anything is timed; the configurations
are alternated inside one loop of ``--steps`` (>= 20) rounds, so drift hits all alike; median, min, max and the spread (max - min) / median of each are
recorded, and ``nadamw_vs_adamw_percent`` = 100 * (nadamw / adamw - 1) of the medians (expected within +-5).
The learning rates are tiny (the weights barely move over the run).  Needs the GPU: there is no CPU fallback."""
import argparse
import json
import os
import socket
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.muon_step import _alternate, _stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--model", default="ViT-B-32")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nadamw_step.json"))
    a = ap.parse_args()
    assert a.steps >= 20, "at least 20 timed steps"
    assert torch.cuda.is_available(), "needs the MI355X (no CPU fallback)"
    from open_clip_amd import OptimizerCfg, create_optimizer
    from open_clip_amd.configs import get_model_config
    from open_clip_amd.loss import NativeClipLoss
    from open_clip_amd.model import NativeCLIP, _WeightCache
    from open_clip_amd.optim import weight_caches_of
    from open_clip_amd.synth import init_state_dict, synthetic_batch

    dev = torch.device("cuda:0")
    cfg = get_model_config(a.model)
    torch.manual_seed(0)
    model = NativeCLIP(cfg["embed_dim"], cfg["vision_cfg"], cfg["text_cfg"], output_dict=True, image_stream="bf16")
    model.load_state_dict(init_state_dict(cfg, seed=0))
    model = model.to(dev).train()
    batch = synthetic_batch(cfg, a.batch, seed=1234, device=dev)
    NativeClipLoss()(**model(image=batch["image"], text=batch["text"])).backward()

    ocfg = lambda opt: OptimizerCfg(opt=opt, lr=5e-8, weight_decay=0.2, beta1=0.9, beta2=0.98, eps=1e-6)
    adamw, nadamw = create_optimizer(model, ocfg("adamw")), create_optimizer(model, ocfg("nadamw"))
    torch_nadam = torch.optim.NAdam([{"params": g["params"], "weight_decay": g["weight_decay"]} for g in nadamw.param_groups], lr=5e-8, betas=(0.9, 0.98),
                                    eps=1e-6, decoupled_weight_decay=True)
    caches = weight_caches_of(model)
    cached = [(c, p, kind) for c in caches for p in model.parameters() for kind in ("n", "t") if c.peek(p, kind) is not None]

    scratch = _WeightCache()

    def torch_step():
        torch_nadam.step()
        scratch.clear()
        for _, p, kind in cached:
            scratch.get(p, kind)

    t = _alternate({"adamw": adamw.step, "nadamw": nadamw.step, "torch_nadam": torch_step}, a.steps)
    st = {k: _stats(v) for k, v in t.items()}
    n_params = sum(p.numel() for p in model.parameters())
    out = {"what": "optimizer step alone (same parameters, gradients and groups); method in tools/nadamw_step.py",
           "box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
           "model": a.model, "local_batch": a.batch, "image_stream": "bf16", "timed_steps": a.steps, "warmup_steps": 3,
           "parameters": n_params, "cached_operand_copies": len(cached), "optimizer_step": st,
           "nadamw_vs_adamw_percent": round(100 * (st["nadamw"]["median_ms"] / st["adamw"]["median_ms"] - 1), 2),
           "nadamw_within_5_percent_of_adamw": bool(abs(st["nadamw"]["median_ms"] / st["adamw"]["median_ms"] - 1) <= 0.05),
           "torch_nadam_over_nadamw": round(st["torch_nadam"]["median_ms"] / st["nadamw"]["median_ms"], 2)}
    print(json.dumps(out["optimizer_step"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out, "nadamw vs adamw", out["nadamw_vs_adamw_percent"], "%")


if __name__ == "__main__":
    main()
