"""Times the position-table resampling on one MI355X and writes profiles/pos_resample.json.

    python tools/pos_resample_step.py [--note TEXT] [--out profiles/pos_resample.json]

One process, an otherwise idle device.  Every figure is a MEDIAN of 20 launches / steps, each timed by its own pair of HIP events after warm-up.
  * kernels: ``ocn_pos_resample_fwd`` / ``ocn_pos_resample_bwd`` (bicubic, antialiased, one class-token row) at 7 x 7 -> 14 x 14 with C = 768 and at
    16 x 16 -> 24 x 24 with C = 1024 (ViT-L-14, 224 -> 336).  A launch is queued behind a filler (zeroing a 2 GiB buffer, ~0.4 ms) together with both of
    its events, so that the interval holds the kernel and not the host's time to enqueue it; the filler also evicts the Infinity Cache.  These are
    latency-bound launches of a few hundred workgroups: the bytes are recorded, a bandwidth fraction would say nothing.
  * the ViT-B-16 training step (NativeClipLoss + NativeAdamW, no block recompute) at local batch 1024 on 160 px images, two models in the same process,
    their steps ALTERNATED: ``dynamic`` = the 224 px model with ``dynamic_img_size``, which resamples its 14 x 14 + 1 table to 10 x 10 + 1 inside every
    step and carries the gradient back; ``twin`` = the model built with ``force_image_size=160``, the path the package had at that size before.  Medians
    of 20 steps each and each one's own min - max; whether the dynamic median lies inside the twin's spread is recorded, not required.
Needs the GPU: there is no CPU fallback.
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 20


def _timed(fn, filler=None):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if filler is not None:
        filler()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _stats(times):
    t = sorted(times)
    return t[len(t) // 2], t[0], t[-1]


def kernels(dev):
    from open_clip_amd import ops
    big = torch.empty(1 << 31, dtype=torch.uint8, device=dev)
    rows = []
    for src, dst, C in (((7, 7), (14, 14), 768), ((16, 16), (24, 24), 1024)):
        table = torch.randn(1 + src[0] * src[1], C, device=dev)
        dout = torch.randn(1 + dst[0] * dst[1], C, device=dev)
        for name, fn in (("ocn_pos_resample_fwd", lambda: ops.pos_resample(table, 1, src, dst, "bicubic", True)),
                         ("ocn_pos_resample_bwd", lambda: ops.pos_resample_bwd(dout, 1, src, dst, "bicubic", True))):
            for _ in range(3):
                fn()
            med, lo, hi = _stats([_timed(fn, big.zero_) for _ in range(REPS)])
            rows.append({"kernel": name, "grid": f"{src[0]}x{src[1]} -> {dst[0]}x{dst[1]}", "C": C, "median_us": round(med * 1e3, 2),
                         "min_us": round(lo * 1e3, 2), "max_us": round(hi * 1e3, 2), "bytes": int((table.numel() + dout.numel()) * 4)})
    del big
    return rows


def steps(dev, B=1024, size=160):
    from open_clip_amd.configs import get_model_config
    from open_clip_amd.loss import NativeClipLoss
    from open_clip_amd.model import create_model
    from open_clip_amd.optim import NativeAdamW, param_groups_like_reference, weight_caches_of
    from open_clip_amd.synth import synthetic_batch
    name = "ViT-B-16"
    cfg = get_model_config(name)
    batch = synthetic_batch(dict(cfg, vision_cfg=dict(cfg["vision_cfg"], image_size=size)), B, seed=1234, device=dev)
    loss_fn = NativeClipLoss()
    runs = {}
    for tag, kw in (("dynamic", {"dynamic_img_size": True}), ("twin", {"force_image_size": size})):
        torch.manual_seed(0)
        model = create_model(name, device=dev, output_dict=True, **kw).train()
        opt = NativeAdamW(param_groups_like_reference(model, 0.2), lr=5e-8, betas=(0.9, 0.98), eps=1e-6, weight_caches=weight_caches_of(model))

        def one(model=model, opt=opt):
            opt.zero_grad(set_to_none=True)
            loss = loss_fn(**model(image=batch["image"], text=batch["text"]))
            loss.backward()
            opt.step()
            with torch.no_grad():
                model.logit_scale.clamp_(0, math.log(100))
        runs[tag] = (model, one, [])
    for _, one, _ in runs.values():
        for _ in range(3):
            one()
    torch.cuda.synchronize()
    for _ in range(REPS):  # alternated: whatever drifts on the device reaches both alike
        for _, one, times in runs.values():
            times.append(_timed(one))
    out = {"model": name, "local_batch": B, "image_px": size, "configured_px": {t: list(m.visual.image_size) for t, (m, _, _) in runs.items()},
           "steps_per_median": REPS, "order": "alternating, dynamic first"}
    for tag, (_, _, times) in runs.items():
        med, lo, hi = _stats(times)
        out[tag] = {"step_ms_median": round(med, 3), "step_ms_min_max": [round(lo, 3), round(hi, 3)], "pairs_per_s": round(B / med * 1e3, 1)}
    d, t = out["dynamic"]["step_ms_median"], out["twin"]
    out["dynamic_over_twin"] = round(d / t["step_ms_median"], 4)
    out["dynamic_median_inside_twin_min_max"] = t["step_ms_min_max"][0] <= d <= t["step_ms_min_max"][1]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--note")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pos_resample.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X (no CPU fallback)"
    dev = torch.device("cuda:0")
    out = {"what": "position-table resampling: the two kernels alone, and the ViT-B-16 step at 160 px with dynamic_img_size against the force_image_size=160 "
                   "twin; method in tools/pos_resample_step.py",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
           "launches_or_steps_per_median": REPS}
    out["kernels"] = kernels(dev)
    print(json.dumps(out["kernels"]), flush=True)
    out["training_step"] = steps(dev, a.batch)
    print(json.dumps(out["training_step"]), flush=True)
    if a.note:
        out["note"] = a.note
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
