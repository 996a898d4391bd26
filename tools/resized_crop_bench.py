"""Times the device-side RandomResizedCrop on one MI355X and writes profiles/resized_crop.json.

    python tools/resized_crop_bench.py [--steps 20] [--out profiles/resized_crop.json]

Three figures, each the median of ``--steps`` (>= 20) alternated runs (method of tools/muon_step.py: HIP events around every single call, every
configuration warmed up before anything is timed, the configurations of one group alternated inside one loop so drift hits all alike):
    kernel        ocn_resized_crop_u8 at B = 4096, 256 x 256 -> 224 x 224, boxes from random_resized_crop_boxes at its defaults: microseconds and the
                  achieved GB/s of the bytes it has to move, 3 * (sum of the box areas + B * 224 * 224)
    patchify      the ocn_patchify_u8 launch on the cropped batch, the yardstick: it reads the same kind of pixels and writes comparable bytes
    step          the ViT-B-32 training step (forward, ClipLoss, backward, AdamW) at local batch 4096 fed through DeviceBatchPipeline from pinned host
                  memory, once with 256 x 256 sources cropped on the device (crop_size=224) and once with pre-cropped 224 x 224 host pixels
Needs the GPU: there is no CPU fallback."""
import argparse
import json
import math
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
    ap.add_argument("--source", type=int, default=256)
    ap.add_argument("--no-step", action="store_true", help="kernel and patchify only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resized_crop.json"))
    a = ap.parse_args()
    assert a.steps >= 20, "at least 20 timed runs"
    assert torch.cuda.is_available(), "needs the MI355X (no CPU fallback)"
    from open_clip_amd import ops
    from open_clip_amd.configs import get_model_config
    from open_clip_amd.input_pipeline import DeviceBatchPipeline, random_resized_crop_boxes
    from open_clip_amd.loss import NativeClipLoss
    from open_clip_amd.model import NativeCLIP
    from open_clip_amd.optim import NativeAdamW, param_groups_like_reference, weight_caches_of
    from open_clip_amd.synth import init_state_dict, synthetic_batch

    dev = torch.device("cuda:0")
    cfg = get_model_config(a.model)
    B, Hs, S, P = a.batch, a.source, cfg["vision_cfg"]["image_size"], cfg["vision_cfg"]["patch_size"]
    L = cfg["text_cfg"]["context_length"]
    g = torch.Generator().manual_seed(7)
    src_host = torch.randint(0, 256, (B, Hs, Hs, 3), generator=g, dtype=torch.uint8).pin_memory()
    boxes_host = random_resized_crop_boxes(B, Hs, Hs, generator=g)

    # ---- the kernel beside the patchify launch ----
    src, boxes = src_host.to(dev), boxes_host.to(dev)
    cropped = torch.empty((B, S, S, 3), dtype=torch.uint8, device=dev)
    mean, std = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
    Kpad = (3 * P * P + 63) // 64 * 64
    t = _alternate({"resized_crop_u8": lambda: ops.resized_crop_u8(src, boxes, S, out=cropped),
                    "patchify_u8": lambda: ops.patchify_u8(cropped, P, Kpad, mean, std, True)}, a.steps)
    st = {k: _stats(v) for k, v in t.items()}
    crop_bytes = 3 * (int((boxes_host[:, 2].long() * boxes_host[:, 3].long()).sum()) + B * S * S)
    patch_bytes = B * S * S * 3 + B * (S // P) ** 2 * Kpad * 2
    kernel = {"shape": f"B = {B}, {Hs} x {Hs} -> {S} x {S}, boxes: random_resized_crop_boxes defaults (scale 0.9-1.0, ratio 3/4-4/3)",
              "mean_box_side": round(math.sqrt(crop_bytes / 3 / B - S * S), 1),
              "resized_crop_u8": dict(st["resized_crop_u8"], median_us=round(1e3 * st["resized_crop_u8"]["median_ms"], 1), bytes=crop_bytes,
                                      gb_per_s=round(crop_bytes / st["resized_crop_u8"]["median_ms"] / 1e6, 1)),
              "patchify_u8": dict(st["patchify_u8"], median_us=round(1e3 * st["patchify_u8"]["median_ms"], 1), bytes=patch_bytes,
                                  gb_per_s=round(patch_bytes / st["patchify_u8"]["median_ms"] / 1e6, 1)),
              "crop_over_patchify": round(st["resized_crop_u8"]["median_ms"] / st["patchify_u8"]["median_ms"], 2)}
    print(json.dumps(kernel), flush=True)
    out = {"what": "device-side RandomResizedCrop: the kernel, the patchify launch beside it, the training step fed with and without it; method in "
                   "tools/resized_crop_bench.py",
           "box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
           "timed_runs": a.steps, "warmup_runs": 3, "kernel": kernel}

    # ---- the training step through the pipeline ----
    if not a.no_step:
        pre_host = cropped.cpu().pin_memory()
        del src, cropped
        torch.manual_seed(0)
        model = NativeCLIP(cfg["embed_dim"], cfg["vision_cfg"], cfg["text_cfg"], output_dict=True, image_stream="bf16")
        model.load_state_dict(init_state_dict(cfg, seed=0))
        model = model.to(dev).train()
        text_host = synthetic_batch(cfg, B, seed=1234)["text"].pin_memory()
        loss_fn = NativeClipLoss()
        opt = NativeAdamW(param_groups_like_reference(model, 0.2), lr=5e-8, betas=(0.9, 0.98), eps=1e-6, weight_caches=weight_caches_of(model))
        kw = dict(plan_text_vocab=cfg["text_cfg"]["vocab_size"] if model.pack_text else None, attn_buckets=model.attn_buckets)
        pipes = {"device_crop": (DeviceBatchPipeline(dev, (B, Hs, Hs, 3), (B, L), crop_size=S, crop_generator=torch.Generator().manual_seed(8), **kw), src_host),
                 "host_precropped": (DeviceBatchPipeline(dev, (B, S, S, 3), (B, L), **kw), pre_host)}
        for pipe, pixels in pipes.values():
            pipe.submit(pixels, text_host)

        def step_of(name):
            pipe, pixels = pipes[name]

            def step():
                b = pipe.next()
                pipe.submit(pixels, text_host)  # the next batch's copy (and its boxes) under this batch's compute
                opt.zero_grad(set_to_none=True)
                loss_fn(**model(image=b["image"], text=b["text"])).backward()
                pipe.release(b)
                opt.step()
            return step

        ts = _alternate({k: step_of(k) for k in pipes}, a.steps)
        sst = {k: _stats(v) for k, v in ts.items()}
        out["step"] = {"model": a.model, "local_batch": B, "image_stream": "bf16", "what": "forward + ClipLoss + backward + AdamW, batch through "
                       "DeviceBatchPipeline from pinned host memory (the next batch's copy overlaps the step)", **sst,
                       "device_crop_minus_precropped_ms": round(sst["device_crop"]["median_ms"] - sst["host_precropped"]["median_ms"], 3),
                       "device_crop_vs_precropped_percent": round(100 * (sst["device_crop"]["median_ms"] / sst["host_precropped"]["median_ms"] - 1), 2),
                       "pairs_per_s_device_crop": round(B / sst["device_crop"]["median_ms"] * 1e3)}
        print(json.dumps(out["step"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
