"""Times the device-side colour jitter / grayscale on one MI355X and writes profiles/color_jitter.json.

    python tools/color_jitter_bench.py [--steps 20] [--out profiles/color_jitter.json]

Each figure is the median of ``--steps`` (>= 20) alternated runs (method of tools/muon_step.py: HIP events around every single call, every
configuration warmed up before anything is timed, the configurations of one group alternated inside one loop so drift hits all alike):
    kernel        ops.color_jitter_u8 (both launches: the contrast means, then the apply pass) at B = 4096, 224 x 224, out of place, with
                    drawn              parameters from color_jitter_plan((0.4, 0.4, 0.4, 0.1), p = 0.8, grayscale 0.2)
                    drawn_no_contrast  the same plans with the contrast step taken out: every workgroup of the mean pass leaves at once, so
                                       drawn - drawn_no_contrast is what the mean pass costs (the contrast step itself is one fma per channel)
                    all_steps          every image runs all four steps
                    untouched          plan 0 everywhere: the apply pass as a copy -- the byte rate of its access pattern without arithmetic
                  microseconds and the achieved GB/s of the bytes each has to move (apply: 2 x B H W 3; mean: B H W 3 per image with a contrast step)
    behind_crop   ocn_resized_crop_u8 256 x 256 -> 224 x 224 alone, and followed by the jitter in place on its output (drawn parameters)
    step          the ViT-B-32 training step (forward, ClipLoss, backward, AdamW) at local batch 4096 fed through DeviceBatchPipeline from pinned host
                  memory with 256 x 256 sources, once with the device crop only and once with crop + jitter + grayscale
Needs the GPU: there is no CPU fallback."""
import argparse
import json
import os
import socket
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.muon_step import _alternate, _stats  # noqa: E402

COLOR_JITTER, JITTER_PROB, GRAY_PROB = (0.4, 0.4, 0.4, 0.1), 0.8, 0.2


def _without_contrast(plan):
    """the plans with every contrast code (2) taken out and the later steps moved down"""
    out = []
    for p in plan.tolist():
        codes = [c for c in ((p >> (3 * k)) & 7 for k in range(4)) if c != 2]
        out.append(sum(c << (3 * k) for k, c in enumerate(codes)) + (p & (1 << 12)))
    return torch.tensor(out, dtype=torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--model", default="ViT-B-32")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--source", type=int, default=256)
    ap.add_argument("--no-step", action="store_true", help="kernels only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "color_jitter.json"))
    a = ap.parse_args()
    assert a.steps >= 20, "at least 20 timed runs"
    assert torch.cuda.is_available(), "needs the MI355X (no CPU fallback)"
    from open_clip_amd import ops
    from open_clip_amd.configs import get_model_config
    from open_clip_amd.input_pipeline import DeviceBatchPipeline, color_jitter_plan, random_resized_crop_boxes
    from open_clip_amd.loss import NativeClipLoss
    from open_clip_amd.model import NativeCLIP
    from open_clip_amd.optim import NativeAdamW, param_groups_like_reference, weight_caches_of
    from open_clip_amd.synth import init_state_dict, synthetic_batch

    dev = torch.device("cuda:0")
    cfg = get_model_config(a.model)
    B, Hs, S = a.batch, a.source, cfg["vision_cfg"]["image_size"]
    L = cfg["text_cfg"]["context_length"]
    g = torch.Generator().manual_seed(7)
    src_host = torch.randint(0, 256, (B, Hs, Hs, 3), generator=g, dtype=torch.uint8).pin_memory()
    boxes = random_resized_crop_boxes(B, Hs, Hs, generator=g).to(dev)
    factors_host, plan_host = color_jitter_plan(B, COLOR_JITTER, JITTER_PROB, GRAY_PROB, generator=g)
    all_steps = color_jitter_plan(B, COLOR_JITTER, 1.0, GRAY_PROB, generator=g)
    with_contrast = float((((plan_host[:, None] >> (3 * torch.arange(4))[None, :]) & 7) == 2).any(dim=1).double().mean())

    # ---- the kernel alone ----
    src = src_host.to(dev)
    cropped = ops.resized_crop_u8(src, boxes, S)
    out = torch.empty_like(cropped)
    plans = {"drawn": (factors_host, plan_host), "drawn_no_contrast": (factors_host, _without_contrast(plan_host)), "all_steps": all_steps,
             "untouched": (torch.ones(B, 4), torch.zeros(B, dtype=torch.int32))}
    plans = {k: (f.to(dev), p.to(dev)) for k, (f, p) in plans.items()}

    def jitter_of(name):
        f, p = plans[name]
        return lambda: ops.color_jitter_u8(cropped, f, p, out=out)

    st = {k: _stats(v) for k, v in _alternate({k: jitter_of(k) for k in plans}, a.steps).items()}
    image_bytes = B * S * S * 3
    contrast_share = {"drawn": with_contrast, "drawn_no_contrast": 0.0, "all_steps": 1.0, "untouched": 0.0}
    kernel = {"shape": f"B = {B}, {S} x {S}, out of place; color_jitter = {COLOR_JITTER}, p = {JITTER_PROB}, grayscale {GRAY_PROB}",
              "images_with_a_contrast_step": round(with_contrast, 4)}
    for k, s in st.items():
        nbytes = int(image_bytes * (2 + contrast_share[k]))
        kernel[k] = dict(s, median_us=round(1e3 * s["median_ms"], 1), bytes=nbytes, gb_per_s=round(nbytes / s["median_ms"] / 1e6, 1))
    kernel["mean_pass_us"] = round(1e3 * (st["drawn"]["median_ms"] - st["drawn_no_contrast"]["median_ms"]), 1)
    kernel["estimate_from_bytes_us"] = round((2 + with_contrast) * image_bytes / 6.3e12 * 1e6, 1)  # at the 6.3 TB/s copy rate
    print(json.dumps(kernel), flush=True)

    # ---- behind the crop ----
    f, p = plans["drawn"]
    bt = {k: _stats(v) for k, v in _alternate({"crop": lambda: ops.resized_crop_u8(src, boxes, S, out=cropped),
                                               "crop_then_jitter": lambda: ops.color_jitter_u8(ops.resized_crop_u8(src, boxes, S, out=cropped), f, p, out=cropped)},
                                              a.steps).items()}
    behind = dict(bt, jitter_behind_crop_us=round(1e3 * (bt["crop_then_jitter"]["median_ms"] - bt["crop"]["median_ms"]), 1))
    print(json.dumps(behind), flush=True)
    res = {"what": "device-side colour jitter + grayscale: the kernel alone, behind the crop, and the training step fed with and without it; method in "
                   "tools/color_jitter_bench.py",
           "box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
           "timed_runs": a.steps, "warmup_runs": 3, "kernel": kernel, "behind_crop": behind}

    # ---- the training step through the pipeline ----
    if not a.no_step:
        del src, cropped, out
        torch.manual_seed(0)
        model = NativeCLIP(cfg["embed_dim"], cfg["vision_cfg"], cfg["text_cfg"], output_dict=True, image_stream="bf16")
        model.load_state_dict(init_state_dict(cfg, seed=0))
        model = model.to(dev).train()
        text_host = synthetic_batch(cfg, B, seed=1234)["text"].pin_memory()
        loss_fn = NativeClipLoss()
        opt = NativeAdamW(param_groups_like_reference(model, 0.2), lr=5e-8, betas=(0.9, 0.98), eps=1e-6, weight_caches=weight_caches_of(model))
        kw = dict(plan_text_vocab=cfg["text_cfg"]["vocab_size"] if model.pack_text else None, attn_buckets=model.attn_buckets, crop_size=S)
        pipes = {"crop_only": DeviceBatchPipeline(dev, (B, Hs, Hs, 3), (B, L), crop_generator=torch.Generator().manual_seed(8), **kw),
                 "crop_jitter": DeviceBatchPipeline(dev, (B, Hs, Hs, 3), (B, L), crop_generator=torch.Generator().manual_seed(8), color_jitter=COLOR_JITTER,
                                                    color_jitter_prob=JITTER_PROB, gray_scale_prob=GRAY_PROB,
                                                    jitter_generator=torch.Generator().manual_seed(9), **kw)}
        for pipe in pipes.values():
            pipe.submit(src_host, text_host)

        def step_of(name):
            pipe = pipes[name]

            def step():
                b = pipe.next()
                pipe.submit(src_host, text_host)  # the next batch's copy (and its parameters) under this batch's compute
                opt.zero_grad(set_to_none=True)
                loss_fn(**model(image=b["image"], text=b["text"])).backward()
                pipe.release(b)
                opt.step()
            return step

        sst = {k: _stats(v) for k, v in _alternate({k: step_of(k) for k in pipes}, a.steps).items()}
        res["step"] = {"model": a.model, "local_batch": B, "image_stream": "bf16", "what": "forward + ClipLoss + backward + AdamW, batch through "
                       "DeviceBatchPipeline from pinned host memory (the next batch's copy overlaps the step)", **sst,
                       "jitter_minus_crop_only_ms": round(sst["crop_jitter"]["median_ms"] - sst["crop_only"]["median_ms"], 3),
                       "jitter_vs_crop_only_percent": round(100 * (sst["crop_jitter"]["median_ms"] / sst["crop_only"]["median_ms"] - 1), 2),
                       "pairs_per_s_crop_jitter": round(B / sst["crop_jitter"]["median_ms"] * 1e3)}
        print(json.dumps(res["step"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
