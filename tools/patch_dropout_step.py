"""Times the training step with patch dropout (transformer.py:17-58) on one MI355X and writes profiles/patch_dropout_step.json.

    python tools/patch_dropout_step.py [--parent-bench-json FILE] [--this-bench-json FILE] [--out profiles/patch_dropout_step.json]

One process, the bench's configuration (bench.py: ViT-B-32, local batch 4096, bf16 image stream, packed text, towers on two streams, NativeClipLoss +
NativeAdamW), at ``patch_dropout`` 0, 0.5 and 0.75; then ViT-L-14 at BASELINE config 4's batch (2048) with block recompute at 0 and 0.5.
Method: every shape is warmed up (3 steps) before it is timed; a step time is a host clock around ``--steps`` steps that end in a device
synchronise, taken ``--repeats`` times (the spread between those repeats is stated: it is the resolution of every comparison in the file);
tower and embed times are HIP events around that part alone on an otherwise idle device (forward + backward of ``encode_image``; the forward and
the backward of the image embed = patchify, patch GEMM, assemble, ln_pre).  The clock the GPU ran at (rocm-smi, read only) and the box are named.
``--parent-bench-json``: a file holding the JSON line bench.py of the PARENT commit printed on the same box in the same job; its ``ms_per_step``
is put beside the step at patch_dropout 0 (the default path is unchanged: the two should agree within the spread).  ``--this-bench-json``: the same
line from THIS tree's bench.py in that job -- bench against bench is the like-for-like pair (this tool's step loop is not the bench's).
Needs the GPU: there is no CPU fallback.
"""
import argparse
import json
import math
import os
import socket
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _clock():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=20).stdout
        card = next(iter(json.loads(out).values()))
        return {k: v for k, v in card.items() if "sclk" in k.lower() or "mclk" in k.lower()}
    except Exception as e:  # the reading is a courtesy, never a reason to lose the measurement
        return {"error": repr(e)[:200]}


def _events(fn, reps):
    """ms per call of ``fn`` (HIP events around ``reps`` calls on the current stream, after one warm call)"""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def measure(model_name, B, prob, steps, repeats, recompute, dev):
    from open_clip_amd import ops
    from open_clip_amd.configs import forward_gflops_per_pair, get_model_config, vision_tokens
    from open_clip_amd.loss import NativeClipLoss
    from open_clip_amd.model import NativeCLIP, _VisionEmbedFn
    from open_clip_amd.optim import NativeAdamW, param_groups_like_reference, weight_caches_of
    from open_clip_amd.synth import init_state_dict, synthetic_batch

    cfg = get_model_config(model_name)
    torch.manual_seed(0)
    model = NativeCLIP(cfg["embed_dim"], dict(cfg["vision_cfg"], patch_dropout=prob), cfg["text_cfg"], output_dict=True, image_stream="bf16")
    model.load_state_dict(init_state_dict(cfg, seed=0))
    model = model.to(dev).train()
    batch = synthetic_batch(cfg, B, seed=1234, device=dev)
    kept_blocks = None
    if recompute:
        rows_t = int((batch["text"].argmax(dim=-1) + 1).sum())
        free = torch.cuda.mem_get_info(dev)[0] - 16 * sum(p.numel() for p in model.parameters())
        kept_blocks = model.plan_grad_checkpointing(B, int(0.85 * free), text_rows=rows_t)
    loss_fn = NativeClipLoss()
    opt = NativeAdamW(param_groups_like_reference(model, 0.2), lr=5e-8, betas=(0.9, 0.98), eps=1e-6, weight_caches=weight_caches_of(model))

    def step():
        opt.zero_grad(set_to_none=True)
        loss = loss_fn(**model(image=batch["image"], text=batch["text"]))
        loss.backward()
        opt.step()
        with torch.no_grad():
            model.logit_scale.clamp_(0, math.log(100))
        return loss

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    samples = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = step()
        torch.cuda.synchronize()
        samples.append((time.perf_counter() - t0) / steps * 1e3)
    step_ms = sorted(samples)[len(samples) // 2]

    # image tower alone (forward + backward of encode_image, one stream, nothing beside it)
    def tower():
        for p in model.visual.parameters():
            p.grad = None
        f = model.encode_image(batch["image"], normalize=True)
        f.backward(torch.ones_like(f))

    tower_ms = _events(tower, 5)

    # image embed alone: patchify + patch GEMM + assemble + ln_pre, forward and backward apart
    v = model.visual
    ex = model._exec_options(True)
    G = v.grid_size[0] * v.grid_size[1]
    keep = inv = None
    if prob > 0:
        keep, inv = ops.patch_keep_plan(1, B, G, v.patch_dropout.num_keep(G), dev)
    args = (batch["image"], v.conv1.weight, v.class_embedding, v.positional_embedding, v.ln_pre.weight, v.ln_pre.bias, ex, v.patch_size[0], None, keep, inv)
    with torch.no_grad():
        embed_fwd_ms = _events(lambda: _VisionEmbedFn.apply(*args), 10)
    x0 = _VisionEmbedFn.apply(*args)
    gx = torch.ones_like(x0)
    both_ms = _events(lambda: _VisionEmbedFn.apply(*args).backward(gx), 10)
    plan_ms = _events(lambda: ops.patch_keep_plan(1, B, G, keep.shape[1], dev), 10) if prob > 0 else 0.0
    tokens = vision_tokens(cfg, prob)
    gf = forward_gflops_per_pair(cfg, prob)
    image_gf = _image_gflops(cfg, prob)
    rec = {"model": model_name, "local_batch": B, "patch_dropout": prob, "image_tokens": tokens, "block_recompute": bool(recompute),
           "kept_blocks_image_text": list(kept_blocks) if kept_blocks else None,
           "step_ms": round(step_ms, 3), "step_ms_repeats": [round(s, 3) for s in samples],
           "step_ms_spread_percent": round(100 * (max(samples) - min(samples)) / step_ms, 2),
           "pairs_per_s": round(B / step_ms * 1e3, 1),
           "image_tower_fwd_bwd_ms": round(tower_ms, 3), "image_embed_fwd_ms": round(embed_fwd_ms, 4), "image_embed_bwd_ms": round(both_ms - embed_fwd_ms, 4),
           "keep_plan_ms": round(plan_ms, 4),
           "executed_forward_gflops_per_pair": round(gf, 3), "executed_image_tower_forward_gflops_per_image": round(image_gf, 3),
           "image_tower_ms_per_executed_forward_tflop": round(tower_ms / (image_gf * B / 1e3), 4),
           "final_loss": float(loss.detach())}
    del model, opt, batch
    torch.cuda.empty_cache()
    return rec


def _image_gflops(cfg, prob):
    """executed forward GFLOPs of the image tower alone: the image terms of configs.forward_gflops_per_pair"""
    from open_clip_amd.configs import vision_tokens
    v, e = cfg["vision_cfg"], cfg["embed_dim"]
    lv, w = vision_tokens(cfg, prob), v["width"]
    r = int(w * v.get("mlp_ratio", 4.0)) / w
    macs = v["layers"] * lv * ((4 + 2 * r) * w * w + 2 * lv * w) + (lv - 1) * w * 3 * v["patch_size"] ** 2 + w * e
    return 2 * macs / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-bench-json")
    ap.add_argument("--this-bench-json")
    ap.add_argument("--skip-vitl", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patch_dropout_step.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X (no CPU fallback)"
    dev = torch.device("cuda:0")
    out = {"what": "training step with patch dropout in the image tower; method in tools/patch_dropout_step.py",
           "box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
           "clock_before": _clock(), "steps_per_repeat": a.steps, "repeats": a.repeats, "warmup_steps": 3, "runs": []}
    for prob in (0.0, 0.5, 0.75):
        out["runs"].append(measure("ViT-B-32", 4096, prob, a.steps, a.repeats, False, dev))
        print(json.dumps(out["runs"][-1]), flush=True)
    if not a.skip_vitl:
        for prob in (0.0, 0.5):
            out["runs"].append(measure("ViT-L-14", 2048, prob, max(2, a.steps // 3), a.repeats, True, dev))
            print(json.dumps(out["runs"][-1]), flush=True)
    out["clock_after"] = _clock()
    base = out["runs"][0]
    for key, path, what in (("parent_commit_bench", a.parent_bench_json, "bench.py of the parent commit"), ("this_commit_bench", a.this_bench_json, "bench.py of this tree")):
        if path and os.path.exists(path):
            line = [ln for ln in open(path).read().splitlines() if ln.startswith("{")][-1]
            rec = json.loads(line)
            out[key] = {"ms_per_step": rec.get("ms_per_step"), "value_pairs_per_s": rec.get("value"), "steps": rec.get("steps"),
                        "note": what + ", same box, same job; the default path is unchanged: the two bench lines, and runs[0].step_ms, agree within runs[0].step_ms_spread_percent"}
    out["ratios_vs_patch_dropout_0"] = [
        {"model": r["model"], "patch_dropout": r["patch_dropout"],
         "step": round(r["step_ms"] / b["step_ms"], 4), "image_tower": round(r["image_tower_fwd_bwd_ms"] / b["image_tower_fwd_bwd_ms"], 4),
         "image_embed_fwd": round(r["image_embed_fwd_ms"] / b["image_embed_fwd_ms"], 4), "image_embed_bwd": round(r["image_embed_bwd_ms"] / b["image_embed_bwd_ms"], 4),
         "image_tower_ms_per_executed_flop": round(r["image_tower_ms_per_executed_forward_tflop"] / b["image_tower_ms_per_executed_forward_tflop"], 4)}
        for r in out["runs"] for b in out["runs"] if b["model"] == r["model"] and b["patch_dropout"] == 0.0 and r["patch_dropout"] > 0]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
