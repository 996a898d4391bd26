"""Times the CLIPA additions on one MI355X and writes profiles/clipa_step.json.

    python tools/clipa_step.py [--parent-bench FILE ...] [--this-bench FILE ...] [--note TEXT] [--out profiles/clipa_step.json]

One process.  Every figure is a MEDIAN of 20 launches / steps, each timed by its own pair of HIP events on an otherwise idle device, after warm-up.
A kernel launch is queued behind a filler (zeroing a 2 GiB buffer, ~0.4 ms) together with both of its events, so that the interval holds the kernel and
not the host's time to enqueue it (tens of microseconds here, as long as the kernels themselves); the filler also evicts the Infinity Cache.
  * kernels: ``ocn_mean_pool_fwd`` / ``ocn_mean_pool_bwd`` at ViT-L-14-CLIPA's own head (B = 256 images, T = 257 tokens, C = 1024) on an fp32 and on a bf16
    stream, and ``ocn_layernorm_fwd`` on the same matrix beside them: LayerNorm forward reads the same bytes AND writes them again in bf16, so neither
    pooling kernel should take longer than it.  Bytes are what the algorithm needs (computed from the shapes), the fraction is of the 6.3 TB/s copy
    rate (MI355X_MICROARCH: HBM3E stream copy).  The bf16 matrix (135 MB) fits the 256 MiB Infinity Cache and every launch re-reads the same buffer, so
    its rates could exceed what HBM alone gives, were it not for the filler in front of every launch.
  * one training step of ViT-L-14-CLIPA at batch 256, bf16 image stream (NativeClipLoss + NativeAdamW, no block recompute): step time, and the image
    tower alone (forward + backward of ``encode_image``).
  * ``--parent-bench`` / ``--this-bench``: files holding the JSON line plain ``python bench.py`` printed for the parent commit / for this tree in the same
    job on the same box, alternating; all values are recorded and this tree's headline is placed against the spread of the parent's own runs (the
    existing models run none of the new code).
Needs the GPU: there is no CPU fallback.
"""
import argparse
import json
import math
import os
import socket
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.3e12  # bytes / s
REPS = 20


def _median_ms(fn, warm=3, reps=REPS, filler=None):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if filler is not None:
            filler()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def _row(name, ms, bytes_):
    med, lo, hi = ms
    return {"kernel": name, "median_us": round(med * 1e3, 2), "min_us": round(lo * 1e3, 2), "max_us": round(hi * 1e3, 2), "bytes": int(bytes_),
            "tb_per_s": round(bytes_ / (med * 1e-3) / 1e12, 3), "fraction_of_copy_rate": round(bytes_ / (med * 1e-3) / COPY_RATE, 3)}


def kernels(dev):
    from open_clip_amd import ops
    B, T, C = 256, 257, 1024
    out = {"B": B, "T": T, "C": C, "rows": []}
    w, b = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    d = torch.randn(B, C, device=dev)
    big = torch.empty(1 << 31, dtype=torch.uint8, device=dev)
    fill = big.zero_
    for name, dtype, el in (("fp32 stream", torch.float32, 4), ("bf16 stream", torch.bfloat16, 2)):
        x = torch.randn(B * T, C, device=dev).to(dtype)
        rows = [
            _row(f"ocn_mean_pool_fwd [{name}]", _median_ms(lambda: ops.mean_pool_fwd(x, B, T, 1), filler=fill), B * (T - 1) * C * el + B * C * 4),
            # the backward as the head calls it: dx + dx16 on the fp32 stream, dx16 alone on the bf16 stream
            _row(f"ocn_mean_pool_bwd [{name}]", _median_ms(lambda: ops.mean_pool_bwd(d, B, T, 1, want_f32=dtype == torch.float32), filler=fill),
                 B * C * 4 + B * T * C * (6 if dtype == torch.float32 else 2)),
            _row(f"ocn_layernorm_fwd [{name}, bf16 result]", _median_ms(lambda: ops.layernorm_fwd(x, w, b), filler=fill), B * T * C * (el + 2) + B * T * 8),
        ]
        ln = rows[2]["median_us"]
        for r in rows[:2]:
            r["over_layernorm_fwd"] = round(r["median_us"] / ln, 3)
        out["rows"] += rows
        del x
    del big
    out["pool_slower_than_layernorm_fwd"] = [r["kernel"] for r in out["rows"] if r.get("over_layernorm_fwd", 0) > 1.0]
    return out


def step(dev):
    from open_clip_amd.configs import forward_gflops_per_pair, get_model_config
    from open_clip_amd.loss import NativeClipLoss
    from open_clip_amd.model import NativeCLIP
    from open_clip_amd.optim import NativeAdamW, param_groups_like_reference, weight_caches_of
    from open_clip_amd.synth import init_state_dict, synthetic_batch
    name, B = "ViT-L-14-CLIPA", 256
    cfg = get_model_config(name)
    torch.manual_seed(0)
    model = NativeCLIP(cfg["embed_dim"], cfg["vision_cfg"], cfg["text_cfg"], output_dict=True, image_stream="bf16")
    model.load_state_dict(init_state_dict(cfg, seed=0))
    model = model.to(dev).train()
    batch = synthetic_batch(cfg, B, seed=1234, device=dev)
    loss_fn = NativeClipLoss()
    opt = NativeAdamW(param_groups_like_reference(model, 0.2), lr=5e-8, betas=(0.9, 0.98), eps=1e-6, weight_caches=weight_caches_of(model))
    last = {}

    def one():
        opt.zero_grad(set_to_none=True)
        loss = loss_fn(**model(image=batch["image"], text=batch["text"]))
        loss.backward()
        opt.step()
        with torch.no_grad():
            model.logit_scale.clamp_(0, math.log(100))
        last["loss"] = loss

    def tower():
        for p in model.visual.parameters():
            p.grad = None
        f = model.encode_image(batch["image"], normalize=True)
        f.backward(torch.ones_like(f))

    s, t = _median_ms(one), _median_ms(tower)
    return {"model": name, "local_batch": B, "image_stream": "bf16", "image_tokens": 257, "text_tokens": cfg["text_cfg"]["context_length"], "pack_text": model.pack_text,
            "step_ms_median": round(s[0], 3), "step_ms_min_max": [round(s[1], 3), round(s[2], 3)], "pairs_per_s": round(B / s[0] * 1e3, 1),
            "image_tower_fwd_bwd_ms_median": round(t[0], 3), "image_tower_ms_min_max": [round(t[1], 3), round(t[2], 3)],
            "forward_gflops_per_pair": round(forward_gflops_per_pair(cfg), 2), "final_loss": float(last["loss"].detach())}


def bench_lines(paths):
    vals = []
    for p in paths or []:
        line = [ln for ln in open(p).read().splitlines() if ln.startswith("{")][-1]
        rec = json.loads(line)
        vals.append({"file": os.path.basename(p), "value": rec.get("value"), "unit": rec.get("unit"), "ms_per_step": rec.get("ms_per_step")})
    return vals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-bench", nargs="*")
    ap.add_argument("--this-bench", nargs="*")
    ap.add_argument("--note")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clipa_step.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X (no CPU fallback)"
    dev = torch.device("cuda:0")
    out = {"what": "CLIPA: pooling kernels beside LayerNorm forward, one ViT-L-14-CLIPA training step, bench.py of the parent and of this tree; method in tools/clipa_step.py",
           "box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
           "launches_or_steps_per_median": REPS, "copy_rate_bytes_per_s": COPY_RATE}
    out["kernels"] = kernels(dev)
    print(json.dumps(out["kernels"]), flush=True)
    if not a.skip_step:
        out["training_step"] = step(dev)
        print(json.dumps(out["training_step"]), flush=True)
    parent, this = bench_lines(a.parent_bench), bench_lines(a.this_bench)
    if parent and this:
        pv, tv = [r["value"] for r in parent], [r["value"] for r in this]
        out["bench_existing_models"] = {
            "parent_commit": parent, "this_tree": this, "order": "alternating, parent first, same job, same box",
            "parent_spread": [min(pv), max(pv)], "this_headline_median": sorted(tv)[len(tv) // 2],
            "this_headline_inside_parent_spread": min(pv) <= sorted(tv)[len(tv) // 2] <= max(pv)}
    if a.note:
        out["note"] = a.note
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
