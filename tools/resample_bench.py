"""Times the device-side resampler of ragged sources (ocn_resample_u8) on one MI355X and writes profiles/resample.json.

    python tools/resample_bench.py [--steps 20] [--out profiles/resample.json]

Four groups of figures, each the median of ``--steps`` (>= 20) alternated runs (method of tools/muon_step.py and tools/resized_crop_bench.py: HIP
events around every single call, every configuration warmed up before anything is timed, the configurations of one group alternated inside one
loop so drift hits all alike).  Figures only: no bar is set.
    eval          B = 4096 images of seeded ImageNet-like sizes (long side 400-600, short side 0.65-0.85 of it, both orientations; mean about
                  500 x 375), the validation transform 'shortest' -> 224: microseconds and GB/s over the bytes the algorithm needs, 3 * (the source
                  pixels under each output window + B * 224 * 224)
    fixed         256 x 256 sources, train plans equal to random_resized_crop_boxes' boxes: ocn_resample_u8 beside ocn_resized_crop_u8 on the same
                  pixels and boxes (the outputs are compared bit for bit before anything is timed)
    unaligned     the same number of pixels per image with Ws = 255, 254, 253 (row bytes = 1, 2, 3 mod 4: the dword-pair path) beside Ws = 256 (one
                  dword per tap), the new kernel on all four
    step          the ViT-B-32 training step (forward, ClipLoss, backward, AdamW) at local batch 4096 fed from pinned host memory through
                  DeviceBatchPipeline.ragged(train=True) -- submit() packs the 4096 images into the arena on the host, under the previous step's
                  compute -- and through the fixed-size pipeline DeviceBatchPipeline(crop_size=224), the same 256 x 256 sources either way
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


def imagenet_like_sizes(B, generator):
    long = torch.randint(400, 601, (B,), generator=generator)
    short = torch.round(long.double() * (0.65 + 0.2 * torch.rand(B, dtype=torch.float64, generator=generator))).long()
    landscape = torch.rand(B, generator=generator) < 0.7
    return torch.stack([torch.where(landscape, short, long), torch.where(landscape, long, short)], dim=1)


def packed_offsets(sizes, align=16):
    nbytes = (sizes[:, 0] * sizes[:, 1] * 3 + align - 1) // align * align
    offsets = torch.zeros(sizes.shape[0], dtype=torch.int64)
    offsets[1:] = nbytes.cumsum(0)[:-1]
    return offsets, int(nbytes.sum())


def needed_bytes(plan, Ho, Wo):
    """3 * (source pixels under the output window + output pixels): per axis the output covers min(m, R - max(o, 0)) resized indices = that many x n / R
    source positions (the filter's support beyond the window's edge is not counted)"""
    p = plan.double()
    rows = (torch.minimum(torch.tensor(float(Ho)), p[:, 6] - p[:, 8].clamp(min=0)) * p[:, 4] / p[:, 6]).clamp(max=p[:, 4])
    cols = (torch.minimum(torch.tensor(float(Wo)), p[:, 7] - p[:, 9].clamp(min=0)) * p[:, 5] / p[:, 7]).clamp(max=p[:, 5])
    return int(3 * ((rows * cols).sum() + plan.shape[0] * Ho * Wo))


def rate(stats, nbytes):
    return dict(stats, median_us=round(1e3 * stats["median_ms"], 1), bytes=nbytes, gb_per_s=round(nbytes / stats["median_ms"] / 1e6, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--model", default="ViT-B-32")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--no-step", action="store_true", help="kernels only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample.json"))
    a = ap.parse_args()
    assert a.steps >= 20, "at least 20 timed runs"
    assert torch.cuda.is_available(), "needs the MI355X (no CPU fallback)"
    from open_clip_amd import ops
    from open_clip_amd.configs import get_model_config
    from open_clip_amd.input_pipeline import DeviceBatchPipeline, check_resample_plan, eval_resample_plan, train_resample_plan
    from open_clip_amd.loss import NativeClipLoss
    from open_clip_amd.model import NativeCLIP
    from open_clip_amd.optim import NativeAdamW, param_groups_like_reference, weight_caches_of
    from open_clip_amd.synth import init_state_dict, synthetic_batch

    dev = torch.device("cuda:0")
    cfg = get_model_config(a.model)
    B, S, L = a.batch, cfg["vision_cfg"]["image_size"], cfg["text_cfg"]["context_length"]
    g = torch.Generator().manual_seed(7)
    out = {"what": "device-side resampling of ragged sources (ocn_resample_u8): the validation transform at ImageNet-like sizes, the new kernel beside "
                   "ocn_resized_crop_u8 on fixed-size sources, unaligned against aligned rows, the training step fed through the ragged pipeline; "
                   "method in tools/resample_bench.py",
           "box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
           "timed_runs": a.steps, "warmup_runs": 3}
    result = torch.empty((B, S, S, 3), dtype=torch.uint8, device=dev)

    # ---- (a) the validation transform on ragged sources ----
    sizes = imagenet_like_sizes(B, g)
    offsets, total = packed_offsets(sizes)
    plan = eval_resample_plan(sizes, S, "shortest")
    check_resample_plan(plan, offsets, total, S)
    arena = torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev)
    od, pd = offsets.to(dev), plan.to(dev)
    t = _alternate({"resample_u8": lambda: ops.resample_u8(arena, od, pd, S, out=result)}, a.steps)
    nb = needed_bytes(plan, S, S)
    out["eval"] = {"shape": f"B = {B}, sizes seeded (mean {float(sizes[:, 0].double().mean()):.0f} x {float(sizes[:, 1].double().mean()):.0f}, "
                            f"{int((sizes[:, 1] > sizes[:, 0]).sum())} landscape), shortest -> {S} x {S}", "arena_bytes": total,
                   "resample_u8": rate(_stats(t["resample_u8"]), nb)}
    print(json.dumps(out["eval"]), flush=True)
    del arena

    # ---- (b), (c) train plans: fixed-size sources beside the crop kernel, unaligned rows beside aligned ones ----
    cases, fns = {}, {}
    for Ws in (256, 255, 254, 253):
        Hs = round(256 * 256 / Ws)
        sz = torch.tensor([(Hs, Ws)] * B)
        offs, tot = packed_offsets(sz)
        pl = train_resample_plan(sz, S, generator=torch.Generator().manual_seed(8))
        check_resample_plan(pl, offs, tot, S)
        ar = torch.randint(0, 256, (tot,), dtype=torch.uint8, device=dev)
        cases[Ws] = (Hs, ar, offs.to(dev), pl.to(dev), needed_bytes(pl, S, S))
        fns[f"resample_u8_{Hs}x{Ws}"] = (lambda c: lambda: ops.resample_u8(c[1], c[2], c[3], S, out=result))(cases[Ws])
    Hs, ar, offs, pl, nb256 = cases[256]
    boxes = pl[:, 2:6].contiguous()
    src = ar.view(B, 256, 256, 3)
    same = torch.equal(ops.resample_u8(ar, offs, pl, S), ops.resized_crop_u8(src, boxes, S))
    fns["resized_crop_u8_256x256"] = lambda: ops.resized_crop_u8(src, boxes, S, out=result)
    t = _alternate(fns, a.steps)
    st = {k: _stats(v) for k, v in t.items()}
    out["fixed"] = {"shape": f"B = {B}, 256 x 256 -> {S} x {S}, train plans = random_resized_crop_boxes defaults", "outputs_bit_identical": same,
                    "resample_u8": rate(st["resample_u8_256x256"], nb256), "resized_crop_u8": rate(st["resized_crop_u8_256x256"], nb256),
                    "resample_over_resized_crop": round(st["resample_u8_256x256"]["median_ms"] / st["resized_crop_u8_256x256"]["median_ms"], 3)}
    out["unaligned"] = {"what": "row bytes mod 4 = 0 (one dword per tap) against 1, 2, 3 (the aligned dword pair, shifted)",
                        **{f"{cases[Ws][0]}x{Ws}_rowbytes_mod4_{(3 * Ws) % 4}": dict(rate(st[f"resample_u8_{cases[Ws][0]}x{Ws}"], cases[Ws][4]),
                                                                                  over_aligned=round(st[f"resample_u8_{cases[Ws][0]}x{Ws}"]["median_ms"]
                                                                                                     / st["resample_u8_256x256"]["median_ms"], 3))
                           for Ws in (256, 255, 254, 253)}}
    print(json.dumps(out["fixed"]), flush=True)
    print(json.dumps(out["unaligned"]), flush=True)

    # ---- (d) the training step through the ragged pipeline and through the fixed-size one ----
    if not a.no_step:
        src_host = src.cpu().pin_memory()
        del cases, fns, ar, src, result
        torch.cuda.empty_cache()
        torch.manual_seed(0)
        model = NativeCLIP(cfg["embed_dim"], cfg["vision_cfg"], cfg["text_cfg"], output_dict=True, image_stream="bf16")
        model.load_state_dict(init_state_dict(cfg, seed=0))
        model = model.to(dev).train()
        text_host = synthetic_batch(cfg, B, seed=1234)["text"].pin_memory()
        loss_fn = NativeClipLoss()
        opt = NativeAdamW(param_groups_like_reference(model, 0.2), lr=5e-8, betas=(0.9, 0.98), eps=1e-6, weight_caches=weight_caches_of(model))
        kw = dict(plan_text_vocab=cfg["text_cfg"]["vocab_size"] if model.pack_text else None, attn_buckets=model.attn_buckets)
        images = list(src_host)  # B views [256, 256, 3]: what a loader would hand over, one decoded image at a time
        pipes = {"ragged_train": (DeviceBatchPipeline.ragged(dev, B, (B, L), S, B * 256 * 256 * 3, train=True,
                                                             crop_generator=torch.Generator().manual_seed(8), **kw), images),
                 "fixed_crop": (DeviceBatchPipeline(dev, (B, 256, 256, 3), (B, L), crop_size=S, crop_generator=torch.Generator().manual_seed(8), **kw), src_host)}
        for pipe, pixels in pipes.values():
            pipe.submit(pixels, text_host)

        def step_of(name):
            pipe, pixels = pipes[name]

            def step():
                b = pipe.next()
                pipe.submit(pixels, text_host)  # the next batch's packing, plan and copy under this batch's compute
                opt.zero_grad(set_to_none=True)
                loss_fn(**model(image=b["image"], text=b["text"])).backward()
                pipe.release(b)
                opt.step()
            return step

        ts = _alternate({k: step_of(k) for k in pipes}, a.steps)
        sst = {k: _stats(v) for k, v in ts.items()}
        out["step"] = {"model": a.model, "local_batch": B, "image_stream": "bf16", "what": "forward + ClipLoss + backward + AdamW, 256 x 256 sources from "
                       "pinned host memory; ragged_train packs them into the arena on the host in submit()", **sst,
                       "ragged_minus_fixed_ms": round(sst["ragged_train"]["median_ms"] - sst["fixed_crop"]["median_ms"], 3),
                       "ragged_vs_fixed_percent": round(100 * (sst["ragged_train"]["median_ms"] / sst["fixed_crop"]["median_ms"] - 1), 2),
                       "pairs_per_s_ragged": round(B / sst["ragged_train"]["median_ms"] * 1e3)}
        print(json.dumps(out["step"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
