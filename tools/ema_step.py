"""Times the model-EMA update on one MI355X and writes profiles/ema_step.json.

    python tools/ema_step.py [--steps 20] [--out profiles/ema_step.json]

ViT-B-32 at the bench's configuration (local batch 4096, bf16 image stream).  One forward / backward leaves gradients in place; then
    (a) native          ``NativeModelEma.update`` (one ocn_ema_lerp_multi launch over the whole model)
    (b) foreach_lerp_1/2/3  ``torch._foreach_lerp_`` over the same two tensor lists -- the YARDSTICK, three separately sampled groups: the widest gap
                        between their medians is what a difference between two medians of this measurement means at all
    (c) adamw           the NativeAdamW step alone (28 B per parameter plus the operand copies, for scale)
are timed alone, then (d) the whole training step without and with the update, then (e) the host time of one ``update`` call.
Method: HIP events around every single call; every configuration is warmed up (3 calls) before anything is timed; the configurations are alternated
inside one loop of ``--steps`` (>= 20) rounds, so drift hits all alike; median, min, max and the spread (max - min) / median of each are recorded.
For (a)-(c) every timed call is queued behind a few milliseconds of unrelated device work (a bf16 matmul), so that the host has issued the call before
the device reaches the first event: the interval is then device time, as inside a training step, where the host runs ahead.  (An ``update`` walks both
``state_dict()``s and revalidates ~600 addresses on the host, which takes longer than its kernel: from an idle device a single call is bound by (e).)
(e) is ``time.perf_counter`` around ``update`` calls that are NOT followed by a synchronise (the enqueue: table revalidation included), median of 50.
Bytes: 12 B per averaged element (8 read + 4 written); ``share_of_copy_rate`` = that over the 6.29 TB/s float4-copy rate, over the measured time.
``native_no_slower_than_foreach`` = median(a) - median(b) <= widest gap between the three (b) medians, (b) = the middle one of the three.
The learning rates are tiny (the weights barely move over the run).  Needs the GPU: there is no CPU fallback."""
import argparse
import json
import math
import os
import socket
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.muon_step import _alternate, _stats  # noqa: E402

COPY_RATE = 6.29e12  # B/s, float4 copy on the MI355X


def _alternate_queued(fns, rounds, filler, warmup=3):
    """``muon_step._alternate`` with ``filler()`` enqueued in front of every timed call (outside its events)"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    events = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            filler()
            e0.record()
            fn()
            e1.record()
            events[k].append((e0, e1))
        torch.cuda.synchronize()
    return {k: [e0.elapsed_time(e1) for e0, e1 in v] for k, v in events.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--model", default="ViT-B-32")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_step.json"))
    a = ap.parse_args()
    assert a.steps >= 20, "at least 20 timed steps"
    assert torch.cuda.is_available(), "needs the MI355X (no CPU fallback)"
    from open_clip_amd import NativeModelEma
    from open_clip_amd.configs import get_model_config
    from open_clip_amd.loss import NativeClipLoss
    from open_clip_amd.model import NativeCLIP
    from open_clip_amd.optim import NativeAdamW, param_groups_like_reference, weight_caches_of
    from open_clip_amd.synth import init_state_dict, synthetic_batch

    dev = torch.device("cuda:0")
    cfg = get_model_config(a.model)
    torch.manual_seed(0)
    model = NativeCLIP(cfg["embed_dim"], cfg["vision_cfg"], cfg["text_cfg"], output_dict=True, image_stream="bf16")
    model.load_state_dict(init_state_dict(cfg, seed=0))
    model = model.to(dev).train()
    batch = synthetic_batch(cfg, a.batch, seed=1234, device=dev)
    loss_fn = NativeClipLoss()

    def fwd_bwd():
        model.zero_grad(set_to_none=True)
        loss_fn(**model(image=batch["image"], text=batch["text"])).backward()

    fwd_bwd()
    adamw = NativeAdamW(param_groups_like_reference(model, 0.2), lr=5e-8, betas=(0.9, 0.98), eps=1e-6, weight_caches=weight_caches_of(model))
    ema = NativeModelEma(model, decay=0.9999)
    twin_list, model_list = list(ema.module.state_dict().values()), list(model.state_dict().values())
    assert all(t.dtype == torch.float32 for t in twin_list + model_list)
    weight = 1.0 - ema.get_decay()
    n_elem = sum(t.numel() for t in twin_list)
    n_bytes = 12 * n_elem
    floor_ms = n_bytes / COPY_RATE * 1e3

    fill_a = torch.randn(8192, 8192, device=dev).bfloat16()
    fill_out = torch.empty_like(fill_a)
    t = _alternate({"mm": lambda: torch.mm(fill_a, fill_a, out=fill_out)}, 5)
    mm_ms = sorted(t["mm"])[2]
    n_fill = max(1, math.ceil(5.0 / mm_ms))  # >= 5 ms of device work: more than the host needs to issue any of the timed calls

    def filler():
        for _ in range(n_fill):
            torch.mm(fill_a, fill_a, out=fill_out)

    fns = {"native": lambda: ema.update(model),
           "foreach_lerp_1": lambda: torch._foreach_lerp_(twin_list, model_list, weight),
           "foreach_lerp_2": lambda: torch._foreach_lerp_(twin_list, model_list, weight),
           "foreach_lerp_3": lambda: torch._foreach_lerp_(twin_list, model_list, weight),
           "adamw": adamw.step}
    t = _alternate_queued(fns, a.steps, filler)
    alone = {k: _stats(v) for k, v in t.items()}
    print(json.dumps(alone), flush=True)
    b_medians = sorted(alone[k]["median_ms"] for k in ("foreach_lerp_1", "foreach_lerp_2", "foreach_lerp_3"))
    b_med, b_gap = b_medians[1], b_medians[2] - b_medians[0]
    a_med = alone["native"]["median_ms"]

    def train_step(with_ema):
        def run():
            fwd_bwd()
            adamw.step()
            with torch.no_grad():
                model.logit_scale.clamp_(0, math.log(100))
            if with_ema:
                ema.update(model)
        return run

    t = _alternate({"without_ema": train_step(False), "with_ema": train_step(True)}, a.steps)
    training = {k: _stats(v) for k, v in t.items()}
    print(json.dumps(training), flush=True)

    host = []
    torch.cuda.synchronize()
    for _ in range(50):
        t0 = time.perf_counter()
        ema.update(model)
        host.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()

    out = {"what": "model-EMA update alone, against torch._foreach_lerp_ and the NativeAdamW step, and inside the training step; method in tools/ema_step.py",
           "box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
           "model": a.model, "local_batch": a.batch, "image_stream": "bf16", "timed_steps": a.steps, "warmup_steps": 3,
           "averaged_tensors": len(twin_list), "averaged_elements": n_elem, "bytes_per_update": n_bytes,
           "floor_ms_at_6.29_TB_per_s": round(floor_ms, 4), "filler_ms_in_front_of_each_timed_call": round(n_fill * mm_ms, 2),
           "update_alone": alone,
           "native_share_of_copy_rate": round(floor_ms / a_med, 3), "native_TB_per_s": round(n_bytes / (a_med * 1e-3) / 1e12, 3),
           "foreach_share_of_copy_rate": round(floor_ms / b_med, 3),
           "foreach_median_ms": b_med, "foreach_widest_gap_between_group_medians_ms": round(b_gap, 4),
           "native_minus_foreach_ms": round(a_med - b_med, 4), "native_no_slower_than_foreach": bool(a_med - b_med <= b_gap),
           "native_over_adamw": round(a_med / alone["adamw"]["median_ms"], 3),
           "training_step": training,
           "training_step_with_minus_without_ms": round(training["with_ema"]["median_ms"] - training["without_ema"]["median_ms"], 3),
           "update_host_ms": _stats(host)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out, "native", a_med, "ms, foreach", b_med, "ms (gap", round(b_gap, 4), "), share of the copy rate", out["native_share_of_copy_rate"])


if __name__ == "__main__":
    main()
