"""Times the Muon optimizer step on one MI355X and writes profiles/muon_step.json.

    python tools/muon_step.py [--steps 20] [--out profiles/muon_step.json]

ViT-B-32 at the bench's configuration (local batch 4096, bf16 image stream).  One forward / backward leaves gradients in place; then the OPTIMIZER STEP
ALONE is timed for four configurations over the same parameters and gradients:
    adamw            NativeAdamW (one launch)
    muon_batched     NativeMuon, Newton-Schulz products as batched launches over equal-shape matrices (ocn_gemm_nt_batched)
    muon_per_matrix  NativeMuon, one matrix at a time through ocn_gemm_nt
    muon_torch       the same formula in plain torch: bf16 torch.bmm / baddbmm over matrices stacked by shape, foreach updates, fused torch AdamW for
                     the fallback parameters (the strongest eager statement; it refreshes no operand copies -- those casts would run in the next forward)
and the WHOLE TRAINING STEP with NativeAdamW and with NativeMuon (batched).
Method: HIP events around every single step; every configuration is warmed up (3 steps: every shape has run) before anything is timed; the configurations
are alternated inside one loop of ``--steps`` (>= 20) rounds, so drift hits all alike; median, min, max and the spread (max - min) / median of each are
recorded.  The Newton-Schulz loop alone is timed the same way for both backends; its rate is  sum 5 (4 m^2 n + 2 m^3) / time.
The learning rates are tiny (the weights barely move over the run).  Needs the GPU: there is no CPU fallback."""
import argparse
import json
import math
import os
import socket
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NS = (3.4445, -4.7750, 2.0315)


class TorchMuon:
    """the update of NativeMuon written in torch over the same groups (timing comparison only)"""

    def __init__(self, groups, lr, momentum=0.95, ns_steps=5, betas=(0.9, 0.95), eps=1e-8):
        from open_clip_amd.optim import muon_lr_scale, takes_muon
        self.lr, self.momentum, self.ns_steps = lr, momentum, ns_steps
        by_shape, fallback = {}, []
        for g in groups:
            for p in g["params"]:
                if p.grad is None:
                    continue
                if takes_muon(g, p):
                    by_shape.setdefault((p.shape[0], p.numel() // p.shape[0], g["weight_decay"]), []).append(p)
                else:
                    fallback.append({"params": [p], "weight_decay": g["weight_decay"]})
        self.stacks = [(ps, torch.zeros(len(ps), r, c, device=ps[0].device), 1.0 - lr * wd, -lr * muon_lr_scale("match_rms_adamw", r, c))
                       for (r, c, wd), ps in by_shape.items()]
        self.adamw = torch.optim.AdamW(fallback, lr=lr, betas=betas, eps=eps, fused=True)

    @torch.no_grad()
    def step(self):
        a, b, c = NS
        self.adamw.step()
        for ps, buf, decay, step in self.stacks:
            g = torch.stack([p.grad.reshape(p.shape[0], -1) for p in ps])
            buf.lerp_(g, 1.0 - self.momentum)
            u = g.lerp(buf, self.momentum)
            x = (u / (u.flatten(1).norm(dim=1).view(-1, 1, 1) + 1e-7)).bfloat16()
            tall = x.shape[1] > x.shape[2]
            x = x.transpose(1, 2).contiguous() if tall else x
            for _ in range(self.ns_steps):
                A = torch.bmm(x, x.transpose(1, 2))
                B = torch.baddbmm(A, A, A, beta=b, alpha=c)
                x = torch.baddbmm(x, B, x, beta=a, alpha=1.0)
            x = (x.transpose(1, 2) if tall else x).float()
            ws = [p.view(p.shape[0], -1) for p in ps]
            torch._foreach_mul_(ws, decay)
            torch._foreach_add_(ws, list(x.unbind(0)), alpha=step)


def _stats(samples):
    s = sorted(samples)
    med = s[len(s) // 2]
    return {"median_ms": round(med, 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4), "spread_percent": round(100 * (s[-1] - s[0]) / med, 2),
            "n": len(s)}


def _alternate(fns, rounds, warmup=3):
    """per-call device times (ms) of every fn in ``fns`` (name -> callable): warm-up of each, then ``rounds`` rounds that run each once"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    events = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "muon_step.json"))
    a = ap.parse_args()
    assert a.steps >= 20, "at least 20 timed steps"
    assert torch.cuda.is_available(), "needs the MI355X (no CPU fallback)"
    from open_clip_amd.configs import get_model_config
    from open_clip_amd.loss import NativeClipLoss
    from open_clip_amd.model import NativeCLIP
    from open_clip_amd.optim import NativeAdamW, NativeMuon, muon_param_groups, param_groups_like_reference, takes_muon, weight_caches_of
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
        loss = loss_fn(**model(image=batch["image"], text=batch["text"]))
        loss.backward()
        return loss

    fwd_bwd()
    caches = weight_caches_of(model)
    groups = muon_param_groups(model, 0.2)
    lr = 1e-7
    opts = {"adamw": NativeAdamW(param_groups_like_reference(model, 0.2), lr=5e-8, betas=(0.9, 0.98), eps=1e-6, weight_caches=caches),
            "muon_batched": NativeMuon(muon_param_groups(model, 0.2), lr=lr, weight_caches=caches, _backend="batched"),
            "muon_per_matrix": NativeMuon(muon_param_groups(model, 0.2), lr=lr, weight_caches=caches, _backend="per_matrix"),
            "muon_torch": TorchMuon(groups, lr=lr)}
    shapes = {}
    flop = 0
    for g in groups:
        for p in g["params"]:
            if takes_muon(g, p) and p.grad is not None:
                r, c = p.shape[0], p.numel() // p.shape[0]
                m, n = min(r, c), max(r, c)
                shapes[f"{r}x{c}"] = shapes.get(f"{r}x{c}", 0) + 1
                flop += 5 * (4 * m * m * n + 2 * m ** 3)
    out = {"what": "optimizer step alone (same parameters, same gradients) and whole training step; method in tools/muon_step.py",
           "box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
           "model": a.model, "local_batch": a.batch, "image_stream": "bf16", "timed_steps": a.steps, "warmup_steps": 3,
           "muon_matrices": shapes, "newton_schulz_tflop_per_step": round(flop / 1e12, 4)}
    t = _alternate({k: o.step for k, o in opts.items()}, a.steps)
    out["optimizer_step"] = {k: _stats(v) for k, v in t.items()}
    print(json.dumps(out["optimizer_step"]), flush=True)

    def ns_only(opt):
        plan = opt._plan
        return lambda: [opt._newton_schulz(ws, 5) for ws in plan["groups"]]

    t = _alternate({k: ns_only(opts[k]) for k in ("muon_batched", "muon_per_matrix")}, a.steps)
    out["newton_schulz_alone"] = {k: dict(_stats(v), tflops=round(flop / 1e12 / (sorted(v)[len(v) // 2] / 1e3), 1)) for k, v in t.items()}
    print(json.dumps(out["newton_schulz_alone"]), flush=True)
    del opts["muon_torch"], opts["muon_per_matrix"]

    def train_step(opt):
        def run():
            fwd_bwd()
            opt.step()
            with torch.no_grad():
                model.logit_scale.clamp_(0, math.log(100))
        return run

    t = _alternate({k: train_step(opts[k]) for k in ("adamw", "muon_batched")}, a.steps)
    out["training_step"] = {k: _stats(v) for k, v in t.items()}
    print(json.dumps(out["training_step"]), flush=True)
    st = out["optimizer_step"]
    b, pm, th = st["muon_batched"], st["muon_per_matrix"], st["muon_torch"]
    out["default_backend"] = "batched" if b["median_ms"] < pm["median_ms"] else "per_matrix"
    spread_ms = (b["max_ms"] - b["min_ms"]) + (th["max_ms"] - th["min_ms"])
    out["batched_vs_torch"] = {"batched_minus_torch_ms": round(b["median_ms"] - th["median_ms"], 4), "spread_of_the_two_ms": round(spread_ms, 4),
                               "batched_no_slower_than_torch_within_spread": bool(b["median_ms"] - th["median_ms"] <= spread_ms)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
