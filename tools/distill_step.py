"""Times distillation on one MI355X and writes profiles/distill_step.json.

    python tools/distill_step.py [--steps 20] [--batch 4096] [--out profiles/distill_step.json]

(a) loss alone      forward + backward of ``NativeClipLoss`` against ``NativeDistillClipLoss`` (contrastive + distillation, two Functions) on unit
                    features: single process at [B, N, E] = [4096, 4096, 512], and the row-sharded global form at [4096, 32768, 512] with this process
                    playing rank 0 of 8 (the all-gather hands out 32768 prepared rows, the reduce-scatter keeps the first 4096 rows of its input, the
                    all-reduce is an identity: the kernels and their shapes are a rank's, the wire time is not in the figure).  Teacher width 768.
(b) row kernel      ``ocn_distill_rows`` alone at [4096, 4096] and [4096, 32768] beside its byte estimate: both fp32 matrices read twice and G written
                    once = 18 B per logit, at the 6.29 TB/s float4-copy rate.
(c) whole step      ViT-B-32 student (bf16 image stream, NativeAdamW) under a ViT-L-14 teacher: the student step without distillation, the teacher's
                    forward alone (eval, no_grad), the distillation step, and the same step with the reference's ATen ``DistillClipLoss`` on the native
                    models' features (when the reference's package is importable; else recorded as not measured).
Method (tools/ema_step.py's): HIP events around every call, every configuration warmed up (3 calls) before anything is timed, the configurations of a
group alternated inside one loop of ``--steps`` (>= 20) rounds; median, min, max and spread of each.  For (a) and (b) every timed call is queued behind
a few milliseconds of unrelated device work, so that the host has issued it before the device reaches the first event: the interval is device time, as
inside a training step where the host runs ahead.  The JSON is rewritten after every group.  Needs the GPU: there is no CPU fallback."""
import argparse
import json
import math
import os
import socket
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.ema_step import COPY_RATE, _alternate_queued  # noqa: E402
from tools.muon_step import _alternate, _stats  # noqa: E402

S_STUDENT, S_TEACHER = 14.2857, 20.0


def _unit_features(n, e, seed, dev):
    """unit image rows, and text rows correlated with their own image (a trained model's diagonal stands out)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    img = torch.nn.functional.normalize(torch.randn(n, e, device=dev, generator=g), dim=-1)
    txt = torch.nn.functional.normalize(0.6 * img + 0.8 * torch.nn.functional.normalize(torch.randn(n, e, device=dev, generator=g), dim=-1), dim=-1)
    return img.contiguous(), txt.contiguous()


class _RankZeroOfW:
    """the loss's collectives while this process plays rank 0 of W: see (a) in the module docstring"""

    def __init__(self, gathered):
        self.gathered = gathered  # [W*B, 2E + 2E_t]: student image | text | teacher image | text; the contrastive part asks for the leading 2E

    def all_gather(self, out, inp, comm=None):
        out.copy_(self.gathered[:, :out.shape[1]])

    def reduce_scatter(self, out, inp, comm=None):
        out.copy_(inp[:out.shape[0]])

    def all_reduce(self, t, comm=None):
        pass


def _loss_alone(dev, steps, filler, B, W, E, Et):
    import open_clip_amd.loss as L
    N = W * B
    I, T = _unit_features(N, E, 1, dev)
    DI, DT = _unit_features(N, Et, 2, dev)
    saved = (L._all_gather, L._reduce_scatter_sum, L._all_reduce_sum)
    if W > 1:
        coll = _RankZeroOfW(torch.cat([I, T, DI, DT], dim=1))
        L._all_gather, L._reduce_scatter_sum, L._all_reduce_sum = coll.all_gather, coll.reduce_scatter, coll.all_reduce
    kw = dict(rank=0, world_size=W, row_sharded=W > 1)
    clip, distill = L.NativeClipLoss(**kw), L.NativeDistillClipLoss(**kw)
    Ir, Tr = I[:B].clone().requires_grad_(True), T[:B].clone().requires_grad_(True)
    s, ds = torch.tensor(S_STUDENT, device=dev, requires_grad=True), torch.tensor(S_TEACHER, device=dev)
    DIr, DTr = DI[:B].contiguous(), DT[:B].contiguous()

    def run_clip():
        Ir.grad = Tr.grad = s.grad = None
        clip(Ir, Tr, s).backward()

    def run_distill():
        Ir.grad = Tr.grad = s.grad = None
        c, d = distill(Ir, Tr, s, DIr, DTr, ds)
        (c + d).backward()

    try:
        t = _alternate_queued({"clip_loss": run_clip, "distill_clip_loss": run_distill}, steps, filler)
    finally:
        L._all_gather, L._reduce_scatter_sum, L._all_reduce_sum = saved
    out = {k: _stats(v) for k, v in t.items()}
    out["shape_B_N_E_Et"] = [B, N, E, Et]
    out["distill_minus_clip_ms"] = round(out["distill_clip_loss"]["median_ms"] - out["clip_loss"]["median_ms"], 4)
    return out


def _row_kernel(dev, steps, filler, R, N):
    from open_clip_amd import ops
    g = torch.Generator(device=dev).manual_seed(R + N)
    student, teacher = torch.randn(R, N, device=dev, generator=g) * 4, torch.randn(R, N, device=dev, generator=g) * 6
    G = torch.empty(R, N, dtype=torch.bfloat16, device=dev)
    acc = torch.zeros(2, device=dev)
    t = _alternate_queued({"distill_rows": lambda: ops.distill_rows(student, teacher, G, N, 0.5 / R, 0.5 / R, 1.0, acc[0:1], acc[1:2])}, steps, filler)
    out = _stats(t["distill_rows"])
    n_bytes = R * N * 18  # 2 matrices x 2 reads x 4 B + 2 B of G
    floor_ms = n_bytes / COPY_RATE * 1e3
    out.update({"shape_R_N": [R, N], "bytes": n_bytes, "floor_ms_at_6.29_TB_per_s": round(floor_ms, 4),
                "share_of_byte_estimate": round(floor_ms / out["median_ms"], 3), "TB_per_s": round(n_bytes / (out["median_ms"] * 1e-3) / 1e12, 3)})
    return out


def _whole_step(dev, steps, batch_size, student_name, teacher_name):
    from open_clip_amd.configs import get_model_config
    from open_clip_amd.loss import NativeClipLoss, NativeDistillClipLoss
    from open_clip_amd.model import NativeCLIP
    from open_clip_amd.optim import NativeAdamW, param_groups_like_reference, weight_caches_of
    from open_clip_amd.synth import init_state_dict, synthetic_batch

    def build(name, seed, **kw):
        cfg = get_model_config(name)
        m = NativeCLIP(cfg["embed_dim"], cfg["vision_cfg"], cfg["text_cfg"], output_dict=True, **kw)
        m.load_state_dict(init_state_dict(cfg, seed=seed))
        return cfg, m.to(dev)

    cfg, student = build(student_name, 0, image_stream="bf16")
    tcfg, teacher = build(teacher_name, 1, image_stream="bf16")
    assert cfg["vision_cfg"]["image_size"] == tcfg["vision_cfg"]["image_size"] and cfg["text_cfg"]["vocab_size"] == tcfg["text_cfg"]["vocab_size"]
    student.train()
    teacher.eval()
    for p in teacher.parameters():
        p.requires_grad = False
    batch = synthetic_batch(cfg, batch_size, seed=1234, device=dev)
    clip, distill = NativeClipLoss(), NativeDistillClipLoss()
    aten = None
    try:
        from oracle.ref_shim import import_reference, reference_importable
        if reference_importable():
            import_reference()
            from open_clip.loss import DistillClipLoss
            aten = DistillClipLoss()
    except ImportError:
        pass
    student.zero_grad(set_to_none=True)
    clip(**student(image=batch["image"], text=batch["text"])).backward()
    adamw = NativeAdamW(param_groups_like_reference(student, 0.2), lr=5e-8, betas=(0.9, 0.98), eps=1e-6, weight_caches=weight_caches_of(student))

    def teacher_forward():
        with torch.no_grad():
            return teacher(image=batch["image"], text=batch["text"])

    def finish():
        adamw.step()
        with torch.no_grad():
            student.logit_scale.clamp_(0, math.log(100))

    def student_step():
        student.zero_grad(set_to_none=True)
        clip(**student(image=batch["image"], text=batch["text"])).backward()
        finish()

    def distill_step(loss_fn):
        def run():
            student.zero_grad(set_to_none=True)
            out = student(image=batch["image"], text=batch["text"])
            out.update({f"dist_{k}": v for k, v in teacher_forward().items()})
            losses = loss_fn(**out, output_dict=True)
            sum(losses.values()).backward()
            finish()
        return run

    fns = {"student_step_without_distillation": student_step, "teacher_forward_alone": teacher_forward, "distillation_step": distill_step(distill)}
    if aten is not None:
        fns["distillation_step_with_aten_DistillClipLoss"] = distill_step(aten)
    t = _alternate(fns, steps)
    out = {k: _stats(v) for k, v in t.items()}
    out.update({"student": student_name, "teacher": teacher_name, "local_batch": batch_size, "image_stream": "bf16",
                "teacher_embed_dim": tcfg["embed_dim"], "student_embed_dim": cfg["embed_dim"]})
    if aten is None:
        out["distillation_step_with_aten_DistillClipLoss"] = "not measured: the reference's open_clip package is not importable here"
    else:
        out["native_minus_aten_ms"] = round(out["distillation_step"]["median_ms"] - out["distillation_step_with_aten_DistillClipLoss"]["median_ms"], 3)
    out["distillation_minus_student_and_teacher_ms"] = round(out["distillation_step"]["median_ms"] - out["student_step_without_distillation"]["median_ms"]
                                                              - out["teacher_forward_alone"]["median_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--student", default="ViT-B-32")
    ap.add_argument("--teacher", default="ViT-L-14")
    ap.add_argument("--skip-whole-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distill_step.json"))
    a = ap.parse_args()
    assert a.steps >= 20, "at least 20 timed steps"
    assert torch.cuda.is_available(), "needs the MI355X (no CPU fallback)"
    dev = torch.device("cuda:0")
    out = {"what": "distillation: loss alone against NativeClipLoss, the row kernel against its byte estimate, the whole step; method in tools/distill_step.py",
           "box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
           "timed_steps": a.steps, "warmup_steps": 3}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")

    fill_a = torch.randn(8192, 8192, device=dev).bfloat16()
    fill_out = torch.empty_like(fill_a)
    mm_ms = sorted(_alternate({"mm": lambda: torch.mm(fill_a, fill_a, out=fill_out)}, 5)["mm"])[2]
    n_fill = max(1, math.ceil(5.0 / mm_ms))  # >= 5 ms of device work: more than the host needs to issue any of the calls timed behind it

    def filler():
        for _ in range(n_fill):
            torch.mm(fill_a, fill_a, out=fill_out)

    out["filler_ms_in_front_of_each_timed_call"] = round(n_fill * mm_ms, 2)
    out["row_kernel"] = {"4096x4096": _row_kernel(dev, a.steps, filler, 4096, 4096), "4096x32768": _row_kernel(dev, a.steps, filler, 4096, 32768)}
    print(json.dumps(out["row_kernel"]), flush=True)
    save()
    out["loss_alone"] = {"single_process": _loss_alone(dev, a.steps, filler, 4096, 1, 512, 768),
                         "row_sharded_rank_0_of_8": _loss_alone(dev, a.steps, filler, 4096, 8, 512, 768)}
    print(json.dumps(out["loss_alone"]), flush=True)
    save()
    del fill_a, fill_out
    torch.cuda.empty_cache()
    if not a.skip_whole_step:
        out["whole_step"] = _whole_step(dev, a.steps, a.batch, a.student, a.teacher)
        print(json.dumps(out["whole_step"]), flush=True)
        save()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
