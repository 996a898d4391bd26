"""Distillation on the MI355X: the row kernel ``ocn_distill_rows`` against float64, its exact cases and its reproducible form; ``NativeDistillClipLoss``
in a single process and with one process playing four ranks, against the float64 oracle of tests/distill_util.py evaluated on the bf16-rounded operands
the device multiplies; the reference's ``DistillCLIPTask`` around the native loss for one optimizer step.

Bounds.  Row kernel: those tests/test_kernels_gpu.py::test_loss_row_kernels applies to ``ocn_softmax_ce_rows`` (the same arithmetic): loss rel 1e-5,
G rel-L2 <= 4e-3 and every element within ``check(..., bf16_out=True)``'s bound, d/dscale within 1e-4 * sum|g_j l_j| * inv_logit_scale (against the sum
of magnitudes: the result itself is a difference).  Loss level: the feature gradients within TWICE the error of an ideal implementation that the test
computes itself -- the float64 G rounded once to bf16 and multiplied in float64 (the factor 2 covers __expf and the fp32 accumulation order); both
figures go to the report.  The loss value: the kernel's 1e-5 relative plus what the logits' fp32 accumulation can move it by (``_loss_tol``)."""
import math

import pytest
import torch

from oracle.ref_shim import import_reference, reference_importable
from tests.distill_util import distill_on_rounded_operands, distill_rows_f64, rel_l2
from tests.rank_emulation import Collectives, unit_features
from tests.test_kernels_gpu import _report, check

pytestmark = pytest.mark.gpu
F64 = torch.float64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def _strided(x, ld, dev):
    """the values of x [R, N] as a device view with row stride ld"""
    buf = torch.full((x.shape[0], ld), float("nan"), device=dev)
    buf[:, :x.shape[1]] = x.to(dev)
    return buf[:, :x.shape[1]]


def _run_rows(student, teacher, ls, gs, inv_s, det=False):
    from open_clip_amd import ops
    R, N = student.shape
    G = torch.zeros(R, (N + 63) // 64 * 64, dtype=torch.bfloat16, device=student.device)
    acc = torch.zeros(2, device=student.device)
    if det:
        rows = torch.full((R, 3), float("nan"), device=student.device)
        ops.distill_rows(student, teacher, G, N, ls, gs, inv_s, acc[0:1], acc[1:2], det_rows=rows)
        assert float(acc.abs().max()) == 0.0, "the reproducible form adds nothing atomically"
        return G, rows
    ops.distill_rows(student, teacher, G, N, ls, gs, inv_s, acc[0:1], acc[1:2])
    return G, acc


def _rows_oracle(student, teacher, ls, gs, inv_s):
    l, t = student.detach().cpu().to(F64), teacher.detach().cpu().to(F64)
    g = (torch.softmax(l, -1) - torch.softmax(t, -1)) * gs
    return float(distill_rows_f64(l, t).sum() * ls), g, float((g * l).sum() * inv_s), float((g * l).abs().sum() * inv_s)


# ---- 6. row kernel against float64 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,N", [(6, 6), (64, 200), (300, 300), (5, 2500)])
def test_distill_rows_against_float64(dev, R, N):
    """a row shorter than a wave, tails against 4, 64 and 256, several strides per thread; the teacher is a view whose row stride differs from the
    student's.  Two layouts: rows packed at stride N / N + 3 (for these N: scalar loads unless N % 4 == 0 and the stride is, too) and rows on the 16-byte
    grid at stride roundup(N, 4) / + 4, as the loss lays its logits out (16-byte loads, a guarded last chunk where N % 4 != 0)."""
    g = torch.Generator().manual_seed(1000 * R + N)
    s_host, t_host = torch.randn(R, N, generator=g) * 4, torch.randn(R, N, generator=g) * 6  # independent: p - q is not a cancellation
    ls, gs, inv_s = 0.5 / R, 0.5 / R, 1.0 / 14.3
    loss_ref, g_ref, ds_ref, ds_mag = _rows_oracle(s_host, t_host, ls, gs, inv_s)
    n4 = (N + 3) // 4 * 4
    for layout, ld_s, ld_t in (("packed", N, N + 3), ("aligned", n4, n4 + 4)):
        student, teacher = _strided(s_host, ld_s, dev), _strided(t_host, ld_t, dev)
        assert student.stride(0) != teacher.stride(0)
        G, acc = _run_rows(student, teacher, ls, gs, inv_s)
        tag = f"distill_rows[{R}x{N},{layout}]"
        check(f"{tag} loss", acc[0:1].cpu(), torch.tensor([loss_ref]), rel=1e-5)
        check(f"{tag} G", G[:, :N].cpu(), g_ref.float(), rel=4e-3, bf16_out=True)
        assert float(G[:, N:].float().abs().max() if G.shape[1] > N else 0.0) == 0.0, "columns beyond N are not written"
        err = abs(float(acc[1]) - ds_ref)
        _report(f"{tag + ' dscale':46s} err={err:.3e} bound={1e-4 * ds_mag:.3e} value={ds_ref:.6e}")
        assert err <= 1e-4 * ds_mag


# ---- 7. exact cases -------------------------------------------------------------------------------------------------------------------------------------
def test_distill_rows_teacher_equal_to_student_is_exactly_zero(dev):
    R, N, ls, gs = 37, 333, 0.5 / 37, 0.5 / 37
    g = torch.Generator().manual_seed(5)
    student = (torch.randn(R, N, generator=g) * 5).to(dev)
    p = torch.softmax(student.cpu().to(F64), -1)
    entropy = float(-(p * p.log()).sum() * ls)
    for name, teacher in (("the same tensor", student), ("a copy", student.clone()), ("a copy at another stride", _strided(student, N + 7, dev))):
        G, acc = _run_rows(student, teacher, ls, gs, 1.0)
        assert float(G.float().abs().max()) == 0.0 and float(acc[1]) == 0.0, f"teacher = {name}: p and q from one routine cancel exactly"
        assert abs(float(acc[0]) - entropy) <= 1e-5 * entropy, f"teacher = {name}: the loss is the rows' entropy"


def test_distill_rows_constant_rows(dev):
    R, N, ls = 9, 256, 0.25
    G, acc = _run_rows(torch.full((R, N), 3.0, device=dev), torch.full((R, N), -7.0, device=dev), ls, 0.5, 1.0)
    want = R * math.log(256.0) * ls
    assert abs(float(acc[0]) - want) <= 1e-5 * want and float(G.float().abs().max()) == 0.0 and float(acc[1]) == 0.0


def test_distill_rows_extreme_logits_stay_finite(dev):
    """a student row spanning +-300 (exp of the unshifted logits overflows fp32) and a teacher row with one entry 200 above the rest: q is exactly
    one-hot in fp32, so G = bf16(p * gs) off that column and bf16((p - 1) * gs) on it"""
    R, N, gs, col = 3, 1000, 0.5, 417
    student = torch.stack([torch.linspace(-300, 300, N), torch.linspace(300, -300, N), torch.linspace(-300, 300, N).roll(123)]).to(dev)
    teacher = torch.zeros(R, N, device=dev)
    teacher[:, col] = 200.0
    G, acc = _run_rows(student, teacher, 1.0, gs, 1.0)
    assert torch.isfinite(G.float()).all() and torch.isfinite(acc).all()
    p = torch.softmax(student.cpu().to(F64), -1)
    want = p * gs
    want[:, col] -= gs
    check("distill_rows[extreme] G", G[:, :N].cpu(), want.float(), rel=4e-3, bf16_out=True)
    off = torch.ones(N, dtype=torch.bool)
    off[col] = False
    assert float(G[:, :N].cpu()[:, off].float().min()) >= 0.0, "off the teacher's column q is exactly 0: G = bf16(p * gs) >= 0"
    l = student.cpu().to(F64)
    loss_ref = float((torch.logsumexp(l, -1) - l[:, col]).sum())
    assert abs(float(acc[0]) - loss_ref) <= 1e-5 * abs(loss_ref)


# ---- 8. det_rows form -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,N", [(64, 200), (5, 2500)])
def test_distill_rows_reproducible_form(dev, R, N):
    from open_clip_amd import ops
    g = torch.Generator().manual_seed(R + N)
    student, teacher = (torch.randn(R, N, generator=g) * 4).to(dev), (torch.randn(R, N, generator=g) * 6).to(dev)
    ls, gs, inv_s = 0.5 / R, 0.5 / R, 1.0 / 14.3
    G1, rows1 = _run_rows(student, teacher, ls, gs, inv_s, det=True)
    G2, rows2 = _run_rows(student, teacher, ls, gs, inv_s, det=True)
    assert torch.equal(rows1, rows2) and torch.equal(G1, G2) and float(rows1[:, 2].abs().max()) == 0.0
    tot = torch.zeros(3, device=dev)
    ops.colsum_f32(rows1, tot, deterministic=True)
    Ga, acc = _run_rows(student, teacher, ls, gs, inv_s)
    assert torch.equal(Ga, G1)
    for k, name in ((0, "loss"), (1, "dscale")):
        assert abs(float(tot[k]) - float(acc[k])) <= 1e-6 * abs(float(acc[k])), (name, float(tot[k]), float(acc[k]))


# ---- 9. loss level, single process ----------------------------------------------------------------------------------------------------------------------
S_STUDENT, S_TEACHER = 14.2857, 20.0


def _features(N, E, Et, dev):
    I, T = unit_features(N, E, 21, dev)
    DI, DT = unit_features(N, Et, 22, dev)
    return I, T, DI, DT


def _loss_tol(E, Et, loss):
    """The device's logits are fp32 sums of K bf16 products, the oracle's float64 sums of the same products: a logit moves by about
    sqrt(K) * 2^-24 * |s x| |y| <= sqrt(K) * 2^-24 * s (rounding errors of random sign).  D = lse(l) - sum q l has |dD/dl|_1 = |p - q|_1 <= 2 and
    |dD/dt|_1 = sum_j q_j |l_j - q.l| <= range(l) <= 2 s: so |error| <= 2 eps_l + 2 s eps_t, plus the kernel's own 1e-5 relative."""
    eps_l, eps_t = math.sqrt(E) * 2.0 ** -24 * S_STUDENT, math.sqrt(Et) * 2.0 ** -24 * S_TEACHER
    return 2 * eps_l + 2 * S_STUDENT * eps_t + 1e-5 * abs(loss)


def _judge(tag, got, want, ideal):
    """got within twice the ideal implementation's error, both against the float64 oracle"""
    e_got, e_ideal = rel_l2(got, want), rel_l2(ideal, want)
    _report(f"{tag:46s} rel_l2={e_got:.3e} ideal (G rounded once to bf16)={e_ideal:.3e} bound={2 * e_ideal:.3e}")
    assert e_got <= 2 * e_ideal, f"{tag}: rel_l2 {e_got:.3e} > 2 x {e_ideal:.3e}"


@pytest.mark.parametrize("B,E,Et", [(256, 128, 192), (24, 40, 72)])
def test_distill_loss_single_process(dev, B, E, Et):
    """(256, 128, 192): the contrastive part takes the fused one-pass cross-entropy; (24, 40, 72): padded K, no fused path"""
    import open_clip_amd.loss as L
    from open_clip_amd import ops
    I, T, DI, DT = _features(B, E, Et, dev)
    assert ops.fused_logits_ce_supported(B, B, (E + 63) // 64 * 64) == (B == 256)

    def run(loss_fn, distill):
        Ir, Tr, sr = I.clone().requires_grad_(True), T.clone().requires_grad_(True), torch.tensor(S_STUDENT, device=dev, requires_grad=True)
        out = loss_fn(Ir, Tr, sr, DI, DT, torch.tensor(S_TEACHER, device=dev)) if distill else (loss_fn(Ir, Tr, sr),)
        return [(o.detach(),) + torch.autograd.grad(o, (Ir, Tr, sr), retain_graph=True) for o in out]

    # the contrastive output is NativeClipLoss's, bit for bit (the reproducible form: the default one adds with atomics, in any order)
    (c_det, d_det), (c_clip,) = run(L.NativeDistillClipLoss(deterministic=True), True), run(L.NativeClipLoss(deterministic=True), False)
    assert all(torch.equal(a, b) for a, b in zip(c_det, c_clip)), "contrastive part differs from NativeClipLoss(deterministic=True)"
    (c, d), (c_clip,) = run(L.NativeDistillClipLoss(), True), run(L.NativeClipLoss(), False)
    assert all(rel_l2(a, b) <= 1e-5 for a, b in zip(c, c_clip)), "contrastive part differs from NativeClipLoss beyond the order of its atomic sums"
    want = distill_on_rounded_operands(I.cpu(), T.cpu(), S_STUDENT, DI.cpu(), DT.cpu(), S_TEACHER)
    ideal = distill_on_rounded_operands(I.cpu(), T.cpu(), S_STUDENT, DI.cpu(), DT.cpu(), S_TEACHER, ideal=True)
    for tag, (loss, dI, dT, ds) in ((f"distill_loss[{B},{E},{Et}]", d), (f"distill_loss[{B},{E},{Et},det]", d_det)):
        err = abs(float(loss) - want["loss"])
        _report(f"{tag + ' loss':46s} err={err:.3e} bound={_loss_tol(E, Et, want['loss']):.3e} value={want['loss']:.6f}")
        assert err <= _loss_tol(E, Et, want["loss"])
        _judge(f"{tag} dI", dI, want["dI_rows"] + want["dI_cols"], ideal["dI_rows"] + ideal["dI_cols"])
        _judge(f"{tag} dT", dT, want["dT_rows"] + want["dT_cols"], ideal["dT_rows"] + ideal["dT_cols"])
        err = abs(float(ds) - want["dscale"])
        _report(f"{tag + ' dscale':46s} err={err:.3e} bound={1e-4 * want['gl_abs'] / S_STUDENT:.3e} value={want['dscale']:.6e}")
        assert err <= 1e-4 * want["gl_abs"] / S_STUDENT


# ---- 10. rank emulation on the device -------------------------------------------------------------------------------------------------------------------
def test_distill_loss_rank_emulation_every_mode(dev, monkeypatch):
    """W = 4, B = 64, E = 128 (E_t = 192): one process plays rank 1 of each mode of ``_DistillLossFn``; what it hands to the reduce-scatter is recorded.
    Expected per mode, from the oracle restricted to the rank's rows: the gradient through its row operands, and through the column operands [N, E] --
    the reduce-scatter payload (row-sharded: in the forward; gather_with_grad: in the backward) or, in the redundant global form, part of every row."""
    import open_clip_amd.loss as L
    W, B, E, Et, r = 4, 64, 128, 192, 1
    N, lo, hi = W * B, r * B, (r + 1) * B
    I, T, DI, DT = _features(N, E, Et, dev)
    cpu = [x.cpu() for x in (I, T, DI, DT)]
    coll = Collectives(torch.cat([I, T, DI, DT], dim=1))  # ONE packed gather of [WB, 2E + 2E_t]
    monkeypatch.setattr(L, "_all_gather", coll.all_gather)
    monkeypatch.setattr(L, "_reduce_scatter_sum", coll.reduce_scatter)
    monkeypatch.setattr(L, "_all_reduce_sum", coll.all_reduce)
    modes = (("row_sharded", dict(local_loss=False, gather_with_grad=False, row_sharded=True), (lo, hi), 0.5 / N),
             ("local_gwg", dict(local_loss=True, gather_with_grad=True), (lo, hi), 0.5 / B),
             ("local_nograd", dict(local_loss=True, gather_with_grad=False), (lo, hi), 0.5 / B),
             ("global", dict(local_loss=False, gather_with_grad=False), (0, N), 0.5 / N),
             ("global_gwg", dict(local_loss=False, gather_with_grad=True), (0, N), 0.5 / N))
    for mode, kw, rows, weight in modes:
        coll.rs_inputs.clear()
        Ir, Tr = I[lo:hi].clone().requires_grad_(True), T[lo:hi].clone().requires_grad_(True)
        sr = torch.tensor(S_STUDENT, device=dev, requires_grad=True)
        loss = L._DistillLossFn.apply(Ir, Tr, sr, DI[lo:hi], DT[lo:hi], torch.tensor(S_TEACHER, device=dev), kw["local_loss"], kw["gather_with_grad"],
                                      r, W, kw.get("row_sharded", False), None, False)
        loss.backward()
        want, ideal = (distill_on_rounded_operands(cpu[0], cpu[1], S_STUDENT, cpu[2], cpu[3], S_TEACHER, rows=rows, weight=weight, ideal=i) for i in (False, True))
        tag = f"distill_emulated[{mode}]"
        err = abs(float(loss.detach()) - want["loss"])
        _report(f"{tag + ' loss':46s} err={err:.3e} bound={_loss_tol(E, Et, want['loss']):.3e} value={want['loss']:.6f}")
        assert err <= _loss_tol(E, Et, want["loss"])
        assert abs(float(sr.grad) - want["dscale"]) <= 1e-4 * want["gl_abs"] / S_STUDENT
        payload = (lambda o: torch.cat([o["dI_cols"], o["dT_cols"]], dim=1))
        if mode in ("row_sharded", "local_gwg", "local_nograd"):
            _judge(f"{tag} dI", Ir.grad, want["dI_rows"], ideal["dI_rows"])
            _judge(f"{tag} dT", Tr.grad, want["dT_rows"], ideal["dT_rows"])
            assert len(coll.rs_inputs) == (0 if mode == "local_nograd" else 1)
            if coll.rs_inputs:
                _judge(f"{tag} reduce-scatter payload", coll.rs_inputs[0], payload(want), payload(ideal))
        elif mode == "global":
            assert not coll.rs_inputs
            _judge(f"{tag} dI", Ir.grad, (want["dI_rows"] + want["dI_cols"])[lo:hi], (ideal["dI_rows"] + ideal["dI_cols"])[lo:hi])
            _judge(f"{tag} dT", Tr.grad, (want["dT_rows"] + want["dT_cols"])[lo:hi], (ideal["dT_rows"] + ideal["dT_cols"])[lo:hi])
        else:
            assert len(coll.rs_inputs) == 1 and float(Ir.grad.abs().max()) == 0.0 and float(Tr.grad.abs().max()) == 0.0
            whole = (lambda o: torch.cat([o["dI_rows"] + o["dI_cols"], o["dT_rows"] + o["dT_cols"]], dim=1))
            _judge(f"{tag} reduce-scatter payload", coll.rs_inputs[0], whole(want), whole(ideal))


# ---- 11. deterministic=True -----------------------------------------------------------------------------------------------------------------------------
def test_distill_loss_deterministic_is_bit_reproducible(dev):
    import open_clip_amd.loss as L
    I, T, DI, DT = _features(256, 128, 192, dev)
    runs = []
    for _ in range(2):
        Ir, Tr, sr = I.clone().requires_grad_(True), T.clone().requires_grad_(True), torch.tensor(S_STUDENT, device=dev, requires_grad=True)
        c, d = L.NativeDistillClipLoss(deterministic=True)(Ir, Tr, sr, DI, DT, torch.tensor(S_TEACHER, device=dev))
        (c + 0.5 * d).backward()
        runs.append((c.detach(), d.detach(), Ir.grad, Tr.grad, sr.grad))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


# ---- 12. the reference's task ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not reference_importable(), reason="reference packages not available")
def test_distill_task_steps_the_student_and_leaves_the_teacher(dev):
    import types
    import_reference()
    import open_clip_amd
    from open_clip.task import DistillCLIPTask
    from open_clip_amd.configs import get_model_config
    from open_clip_amd.optim import NativeAdamW, param_groups_like_reference, weight_caches_of
    from open_clip_amd.synth import init_state_dict, synthetic_batch
    from tests.test_model_gpu import _build
    cfg = get_model_config("tiny-test")
    student, teacher = _build(cfg, init_state_dict(cfg, seed=71, perturb=True)), _build(cfg, init_state_dict(cfg, seed=72, perturb=True))
    batch = {k: v.cuda() for k, v in synthetic_batch(cfg, 8, seed=600).items()}
    args = types.SimpleNamespace(model="tiny-test", distill=True, siglip=False, local_loss=False, gather_with_grad=False, rank=0, world_size=1)
    task = open_clip_amd.create_task(args, student, dist_model=teacher, device=dev, verbose=False)
    assert type(task) is DistillCLIPTask and type(task.loss) is open_clip_amd.NativeDistillClipLoss
    task.train()
    assert student.training and not teacher.training
    before = [p.detach().clone() for p in teacher.parameters()]
    losses, _ = task.training_forward(batch)
    assert {"contrastive_loss", "distill_loss", "loss"} <= set(losses)
    assert torch.equal(losses["loss"], losses["contrastive_loss"] + losses["distill_loss"])
    losses["loss"].backward()
    out = student(**batch)
    with torch.no_grad():
        t_out = teacher(**batch)
    direct = task.loss(**out, **{f"dist_{k}": v for k, v in t_out.items()}, output_dict=True)
    for k in ("contrastive_loss", "distill_loss"):
        assert abs(float(losses[k]) - float(direct[k])) <= 1e-6 * max(1.0, abs(float(direct[k]))), k
    assert float(losses["distill_loss"]) > 0.0
    assert all(torch.isfinite(p.grad).all() for p in student.parameters()), "every student parameter has a finite gradient"
    assert all(p.grad is None for p in teacher.parameters())
    NativeAdamW(param_groups_like_reference(student, 0.2), lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_caches=weight_caches_of(student)).step()
    torch.cuda.synchronize()
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, teacher.parameters())), "the optimizer step leaves the teacher alone"
