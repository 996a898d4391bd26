"""CPU: ``NativeDistillClipLoss`` (the reference's ``DistillClipLoss``, src/open_clip/loss.py:187-223) above the compute seam, the factory's distillation
branch and the C ABI of ``ocn_distill_rows``.

The HIP compute seam (``open_clip_amd.loss.PairTerm``) is replaced by ``tests/distill_util.CpuDistillPairTerm`` -- the stand-in of
tests/test_dist_loss_gloo.py with the ``grad=`` keyword and a ``distill`` method; the kernels are what tests/test_distill_gpu.py checks.
  1. gloo, world_size 2 and 3: every mode reproduces the per-rank losses and gradients the REFERENCE recorded (tests/golden/distill_loss_w*.npz, written
     by tools/make_distill_golden.py); the row-sharded form gives the global mode's vectors
  2. one process playing 4 ranks: the row-sharded, local_loss + gather_with_grad and redundant global forms sum to float64 autograd of the formula
  3. any weighting of the two outputs is differentiated exactly
  4. the factory: ``create_loss`` / ``create_task(..., dist_model=teacher)``
  5. the C ABI: version 116 in header, library and ctypes table; argument errors of ``ocn_distill_rows`` by name"""
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle.ref_shim import import_reference, reference_available
from tests.distill_util import CpuDistillPairTerm, PackedCollectives, reference_grads
from tests.golden_util import load
from tests.rank_emulation import unit_features

needs_reference = pytest.mark.skipif(not reference_available(), reason="reference tree not present")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (("global", dict(local_loss=False, gather_with_grad=False)),
         ("local_gwg", dict(local_loss=True, gather_with_grad=True)),
         ("local_nograd", dict(local_loss=True, gather_with_grad=False)),
         ("global_gwg", dict(local_loss=False, gather_with_grad=True)),
         ("global_rowsharded", dict(local_loss=False, gather_with_grad=False, row_sharded=True)))


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import open_clip_amd.loss as L
    L.PairTerm = CpuDistillPairTerm
    g = load(f"distill_loss_w{world}.npz")
    feats, dfeats = torch.from_numpy(g["feats"]), torch.from_numpy(g["dist_feats"])
    res = {}
    for mode, kw in MODES:
        img = feats[rank, 0].clone().requires_grad_(True)
        txt = feats[rank, 1].clone().requires_grad_(True)
        s = torch.tensor(float(g["scale"]), requires_grad=True)
        dimg, dtxt = dfeats[rank, 0].clone().requires_grad_(True), dfeats[rank, 1].clone().requires_grad_(True)
        dscale = torch.tensor(float(g["dist_scale"]), requires_grad=True)
        c, d = L.NativeDistillClipLoss(rank=rank, world_size=world, **kw)(img, txt, s, dimg, dtxt, dscale)
        (c + d).backward()
        assert dimg.grad is None and dtxt.grad is None and dscale.grad is None, "the teacher's inputs get no gradient"
        res[mode] = (float(c), float(d), img.grad.numpy(), txt.grad.numpy(), float(s.grad))
    q.put((rank, res))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,port", [(2, 29751), (3, 29752)])
def test_distill_loss_reproduces_the_reference_under_gloo(world, port):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=400) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
    g = load(f"distill_loss_w{world}.npz")
    assert g["dist_feats"].shape[-1] != g["feats"].shape[-1], "the fixture's teacher width differs from the student's"
    for rank in range(world):
        for mode, _ in MODES:
            c, d, di, dt, ds = got[rank][mode]
            pre = f"r{rank}/{'global' if mode == 'global_rowsharded' else mode}/"  # row-sharded: the reference's "global" numbers
            assert abs(c - float(g[pre + "contrastive"])) < 1e-5 and abs(d - float(g[pre + "distill"])) < 1e-5, (rank, mode)
            np.testing.assert_allclose(di, g[pre + "dimg"], rtol=0, atol=1e-5, err_msg=f"{mode} {pre}")
            np.testing.assert_allclose(dt, g[pre + "dtxt"], rtol=0, atol=1e-5, err_msg=f"{mode} {pre}")
            assert abs(ds - float(g[pre + "dscale"])) < 1e-5, (rank, mode)


def _inputs(W, B, E, Et):
    I, T = unit_features(W * B, E, 3, torch.device("cpu"))
    DI, DT = unit_features(W * B, Et, 11, torch.device("cpu"))
    return I, T, torch.tensor(9.5), DI, DT, torch.tensor(12.0)


def test_distill_rank_emulation_sums_to_float64_autograd(monkeypatch):
    """tolerances: those of tests/test_loss_rank_emulation.py"""
    import open_clip_amd.loss as L
    monkeypatch.setattr(L, "PairTerm", CpuDistillPairTerm)
    W, B, E, Et = 4, 6, 16, 24
    I, T, s, DI, DT, ds = _inputs(W, B, E, Et)
    c_ref, d_ref, dI_ref, dT_ref, ds_ref = reference_grads(I, T, s, DI, DT, ds)
    loss_ref = float(c_ref + d_ref)
    coll = PackedCollectives(torch.cat([I, T, DI, DT], dim=1))  # [WB, 2E + 2E_t]
    monkeypatch.setattr(L, "_all_gather", coll.all_gather)
    monkeypatch.setattr(L, "_reduce_scatter_sum", coll.reduce_scatter)
    monkeypatch.setattr(L, "_all_reduce_sum", coll.all_reduce)

    def rank_step(r, **kw):
        sl = slice(r * B, (r + 1) * B)
        Ir, Tr, sr = I[sl].clone().requires_grad_(True), T[sl].clone().requires_grad_(True), s.clone().requires_grad_(True)
        c, d = L.NativeDistillClipLoss(rank=r, world_size=W, **kw)(Ir, Tr, sr, DI[sl], DT[sl], ds)
        (c + d).backward()
        return Ir.grad, Tr.grad, sr.grad, (c + d).detach()

    for kw, mult, tol in ((dict(row_sharded=True), 1, 1.0), (dict(local_loss=True, gather_with_grad=True), W, 10.0)):
        coll.rs_inputs.clear()
        dI, dT, dsc, losses = zip(*(rank_step(r, **kw) for r in range(W)))
        cols = torch.stack(coll.rs_inputs).sum(0)  # every reduce-scatter payload is [WB, 2E]: the teacher's features carry no gradient
        assert cols.shape == (W * B, 2 * E)
        assert torch.allclose((torch.cat(dI) + cols[:, :E]).double(), mult * dI_ref, atol=1e-6 * tol), kw
        assert torch.allclose((torch.cat(dT) + cols[:, E:]).double(), mult * dT_ref, atol=1e-6 * tol), kw
        assert abs(float(torch.stack(losses).sum()) - mult * loss_ref) < 1e-5 * tol and abs(float(torch.stack(dsc).sum()) - mult * float(ds_ref)) < 1e-6 * tol, kw
    r = 2
    dI, dT, dsc, loss = rank_step(r, row_sharded=False)
    assert torch.allclose(dI.double(), dI_ref[r * B:(r + 1) * B], atol=1e-6) and torch.allclose(dT.double(), dT_ref[r * B:(r + 1) * B], atol=1e-6)
    assert abs(float(loss) - loss_ref) < 1e-5 and abs(float(dsc) - float(ds_ref)) < 1e-6


def test_any_weighting_of_the_two_outputs_is_differentiated_exactly(monkeypatch):
    import open_clip_amd.loss as L
    monkeypatch.setattr(L, "PairTerm", CpuDistillPairTerm)
    I, T, s, DI, DT, ds = _inputs(1, 12, 16, 24)

    def grads(wc, wd):
        Ir, Tr, sr = I.clone().requires_grad_(True), T.clone().requires_grad_(True), s.clone().requires_grad_(True)
        c, d = L.NativeDistillClipLoss()(Ir, Tr, sr, DI, DT, ds)
        (wc * c + wd * d).backward()
        return Ir.grad, Tr.grad, sr.grad

    both, only_c, only_d = grads(2.0, 0.25), grads(1.0, 0.0), grads(0.0, 1.0)
    ref = reference_grads(I, T, s, DI, DT, ds, wc=2.0, wd=0.25)[2:]
    assert float(only_d[0].abs().max()) > 1e-3 and not torch.allclose(only_c[0], only_d[0], atol=1e-4), "the two parts have different gradients"
    for got, gc, gd, want in zip(both, only_c, only_d, ref):
        assert torch.allclose(got, 2.0 * gc + 0.25 * gd, atol=1e-7, rtol=1e-6)
        assert torch.allclose(got.double(), want, atol=2e-6)


def test_output_dict_and_signature_follow_the_reference(monkeypatch):
    import inspect
    import open_clip_amd.loss as L
    monkeypatch.setattr(L, "PairTerm", CpuDistillPairTerm)
    I, T, s, DI, DT, ds = _inputs(1, 6, 16, 24)
    loss = L.NativeDistillClipLoss()
    out = loss(image_features=I, text_features=T, logit_scale=s, dist_image_features=DI, dist_text_features=DT, dist_logit_scale=ds, output_dict=True)
    pair = loss(I, T, s, DI, DT, ds)
    assert list(out) == ["contrastive_loss", "distill_loss"] and torch.equal(out["contrastive_loss"], pair[0]) and torch.equal(out["distill_loss"], pair[1])
    assert torch.equal(pair[0], L.NativeClipLoss()(I, T, s)), "the contrastive part is NativeClipLoss's call"
    assert list(inspect.signature(loss.forward).parameters) == ["image_features", "text_features", "logit_scale", "dist_image_features",
                                                                "dist_text_features", "dist_logit_scale", "output_dict"]
    assert inspect.signature(L.NativeDistillClipLoss.__init__) == inspect.signature(L.NativeClipLoss.__init__)


def test_contrastive_part_still_gathers_2E_and_distill_gathers_once(monkeypatch):
    import open_clip_amd.loss as L
    monkeypatch.setattr(L, "PairTerm", CpuDistillPairTerm)
    W, B, E, Et = 2, 4, 16, 24
    I, T, s, DI, DT, ds = _inputs(W, B, E, Et)
    coll = PackedCollectives(torch.cat([I, T, DI, DT], dim=1))
    shapes = []

    def all_gather(out, inp, comm=None):
        shapes.append((tuple(inp.shape), tuple(out.shape)))
        coll.all_gather(out, inp)

    monkeypatch.setattr(L, "_all_gather", all_gather)
    monkeypatch.setattr(L, "_reduce_scatter_sum", coll.reduce_scatter)
    monkeypatch.setattr(L, "_all_reduce_sum", coll.all_reduce)
    L.NativeDistillClipLoss(rank=0, world_size=W, row_sharded=True)(I[:B], T[:B], s, DI[:B], DT[:B], ds)
    assert shapes == [((B, 2 * E), (W * B, 2 * E)), ((B, 2 * E + 2 * Et), (W * B, 2 * E + 2 * Et))]


def test_create_loss_selects_the_distillation_loss():
    import open_clip_amd
    from open_clip_amd.loss import NativeClipLoss, NativeDistillClipLoss
    args = types.SimpleNamespace(model="ViT-B-32", distill=True, local_loss=True, gather_with_grad=True, rank=3, world_size=8)
    loss = open_clip_amd.create_loss(args, deterministic=True)
    assert type(loss) is NativeDistillClipLoss and isinstance(loss, NativeClipLoss) and open_clip_amd.NativeDistillClipLoss is NativeDistillClipLoss
    assert (loss.local_loss, loss.gather_with_grad, loss.rank, loss.world_size, loss.row_sharded, loss.deterministic) == (True, True, 3, 8, False, True)
    args = types.SimpleNamespace(model="ViT-B-32", distill=True, rank=0, world_size=8)
    assert open_clip_amd.create_loss(args).row_sharded and not open_clip_amd.create_loss(args, row_sharded=False).row_sharded
    args.world_size = 1
    assert not open_clip_amd.create_loss(args).row_sharded
    args.distill = False
    assert type(open_clip_amd.create_loss(args)) is NativeClipLoss


def _tiny_cpu(seed):
    from open_clip_amd.configs import get_model_config
    from open_clip_amd.model import NativeCLIP
    from open_clip_amd.synth import init_state_dict
    cfg = get_model_config("tiny-test")
    m = NativeCLIP(cfg["embed_dim"], cfg["vision_cfg"], cfg["text_cfg"], output_dict=True)
    m.load_state_dict(init_state_dict(cfg, seed=seed, perturb=True), strict=True)
    return m


@needs_reference
def test_create_task_builds_the_references_distill_task_around_the_native_loss():
    import_reference()
    import open_clip_amd
    from open_clip.task import DistillCLIPTask
    from open_clip_amd.loss import NativeDistillClipLoss
    student, teacher = _tiny_cpu(1), _tiny_cpu(2)
    args = types.SimpleNamespace(model="tiny-test", distill=True, siglip=False, local_loss=False, gather_with_grad=False, rank=1, world_size=4)
    task = open_clip_amd.create_task(args, student, dist_model=teacher, device=torch.device("cpu"), verbose=False)
    assert type(task) is DistillCLIPTask and task.trainable_module is student and task.teacher is teacher
    assert type(task.loss) is NativeDistillClipLoss and (task.loss.rank, task.loss.world_size, task.loss.row_sharded) == (1, 4, True)
    assert all(not p.requires_grad for p in teacher.parameters()) and all(p.requires_grad for p in student.parameters())
    task.train()
    assert student.training and not teacher.training, "the teacher stays in eval mode"
    with pytest.raises(NotImplementedError, match=r"distill.*requires dist_model"):
        open_clip_amd.create_task(args, student)
    args.distill = False
    with pytest.raises(ValueError, match="dist_model was given but args.distill is not set"):
        open_clip_amd.create_task(args, student, dist_model=teacher)


def test_cabi_version_116_and_distill_rows_argument_errors():
    """host-side validation only: the fake device pointers are never dereferenced (as tests/test_model_ema.py does)"""
    from open_clip_amd import _lib, build
    build.build()
    header = open(os.path.join(ROOT, "include", "openclip_hip.h")).read()
    assert int(re.search(r"#define OCN_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == _lib.load().ocn_version() == 116
    assert re.search(r"116\s+distillation: new ocn_distill_rows \(no signature changed\)", header)
    assert "ocn_distill_rows" in _lib.SIGNATURES and re.search(r"int ocn_distill_rows\(const float\* student, int ld_s, const float\* teacher, int ld_t,", header)
    p = 4096
    ok = dict(student=p, ld_s=8, teacher=p, ld_t=12, G=p, ldg=64, R=2, N=8, ls=0.5, gs=0.5, inv=1.0, loss=p, dscale=p, det=None, stream=None)

    def call(**kw):
        _lib.call("ocn_distill_rows", *{**ok, **kw}.values())

    for name in ("student", "teacher", "G", "loss", "dscale"):
        with pytest.raises(RuntimeError, match=r"ocn_distill_rows failed \(-1\): ocn_distill_rows: null operand"):
            call(**{name: None})
    for kw in (dict(R=0), dict(N=0), dict(R=-1)):
        with pytest.raises(RuntimeError, match=r"ocn_distill_rows failed \(-1\): ocn_distill_rows: bad shape R=-?\d+ N=\d+"):
            call(**kw)
    for kw in (dict(ld_s=7), dict(ld_t=7), dict(ldg=7)):
        with pytest.raises(RuntimeError, match=r"ocn_distill_rows failed \(-1\): ocn_distill_rows: row stride below N=8"):
            call(**kw)
