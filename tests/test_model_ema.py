"""CPU: ``open_clip_amd.NativeModelEma`` / ``setup_ema`` -- the decay schedule against literal values, the host-side plan of ``ocn_ema_lerp_multi``,
the reference's ``CLIPTask`` carrying the native twin through its own state_dict / checkpoint / eval seams, and the refusals.  The average itself
runs on the MI355X only (tests/test_model_ema_gpu.py)."""
import os
import re

import numpy as np
import pytest
import torch

from oracle.ref_shim import import_reference, reference_available

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_reference = pytest.mark.skipif(not reference_available(), reason="reference tree not present")


def _ema(**kw):
    from open_clip_amd import NativeModelEma
    return NativeModelEma(torch.nn.Linear(2, 2), **kw)


def test_get_decay_against_literal_values():
    e = _ema(decay=0.9999, update_after_step=0, use_warmup=True)
    assert e.get_decay(0) == 0.0 and e.get_decay(1) == 0.0
    assert e.get_decay(2) == pytest.approx(1 - 2 ** (-2 / 3), rel=1e-14)
    assert e.get_decay(3) == pytest.approx(1 - 3 ** (-2 / 3), rel=1e-14)
    assert e.get_decay(10 ** 9) == 0.9999
    assert e.get_decay(None) == 0.9999 and e.get_decay() == 0.9999
    e = _ema(decay=0.9999, use_warmup=True, min_decay=0.5)
    assert e.get_decay(1) == 0.0  # the copy step is not lifted
    assert e.get_decay(2) == 0.5  # 1 - 2^(-2/3) = 0.370 < 0.5
    assert e.get_decay(3) == pytest.approx(1 - 3 ** (-2 / 3), rel=1e-14)  # 0.519 > 0.5
    e = _ema(decay=0.9999, use_warmup=True, update_after_step=5)
    assert [e.get_decay(s) for s in (0, 1, 5, 6)] == [0.0] * 4
    assert e.get_decay(7) == pytest.approx(1 - 2 ** (-2 / 3), rel=1e-14)
    assert e.get_decay(8) == pytest.approx(1 - 3 ** (-2 / 3), rel=1e-14)
    assert e.get_decay(10 ** 9 + 5) == 0.9999
    e = _ema(decay=0.9999, use_warmup=True, warmup_gamma=4, warmup_power=1)
    assert e.get_decay(9) == pytest.approx(1 - 1 / 3, rel=1e-14)
    e = _ema(decay=0.99)
    assert e.get_decay(1) == 0.0 and e.get_decay(2) == 0.99 and e.get_decay(None) == 0.99
    assert _ema(decay=0.99, foreach=False).get_decay(2) == 0.99  # accepted and ignored


def test_plan_builder_chunks_modes_and_record_size():
    from open_clip_amd.ema import _EMA_ENTRY, ema_plan
    src = open(os.path.join(ROOT, "open_clip_amd", "csrc", "optim.hip")).read()
    assert _EMA_ENTRY.itemsize == int(re.search(r"static_assert\(sizeof\(EmaEntry\) == (\d+)", src).group(1)) == 32
    chunk = int(re.search(r"constexpr int ADAM_CHUNK = (\d+);", src).group(1))
    assert chunk == 8192
    numels = [1, 4, 8191, 8192, 8193]
    ent, chunks = ema_plan([(4096 + 65536 * i, 8192 + 65536 * i, n) for i, n in enumerate(numels)])
    assert [int((chunks[:, 0] == i).sum()) for i in range(len(numels))] == [1, 1, 1, 1, 2]
    assert chunks.dtype == np.int32 and chunks.shape == (6, 2)
    assert chunks.tolist() == [[0, 0], [1, 0], [2, 0], [3, 0], [4, 0], [4, 1]]
    assert ent["numel"].tolist() == numels and ent["mode"].tolist() == [0] * 5 and ent["pad"].tolist() == [0] * 5
    assert ent["ema"].tolist() == [4096 + 65536 * i for i in range(5)] and ent["src"].tolist() == [8192 + 65536 * i for i in range(5)]
    # mode 2 exactly when a pointer is off the 16-byte grid
    for off_e in (0, 4, 8, 12, 16):
        for off_s in (0, 4, 8, 12, 16):
            ent, _ = ema_plan([(4096 + off_e, 8192 + off_s, 64)])
            assert int(ent["mode"][0]) == (0 if off_e % 16 == 0 and off_s % 16 == 0 else 2), (off_e, off_s)
    ent, chunks = ema_plan([])
    assert ent.shape == (0,) and chunks.shape == (0, 2)
    ent, chunks = ema_plan([(4096, 8192, 0), (4096, 8192, 3 * 8192 + 2)])  # an empty tensor owns no chunk
    assert chunks.tolist() == [[1, 0], [1, 1], [1, 2], [1, 3]]


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """host-side validation only: the fake device pointers are never dereferenced (as tests/test_cabi.py does)"""
    from open_clip_amd import _lib, build
    build.build()
    p = 4096
    for entries, chunks in ((None, p), (p, None)):
        with pytest.raises(RuntimeError, match=r"ocn_ema_lerp_multi failed \(-1\): ocn_ema_lerp_multi: null entry / chunk table"):
            _lib.call("ocn_ema_lerp_multi", entries, chunks, 1, 0.5, None)
    with pytest.raises(RuntimeError, match=r"ocn_ema_lerp_multi failed \(-1\): ocn_ema_lerp_multi: n_chunks must not be negative"):
        _lib.call("ocn_ema_lerp_multi", p, p, -1, 0.5, None)
    for w in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(RuntimeError, match=r"ocn_ema_lerp_multi failed \(-1\): ocn_ema_lerp_multi: weight must be finite"):
            _lib.call("ocn_ema_lerp_multi", p, p, 1, w, None)
    _lib.call("ocn_ema_lerp_multi", p, p, 0, 0.5, None)  # nothing to do: no launch


def _tiny_cpu(seed):
    from open_clip_amd.configs import get_model_config
    from open_clip_amd.model import NativeCLIP
    from open_clip_amd.synth import init_state_dict
    cfg = get_model_config("tiny-test")
    m = NativeCLIP(cfg["embed_dim"], cfg["vision_cfg"], cfg["text_cfg"], output_dict=True)
    m.load_state_dict(init_state_dict(cfg, seed=seed, perturb=True), strict=True)
    return m


@needs_reference
def test_reference_task_carries_the_native_twin(tmp_path):
    import_reference()
    from open_clip.task import CLIPTask
    from open_clip.task.checkpoint import load_checkpoint, save_checkpoint
    from open_clip_amd import NativeModelEma, setup_ema
    from open_clip_amd.loss import NativeClipLoss
    from open_clip_amd.optim import NativeAdamW, param_groups_like_reference

    def make(seed):
        model = _tiny_cpu(seed)
        task = CLIPTask(model, loss=NativeClipLoss(), rank=0, world_size=1, device=torch.device("cpu"), verbose=False)
        return model, task

    model, task = make(3)
    assert not task.has_ema
    assert setup_ema(task, decay=0.99) is task and task.has_ema
    ema = task.trainable_module_ema
    assert type(ema) is NativeModelEma and ema.decay == 0.99 and ema.module is not model
    assert task.get_trainable_module(use_ema=True) is ema.module and task.get_trainable_module(use_ema=False) is model
    task.train()
    assert model.training and task.training and not ema.module.training and not any(m.training for m in ema.module.modules())
    task.eval()
    task.train()
    assert not ema.module.training
    # the twin starts as a copy in storage of its own
    for (k, p), (k2, q) in zip(model.state_dict().items(), ema.module.state_dict().items()):
        assert k == k2 and torch.equal(p, q) and p.data_ptr() != q.data_ptr()
    sd = task.state_dict()
    assert list(sd["state_dict_ema"]) == list(model.state_dict()) == list(sd["state_dict"])
    with torch.no_grad():
        for p in ema.module.parameters():
            p.add_(1.0)
    inference = task.state_dict_for_inference()
    twin_sd = ema.module.state_dict()
    assert list(inference) == list(twin_sd)
    for k, v in inference.items():
        assert v.data_ptr() == twin_sd[k].data_ptr() and torch.equal(v, model.state_dict()[k] + 1.0), k
    # checkpoint round trip through the reference's helpers into a second task that has a twin of its own
    opt = NativeAdamW(param_groups_like_reference(model, 0.2), lr=1e-3)
    ckpt = save_checkpoint(task, opt, epoch=3)
    assert list(ckpt["state_dict_ema"]) == list(model.state_dict())
    path = str(tmp_path / "epoch_3.pt")
    torch.save(ckpt, path)
    model2, task2 = make(4)
    setup_ema(task2, decay=0.99)
    twin2 = task2.trainable_module_ema.module
    assert not torch.equal(model2.token_embedding.weight, model.token_embedding.weight)
    assert load_checkpoint(task2, path) == 3
    for k, v in ema.module.state_dict().items():
        assert torch.equal(twin2.state_dict()[k], v), k
    for k, v in model.state_dict().items():
        assert torch.equal(model2.state_dict()[k], v), k
    assert not torch.equal(twin2.token_embedding.weight, model2.token_embedding.weight)  # the two rows stayed apart
    # without a twin on the loading side the EMA rows are ignored, as with timm's
    model3, task3 = make(5)
    assert load_checkpoint(task3, path) == 3 and not task3.has_ema
    # the average has no CPU path: nothing computes silently
    with pytest.raises(RuntimeError, match="no CPU path"):
        task.update_ema(step=2)


@needs_reference
def test_setup_ema_refuses_fsdp():
    import_reference()
    from open_clip.task import CLIPTask
    from open_clip_amd import setup_ema
    from open_clip_amd.loss import NativeClipLoss
    task = CLIPTask(_tiny_cpu(3), loss=NativeClipLoss(), rank=0, world_size=1, device=torch.device("cpu"), verbose=False)
    task._fsdp_enabled = True
    with pytest.raises(AssertionError, match="EMA must be set up before prepare_fsdp"):
        setup_ema(task)


def test_refusals():
    from open_clip_amd import NativeModelEma
    with torch.device("meta"):
        meta = torch.nn.Linear(4, 4)
    with pytest.raises(ValueError, match="device"):
        NativeModelEma(meta, device="cpu")
    with pytest.raises(ValueError, match="device"):
        NativeModelEma(torch.nn.Linear(4, 4), device="cuda")
    NativeModelEma(meta, device="meta"), NativeModelEma(meta, device=None), NativeModelEma(torch.nn.Linear(4, 4), device=torch.device("cpu"))
    ema = NativeModelEma(torch.nn.Linear(4, 4))
    with pytest.raises(ValueError, match="'bias'"):
        ema.update(torch.nn.Linear(4, 4, bias=False))
    with pytest.raises(ValueError, match="'extra.weight'"):
        other = torch.nn.Linear(4, 4)
        other.extra = torch.nn.Linear(1, 1)
        ema.update(other)
    with pytest.raises(ValueError, match="'weight' has shape"):
        ema.set(torch.nn.Linear(5, 4))
    half = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.Linear(4, 4))
    half[1].weight.data = half[1].weight.data.bfloat16()
    ema = NativeModelEma(half)
    before = [p.clone() for p in ema.module.parameters()]
    with pytest.raises(TypeError, match="'1.weight'"):
        ema.update(half)
    with pytest.raises(TypeError, match="'1.weight'"):
        ema.set(half)
    assert all(torch.equal(p, q) for p, q in zip(ema.module.parameters(), before))  # refused before anything was written
    # an fp32 model on the host: the kernel is the only path
    cpu = torch.nn.Linear(4, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        NativeModelEma(cpu).update(cpu)
