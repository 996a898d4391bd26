"""Model EMA of the HIP path: the exponential moving average of the weights that the reference's task layer keeps through ``timm.utils.ModelEmaV3``
(``TrainingTask.setup_ema`` / ``update_ema`` / ``has_ema``, base_task.py:165-186; ``state_dict()["state_dict_ema"]``, :395-396, :434-437;
``state_dict_for_inference``, :439-443; every ``eval_forward``, clip_task.py:48-50; task/checkpoint.py:81-82, 118-119), without timm.

``NativeModelEma`` holds a deep copy of the model in eval mode (``.module``) and averages into it with ONE launch per update over the whole model
(``ocn_ema_lerp_multi``, include/openclip_hip.h: torch.lerp's two-branch form, fp32): the pointer table of the optimizers (``tables.PinnedTable``), 8192-element
chunks, built once and revalidated against both sides' addresses on every update.  The constructor's options carry the names timm's ModelEmaV3 uses as
far as is known here; timm is not a dependency and nothing was compared with it, so this module -- not timm -- defines what they mean:

  ``get_decay(step)``   ``step is None`` -> ``decay``.  Otherwise ``s = max(0, step - update_after_step - 1)``; ``s <= 0`` -> 0.0 (the twin copies the
                        model); with ``use_warmup`` ``min(max(1 - (1 + s / warmup_gamma) ** -warmup_power, min_decay), decay)``, without it ``decay``.
  ``update(model, step=None)``  ``twin = lerp(twin, model, 1 - get_decay(step))`` over the pairs of both ``state_dict()``s: fp32 entries through the
                        kernel, integer / bool entries copied; ``exclude_buffers``: only parameters are averaged, buffers are copied.  A floating entry
                        that is not fp32 raises TypeError (there is no ATen path for the average), differing keys or shapes raise ValueError.
  ``set(model)``        copies everything: weight 1 through the same launch (exact: the kernel's form returns the source bit for bit).
  ``foreach``           accepted and ignored (one launch is the only form).  ``device`` must be None or the model's device.

``setup_ema(task, decay, **kwargs)`` is ``TrainingTask.setup_ema`` with this class; everything else of the task layer then works as it stands."""
import copy

import numpy as np
import torch
from torch import nn

from . import ops, tables
from .optim import unwrap_model

# EmaEntry of csrc/optim.hip
_EMA_ENTRY = np.dtype([("ema", "<u8"), ("src", "<u8"), ("numel", "<i8"), ("mode", "<i4"), ("pad", "<i4")])
assert _EMA_ENTRY.itemsize == 32


def ema_plan(triples):
    """the tables of ``ocn_ema_lerp_multi`` from ``(ema_ptr, src_ptr, numel)`` triples, on the host: the records (mode 0 = 16-byte vector path when
    both addresses sit on 16 bytes, else 2 = scalar path) and the chunk list, int32 ``[n_chunks, 2]`` of {entry, index}: ceil(numel / 8192) per entry"""
    ent = np.zeros(len(triples), dtype=_EMA_ENTRY)
    for e, (ema_ptr, src_ptr, numel) in zip(ent, triples):
        e["ema"], e["src"], e["numel"] = ema_ptr, src_ptr, numel
        e["mode"] = 0 if ema_ptr % 16 == 0 and src_ptr % 16 == 0 else 2
    return ent, tables.chunk_list(-(-ent["numel"] // tables.CHUNK))


def _device_of(model):
    for t in model.parameters():
        return t.device
    for t in model.buffers():
        return t.device
    return None


class NativeModelEma(nn.Module):
    def __init__(self, model, decay=0.9999, min_decay=0.0, update_after_step=0, use_warmup=False, warmup_gamma=1.0, warmup_power=2 / 3,
                 device=None, foreach=True, exclude_buffers=False):
        super().__init__()
        model = unwrap_model(model)
        have = _device_of(model)
        if device is not None and have is not None:
            want = torch.device(device)
            if want.type != have.type or (want.index is not None and have.index is not None and want.index != have.index):
                raise ValueError(f"NativeModelEma: device={device!r} is not the model's device ({have}); an EMA twin on another device is not "
                                 "implemented (pass device=None)")
        self.module = copy.deepcopy(model).eval()
        self.decay, self.min_decay, self.update_after_step = decay, min_decay, update_after_step
        self.use_warmup, self.warmup_gamma, self.warmup_power = use_warmup, warmup_gamma, warmup_power
        self.foreach, self.exclude_buffers = foreach, exclude_buffers
        self._plan = self._plan_key = None

    def train(self, mode=True):
        """the twin is never trained: it stays in eval mode when the module that owns this one (a task) switches to training"""
        self.training = mode
        self.module.eval()
        return self

    def forward(self, *args, **kwargs):
        return self.module(*args, **kwargs)

    def get_decay(self, step=None):
        if step is None:
            return self.decay
        s = max(0, step - self.update_after_step - 1)
        if s <= 0:
            return 0.0
        if not self.use_warmup:
            return self.decay
        return min(max(1.0 - (1.0 + s / self.warmup_gamma) ** -self.warmup_power, self.min_decay), self.decay)

    def _pairs(self, model):
        """(averaged, copied): the (key, twin tensor, model tensor) triples that go through the kernel and those that are copied; everything is
        checked here, before anything is written"""
        mine, theirs = self.module.state_dict(), unwrap_model(model).state_dict()
        for k in mine:
            if k not in theirs:
                raise ValueError(f"NativeModelEma: the model has no entry '{k}' (the EMA twin has)")
        for k in theirs:
            if k not in mine:
                raise ValueError(f"NativeModelEma: the model's entry '{k}' is not in the EMA twin")
        params = {k for k, _ in self.module.named_parameters()} if self.exclude_buffers else None
        averaged, copied = [], []
        for k, e in mine.items():
            s = theirs[k]
            if e.shape != s.shape:
                raise ValueError(f"NativeModelEma: '{k}' has shape {tuple(s.shape)} in the model and {tuple(e.shape)} in the EMA twin")
            if e.device != s.device:
                raise ValueError(f"NativeModelEma: '{k}' lives on {s.device} in the model and on {e.device} in the EMA twin")
            if (params is not None and k not in params) or not e.is_floating_point():
                copied.append((k, e, s))
                continue
            if e.dtype != torch.float32 or s.dtype != torch.float32:
                raise TypeError(f"NativeModelEma: '{k}' is {s.dtype} in the model and {e.dtype} in the EMA twin; the average runs in fp32 only "
                                "(there is no ATen path)")
            if not (e.is_contiguous() and s.is_contiguous()):
                raise RuntimeError(f"NativeModelEma: '{k}' must be contiguous on both sides")
            if e.numel():
                averaged.append((k, e, s))
        return averaged, copied

    @torch.no_grad()
    def _lerp(self, model, weight):
        averaged, copied = self._pairs(model)
        dev = averaged[0][1].device if averaged else None
        if averaged and dev.type != "cuda":
            raise RuntimeError(f"open_clip_amd: NativeModelEma averages on the MI355X (the model lives on {dev}); there is no CPU path")
        for _, e, s in copied:
            e.copy_(s)
        if averaged:
            # every address of both sides is re-read on every call: model.to(), `p.data = ...`, load_state_dict(assign=True) replace the tensor behind
            # an unchanged name, and a cached address would then read or overwrite freed memory
            key = tuple((e.data_ptr(), s.data_ptr(), e.numel()) for _, e, s in averaged)
            if key != self._plan_key:
                ent, chunks = ema_plan(key)
                self._plan = {"table": tables.PinnedTable(ent, dev), "chunks_dev": torch.from_numpy(chunks).to(dev), "n_chunks": int(chunks.shape[0])}
                self._plan_key = key
            plan = self._plan
            # uploaded on every call, like the optimizers' tables: the copy is ordered on the stream the launch goes to, whichever that is this time
            ops.ema_lerp_multi(plan["table"].upload(), plan["chunks_dev"], plan["n_chunks"], weight)
            tables.finish([e for _, e, _ in averaged])
        # the twin's cached bf16 operand copies are keyed by (address, version): drop them, as after any write through raw pointers
        invalidate = getattr(self.module, "invalidate_weight_caches", None)
        if callable(invalidate):
            invalidate()

    def update(self, model, step=None):
        self._lerp(model, 1.0 - self.get_decay(step))

    def set(self, model):
        self._lerp(model, 1.0)


def setup_ema(task, decay=0.9999, **ema_kwargs):
    """``TrainingTask.setup_ema`` (base_task.py:165-177) with ``NativeModelEma`` in timm's place; returns the task.  ``task.update_ema(step=...)``,
    ``has_ema``, ``state_dict`` / ``load_state_dict``, ``state_dict_for_inference``, ``eval_forward`` and the checkpoint helpers work unmodified."""
    assert not getattr(task, "_fsdp_enabled", False), (
        "EMA must be set up before prepare_fsdp(). FSDP2 sharded parameters are not compatible with NativeModelEma.")
    task.trainable_module_ema = NativeModelEma(unwrap_model(task.trainable_module), decay=decay, **ema_kwargs)
    return task
