"""The reference's loss / task dispatch seam for the native path.

``open_clip.factory.create_task(args, model)`` (factory.py:975-1043, called from open_clip_train/main.py:364) builds the task AND its loss from the
training arguments -- and for a ``NativeCLIP`` it would build the ATen ``ClipLoss`` / ``SigLipLoss``.  ``create_task`` / ``create_loss`` here take the
same arguments and make the same choices (``args.distill`` -> DistillCLIPTask + softmax and distillation loss around the teacher handed in as
``dist_model``, ``args.siglip`` -> SigLIPTask + sigmoid loss, else CLIPTask + softmax loss; ``args.local_loss``,
``args.gather_with_grad``, ``args.rank``, ``args.world_size``, ``args.loss_dist_impl``) with the NATIVE losses inside the REFERENCE's own task
classes, so ``main.py`` needs one changed import and nothing else.  The task classes come from the ``open_clip`` package the caller has installed
(imported here, at call time: this package never depends on it otherwise).  What the native path does not implement raises instead of silently
building something else: CoCa, GenLIP / GenLAP, CLAP (SURVEY.md section 8 marks them out of scope).
"""
import sys
from typing import Optional


def _unsupported(args):
    name = str(getattr(args, "model", "")).lower()
    for key, what in (("coca", "CoCa (CoCaLoss / CoCaTask)"), ("genlap", "GenLAP"), ("genlip", "GenLIP")):
        if key in name:
            return what
    return None


def create_loss(args, comm=None, deterministic: bool = False, row_sharded: Optional[bool] = None):
    """``open_clip.factory.create_loss`` (factory.py:930-972) for the native losses.  ``cache_labels`` has no counterpart (labels are never
    materialised: the kernels compare against ``label_offset + row``).  ``comm``: a ``NativeComm`` (RCCL through the C ABI) for the loss collectives
    instead of torch.distributed's process group.  ``row_sharded`` (ClipLoss with world_size > 1 and ``local_loss=False``): every rank evaluates only
    its own rows of the global logits both ways -- same value and gradients as the reference's redundant form; default on when distributed."""
    from .loss import NativeClipLoss, NativeDistillClipLoss, NativeSigLipLoss
    bad = _unsupported(args)
    if bad is not None:
        raise NotImplementedError(f"open_clip_amd.create_loss: {bad} is not implemented by the native path; use open_clip.factory.create_loss")
    rank, world = int(getattr(args, "rank", 0)), int(getattr(args, "world_size", 1))
    distill = bool(getattr(args, "distill", False))  # factory.py:931-938: the reference tests args.distill first, too
    if getattr(args, "siglip", False) and not distill:
        return NativeSigLipLoss(rank=rank, world_size=world, dist_impl=getattr(args, "loss_dist_impl", None), comm=comm, deterministic=deterministic)
    local_loss = bool(getattr(args, "local_loss", False))
    if row_sharded is None:
        row_sharded = world > 1 and not local_loss
    cls = NativeDistillClipLoss if distill else NativeClipLoss
    return cls(local_loss=local_loss, gather_with_grad=bool(getattr(args, "gather_with_grad", False)), rank=rank, world_size=world,
               row_sharded=bool(row_sharded) and world > 1 and not local_loss, comm=comm, deterministic=deterministic)


def create_task(args, model, dist_model=None, naflex_data_config=None, comm=None, deterministic: bool = False, **task_kwargs):
    """``open_clip.factory.create_task`` (factory.py:975-1043): the reference's ``CLIPTask`` / ``SigLIPTask`` / ``DistillCLIPTask`` around ``model`` with
    the native loss that ``create_loss(args)`` selects.  ``task_kwargs`` go to the task constructor (``device=``, ``dtype=``, ``verbose=``).
    ``args.distill`` (main.py:247: a teacher was named) needs ``dist_model``, the teacher main.py builds with
    ``create_model(args.distill_model, pretrained=args.distill_pretrained)``: any module that returns the feature dict, a ``NativeCLIP`` for the
    teacher's forward to run on the HIP path as well.  The task freezes it, keeps it in eval mode and runs it under ``no_grad``."""
    from .model import NativeCLIP
    if not isinstance(model, NativeCLIP):
        raise TypeError(f"open_clip_amd.create_task wraps a NativeCLIP (got {type(model).__name__}); other models go through open_clip.factory.create_task")
    distill = bool(getattr(args, "distill", False))
    if distill and dist_model is None:
        raise NotImplementedError("open_clip_amd.create_task: args.distill without a teacher is not implemented: distillation requires "
                                  "dist_model=<the teacher model> (main.py builds it from --distill-model / --distill-pretrained)")
    if dist_model is not None and not distill:
        raise ValueError("open_clip_amd.create_task: dist_model was given but args.distill is not set (main.py:247 derives it from --distill-model); "
                         "the teacher would be ignored")
    loss = create_loss(args, comm=comm, deterministic=deterministic)
    try:
        from open_clip.task import CLIPTask, SigLIPTask
    except ImportError as e:  # the task classes are the reference's own: this package restates none of them
        raise ImportError("open_clip_amd.create_task needs the reference's `open_clip` package (open_clip.task.CLIPTask / SigLIPTask) on sys.path") from e
    shared = dict(rank=int(getattr(args, "rank", 0)), world_size=int(getattr(args, "world_size", 1)))
    if distill:
        # the third task class of the same seam, taken from the module the line above imported (tests/test_reference_archive.py pins that line as the
        # package's one import of the reference)
        DistillCLIPTask = sys.modules["open_clip.task"].DistillCLIPTask
        task = DistillCLIPTask(model, dist_model, loss=loss, **shared, **task_kwargs)
    else:
        cls = SigLIPTask if getattr(args, "siglip", False) else CLIPTask
        task = cls(model, loss=loss, **shared, **task_kwargs)
    if naflex_data_config is not None:
        task.set_naflex_data_config(naflex_data_config)
    return task
