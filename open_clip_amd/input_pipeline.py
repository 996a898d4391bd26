"""Host -> device input path of the hot loop: what ``TrainingTask.prepare_batch`` does
(reference ``src/open_clip/task/base_task.py:135-157``: ``tensor.to(device, non_blocking=True)`` per batch, images as the fp32
output of the transform) re-designed for the native path:

  * images travel as DECODED uint8 pixels ``[B, H, W, 3]`` (4x fewer PCIe bytes than fp32 ``[B, 3, H, W]``: 616 MB instead of
    2.47 GB per 4096-image batch); ToTensor + Normalize with the model's mean / std (``constants.py:1-2``) happen inside the
    patch-embedding kernel (``ocn_patchify_u8``), so no normalised image is ever materialised;
  * batches go pinned-host -> device with ``cudaMemcpyAsync`` on a dedicated COPY stream into one of ``depth`` device slots, while
    the compute stream works on the previous slot; the only coupling is two events per slot (copy done -> compute may read;
    compute done with the slot -> the copy stream may overwrite it).

    pipe = DeviceBatchPipeline(device, image_shape=(B, 224, 224, 3), text_shape=(B, 77))
    pipe.submit(u8_host, text_host)              # enqueue the copy of batch i+1 (returns immediately)
    batch = pipe.next()                          # device tensors of batch i, ordered after their copy on the current stream
    out = model(image=batch["image"], text=batch["text"])   # NativeCLIP accepts the uint8 image directly
    pipe.release(batch)                          # any time after the forward is enqueued (records the slot's 'free' event): the backward
                                                 # reads nothing of the slot -- next() hands out per-step copies of the tokens / text layout

``prepare_batch`` keeps working on the result: it leaves integer tensors (uint8 pixels, int64 tokens) untouched.

With ``crop_size`` the pipeline also does the train transform's ``RandomResizedCrop(image_size, scale, interpolation=BICUBIC)`` (reference
``src/open_clip/transform.py:435-440``) on the device: the loader hands over fixed-size decoded SOURCE images (e.g. 256 x 256), ``submit()`` draws
one crop box per image on the host (or takes the caller's), the boxes travel with the batch and ``next()`` runs ``ops.resized_crop_u8`` on the
compute stream.  Nothing comes back to the host:

    pipe = DeviceBatchPipeline(device, image_shape=(B, 256, 256, 3), text_shape=(B, 77), crop_size=224)
    pipe.submit(u8_source_host, text_host)       # boxes drawn here (crop_generator makes them reproducible); boxes=... for fixed ones
    batch = pipe.next()                          # batch["image"]: uint8 [B, 224, 224, 3] of this step, batch["boxes"]: device int32 [B, 4]

With ``color_jitter_prob`` / ``gray_scale_prob`` the two remaining steps of that transform branch, ``color_jitter(*aug_cfg.color_jitter, p)`` and
``gray_scale(p)`` (``transform.py:335-364``, ``:442-450``), run on the device as well, behind the crop as in the reference: ``submit()`` draws per-image
factors, a step order and the grayscale bit on the host (``color_jitter_plan``, or takes the caller's ``jitter=(factors, plan)``), they travel with the
batch and ``next()`` runs ``ops.color_jitter_u8`` -- in place on the crop's fresh output, into a new tensor when there is no crop (the slot is never
modified).  ``from_aug_cfg`` builds the pipeline from the reference's ``AugmentationCfg`` fields:

    pipe = DeviceBatchPipeline.from_aug_cfg(device, (B, 256, 256, 3), (B, 77), 224, {"scale": (0.9, 1.0), "color_jitter": (0.4, 0.4, 0.4, 0.1),
                                                                                   "color_jitter_prob": 0.8, "gray_scale_prob": 0.2})
    batch = pipe.next()                          # batch["jitter"]: device (factors float32 [B, 4], plan int32 [B]) the image was run with

``DeviceBatchPipeline.ragged`` takes decoded images of their OWN sizes and also does the validation transform (``image_transform(is_train=False)``,
``transform.py:461-492``: resize, then centre crop or pad): ``submit()`` packs the list into a pinned byte arena (``pack_images``), makes one plan per
image on the host (``eval_resample_plan``, or ``train_resample_plan`` with ``train=True``), checks it (``check_resample_plan``) and copies the used prefix
of the arena; ``next()`` runs ``ops.resample_u8``:

    pipe = DeviceBatchPipeline.ragged(device, B, (B, 77), 224, arena_bytes=B * 640 * 640 * 3, resize_mode="shortest")
    pipe.submit(list_of_hwc_u8, text_host)
    batch = pipe.next()                          # batch["image"]: uint8 [B, 224, 224, 3]; batch["plan"] int32 [B, 10], batch["offsets"] int64 [B] on the device

PyTorch is plumbing here (pinned allocations, streams, events); the only arithmetic in this file is the sampling of boxes and jitter parameters and the
resize rules, a few small numbers per image."""
import math

import torch

from . import ops

MAX_CROP_RATIO = 4  # largest box side / output side ocn_resized_crop_u8 resamples as given (17 taps per axis); the kernel clamps a larger side


def _size2(size):
    return (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))


def _sample_crop_boxes(Hs, Ws, scale, ratio, generator):
    """the one sampler behind ``random_resized_crop_boxes`` and ``train_resample_plan``: ``Hs``, ``Ws`` int64 [B], the size of each image -> int64
    [B, 4] = (top, left, height, width), by the rule stated at ``random_resized_crop_boxes`` with every image judged against its own size"""
    B = Hs.shape[0]
    u = torch.rand((4, B, 10), dtype=torch.float64, generator=generator)
    target = (Hs * Ws).double()[:, None] * (scale[0] + (scale[1] - scale[0]) * u[0])
    lr0, lr1 = math.log(ratio[0]), math.log(ratio[1])
    r = torch.exp(lr0 + (lr1 - lr0) * u[1])
    w = torch.round(torch.sqrt(target * r)).long()
    h = torch.round(torch.sqrt(target / r)).long()
    ok = (w > 0) & (w <= Ws[:, None]) & (h > 0) & (h <= Hs[:, None])
    first = ok.int().argmax(dim=1, keepdim=True)  # the first maximum: the first attempt that fits
    w, h, found = w.gather(1, first)[:, 0], h.gather(1, first)[:, 0], ok.any(dim=1)
    top = torch.floor(u[2, :, 0] * (Hs - h + 1).clamp(min=1)).long()
    left = torch.floor(u[3, :, 0] * (Ws - w + 1).clamp(min=1)).long()
    in_ratio = Ws.double() / Hs.double()  # the fallback, per image (torch.round is Python's round: half to even)
    narrow, wide = in_ratio < min(ratio), in_ratio > max(ratio)
    fh = torch.where(narrow, torch.minimum(Hs, torch.round(Ws.double() / min(ratio)).long()), Hs)
    fw = torch.where(wide & ~narrow, torch.minimum(Ws, torch.round(Hs.double() * max(ratio)).long()), Ws)
    return torch.where(found[:, None], torch.stack([top, left, h, w], dim=1), torch.stack([(Hs - fh) // 2, (Ws - fw) // 2, fh, fw], dim=1))


def random_resized_crop_boxes(B, Hs, Ws, scale=(0.9, 1.0), ratio=(3 / 4, 4 / 3), generator=None):
    """The sampling rule of torchvision's ``RandomResizedCrop.get_params`` for B images of one source size, vectorised in torch on the CPU:
    host int32 [B, 4] = (top, left, height, width).  Up to 10 attempts per image, each an area ``Hs * Ws * U(scale)`` and an aspect ratio
    log-uniform in ``ratio`` with ``w = round(sqrt(area * r))``, ``h = round(sqrt(area / r))``; the first attempt with ``0 < w <= Ws`` and
    ``0 < h <= Hs`` wins and the corner is uniform in the room left; an image without one gets the centre crop with the source's ratio clamped
    into ``ratio``.  Reproducible under ``generator``; it does NOT reproduce torchvision's random stream (other draws, other order)."""
    return _sample_crop_boxes(torch.full((B,), Hs, dtype=torch.int64), torch.full((B,), Ws, dtype=torch.int64), scale, ratio, generator).to(torch.int32)


def _raise_first(bads, prefix, describe):
    """``bads``: (bool [B], text) pairs in the order of the checks.  The first pair with a true entry raises ValueError for its first such image i:
    ``prefix`` + ``describe(i)`` + the pair's text"""
    for bad, what in bads:
        if bool(bad.any()):
            raise ValueError(f"{prefix}{describe(int(bad.int().argmax()))} {what}")


def check_boxes(boxes, Hs, Ws, size):
    """host-side check of crop boxes [B, 4] = (top, left, height, width) against the source size and the output ``size`` (int or (Ho, Wo)):
    ValueError for an empty box, one that leaves the source, or a side of more than ``MAX_CROP_RATIO`` x the output side"""
    Ho, Wo = _size2(size)
    if boxes.is_cuda:
        raise ValueError("check_boxes: a host-side check (the boxes of a device tensor are never read back)")
    if boxes.dim() != 2 or boxes.shape[1] != 4 or boxes.is_floating_point():
        raise ValueError(f"check_boxes: expected integer boxes [B, 4] = (top, left, height, width), got {boxes.dtype} {tuple(boxes.shape)}")
    b = boxes.long()
    top, left, h, w = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    _raise_first((((h <= 0) | (w <= 0), "is empty"),
                  ((top < 0) | (left < 0) | (top + h > Hs) | (left + w > Ws), f"lies outside the {Hs} x {Ws} source"),
                  ((h > MAX_CROP_RATIO * Ho) | (w > MAX_CROP_RATIO * Wo), f"has a side of more than {MAX_CROP_RATIO} x the {Ho} x {Wo} output")),
                 "check_boxes: box ", lambda i: f"{i} = {tuple(b[i].tolist())} (top, left, height, width)")


RESAMPLE_MAX_SOURCE, RESAMPLE_MAX_RESIZED = 8192, 4096  # the ranges ocn_resample_u8 forces a plan's source sides and resized sides into
RESAMPLE_ALIGN = 16  # byte alignment of an image inside the arena
RESIZE_MODES = ("shortest", "longest", "squash")


def _sizes(sizes):
    sizes = torch.as_tensor(sizes)
    if sizes.dim() != 2 or sizes.shape[1] != 2 or sizes.is_floating_point() or sizes.is_cuda:
        raise ValueError(f"expected host integer sizes [B, 2] = (Hs, Ws), got {sizes.dtype} {tuple(sizes.shape)} on {sizes.device}")
    if bool((sizes < 1).any()):
        raise ValueError(f"image {int((sizes < 1).any(dim=1).int().argmax())} has an empty side")
    return sizes.long()


def eval_resample_plan(sizes, image_size, resize_mode="shortest"):
    """The plan of ``ops.resample_u8`` for the reference's validation transform ``image_transform(is_train=False, resize_mode=...)``
    (transform.py:461-492) on B images of their own sizes, vectorised in torch on the CPU: ``sizes`` int [B, 2] = (Hs, Ws), ``image_size`` an int or
    (Ho, Wo) -> host int32 [B, 10] = (Hs, Ws, 0, 0, Hs, Ws, Rh, Rw, oy, ox): the whole image is resized to Rh x Rw and rows oy .. oy + Ho, columns
    ox .. ox + Wo of that are the output (a negative offset: fill in front).
      shortest, square target: torchvision's ``Resize(int)``: the short side becomes ``size``, the long side ``int(size * long / short)``;
      shortest, other targets: ``ResizeKeepRatio(image_size)`` (transform.py:171-186, longest = 0): ratio = min(Hs / Ho, Ws / Wo), R = round(x / ratio);
        both followed by ``CenterCrop``: o = int(round((R - m) / 2.0)), Python's round (half to even);
      squash: R = (Ho, Wo), o = 0;
      longest: ratio = max(Hs / Ho, Ws / Wo), R = round(x / ratio), then ``CenterCropOrPad`` (transform.py:211-248): o = -((m - R) // 2) on an axis
        with R < m, the crop rule above on one with R > m."""
    Ho, Wo = _size2(image_size)
    if resize_mode not in RESIZE_MODES:
        raise ValueError(f"eval_resample_plan: resize_mode must be one of {RESIZE_MODES} (got {resize_mode!r})")
    s = _sizes(sizes)
    Hs, Ws = s[:, 0], s[:, 1]
    m = torch.tensor([Ho, Wo])
    if resize_mode == "squash":
        R = m[None, :].expand(s.shape[0], 2)
    elif resize_mode == "shortest" and Ho == Wo:
        short, long = torch.minimum(Hs, Ws), torch.maximum(Hs, Ws)
        new_long = torch.floor((Ho * long).double() / short.double()).long()  # int(size * long / short): a true division, truncated
        tall = Hs >= Ws  # the short side is the width (an equal pair: both sides become size either way)
        R = torch.stack([torch.where(tall, new_long, torch.full_like(Hs, Ho)), torch.where(tall, torch.full_like(Ws, Ho), new_long)], dim=1)
    else:
        rh, rw = Hs.double() / Ho, Ws.double() / Wo
        ratio = torch.maximum(rh, rw) if resize_mode == "longest" else torch.minimum(rh, rw)
        R = torch.round(s.double() / ratio[:, None]).long()  # torch.round is Python's round: half to even
    crop = torch.round((R - m).double() / 2.0).long()
    o = torch.zeros_like(R) if resize_mode == "squash" else torch.where(R < m, -((m - R) // 2), crop)
    zero = torch.zeros_like(Hs)
    return torch.stack([Hs, Ws, zero, zero, Hs, Ws, R[:, 0], R[:, 1], o[:, 0], o[:, 1]], dim=1).to(torch.int32)


def train_resample_plan(sizes, image_size, scale=(0.9, 1.0), ratio=(3 / 4, 4 / 3), generator=None):
    """``random_resized_crop_boxes``' rule (torchvision's ``RandomResizedCrop.get_params``) for B images of their OWN sizes, as a plan of
    ``ops.resample_u8``: ``sizes`` int [B, 2] = (Hs, Ws) -> host int32 [B, 10] = (Hs, Ws, top, left, h, w, Ho, Wo, 0, 0).  The area and the fit of an
    attempt are judged against each image's own size, and an image without a fitting attempt gets ITS centre crop with ITS ratio clamped into
    ``ratio``.  The draws are those of ``random_resized_crop_boxes``: for sources of one size the two give the same boxes under the same generator."""
    Ho, Wo = _size2(image_size)
    s = _sizes(sizes)
    box = _sample_crop_boxes(s[:, 0], s[:, 1], scale, ratio, generator)
    return torch.cat([s, box, torch.tensor([Ho, Wo, 0, 0]).expand(s.shape[0], 4)], dim=1).to(torch.int32)


def pack_images(images, arena, offsets_out):
    """lays B decoded images (uint8 HWC host tensors or arrays [Hs, Ws, 3], each of its own size) one behind the other into ``arena`` (a flat uint8
    host tensor, pinned for an asynchronous copy) at offsets that are multiples of 16 and writes those into ``offsets_out`` (host int64 [B]).
    Returns the bytes used (a multiple of 16, or the arena's size): the prefix of the arena that has to travel.  ValueError, naming the image, for
    one that is not uint8 [Hs, Ws, 3] or no longer fits."""
    if arena.dtype != torch.uint8 or arena.dim() != 1 or arena.is_cuda:
        raise ValueError(f"pack_images: the arena must be a flat uint8 host tensor (got {arena.dtype} {tuple(arena.shape)} on {arena.device})")
    if offsets_out.dtype != torch.int64 or tuple(offsets_out.shape) != (len(images),) or offsets_out.is_cuda:
        raise ValueError(f"pack_images: offsets_out must be host int64 [B = {len(images)}] (got {offsets_out.dtype} {tuple(offsets_out.shape)})")
    cap, off = arena.numel(), 0
    for i, image in enumerate(images):
        t = torch.as_tensor(image)
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or t.numel() == 0 or t.is_cuda:
            raise ValueError(f"pack_images: image {i} must be a host uint8 [Hs, Ws, 3] (got {t.dtype} {tuple(t.shape)} on {t.device})")
        n = t.numel()
        if off + n > cap:
            raise ValueError(f"pack_images: image {i} ({t.shape[0]} x {t.shape[1]}, {n} bytes at offset {off}) does not fit the arena of {cap} bytes")
        arena[off:off + n].view(t.shape).copy_(t)
        offsets_out[i] = off
        off = (off + n + RESAMPLE_ALIGN - 1) // RESAMPLE_ALIGN * RESAMPLE_ALIGN
    return min(off, cap)


def check_resample_plan(plan, offsets, arena_bytes, size):
    """host-side check of a plan of ``ops.resample_u8`` (int32 [B, 10] = (Hs, Ws, top, left, nh, nw, Rh, Rw, oy, ox)) and its ``offsets`` (int64 [B])
    against the arena's size and the output ``size`` (int or (Ho, Wo)): ValueError, naming the image, for a source side outside [1, 8192], an empty
    window or one outside the source, a resized side outside [1, 4096], a window side of more than ``MAX_CROP_RATIO`` x its resized side, an output
    offset beyond 4096, an offset that is negative or no multiple of 16, or an image that does not fit the arena"""
    _size2(size)
    if plan.is_cuda or offsets.is_cuda:
        raise ValueError("check_resample_plan: a host-side check (the plan of a device tensor is never read back)")
    if plan.dim() != 2 or plan.shape[1] != 10 or plan.is_floating_point():
        raise ValueError(f"check_resample_plan: expected an integer plan [B, 10] = (Hs, Ws, top, left, nh, nw, Rh, Rw, oy, ox), got {plan.dtype} {tuple(plan.shape)}")
    if offsets.is_floating_point() or tuple(offsets.shape) != (plan.shape[0],):
        raise ValueError(f"check_resample_plan: expected integer offsets [B = {plan.shape[0]}], got {offsets.dtype} {tuple(offsets.shape)}")
    p, off = plan.long(), offsets.long()
    Hs, Ws, top, left, nh, nw, Rh, Rw, oy, ox = (p[:, i] for i in range(10))
    K, S, R = MAX_CROP_RATIO, RESAMPLE_MAX_SOURCE, RESAMPLE_MAX_RESIZED
    _raise_first((((Hs < 1) | (Ws < 1) | (Hs > S) | (Ws > S), f"has a source side outside [1, {S}]"),
                  ((nh <= 0) | (nw <= 0), "has an empty window"),
                  ((top < 0) | (left < 0) | (top + nh > Hs) | (left + nw > Ws), "has a window that lies outside its source"),
                  ((Rh < 1) | (Rw < 1) | (Rh > R) | (Rw > R), f"has a resized side outside [1, {R}]"),
                  ((nh > K * Rh) | (nw > K * Rw), f"has a window side of more than {K} x its resized side: the loader must reduce such an image first "
                                                  "(for instance with PIL's Image.draft at decode time)"),
                  ((oy.abs() > R) | (ox.abs() > R), f"has an output offset beyond {R}"),
                  ((off < 0) | (off % RESAMPLE_ALIGN != 0), f"has an offset that is negative or no multiple of {RESAMPLE_ALIGN}"),
                  (off + Hs * Ws * 3 > int(arena_bytes), f"does not fit the arena of {int(arena_bytes)} bytes")),
                 "check_resample_plan: image ", lambda i: f"{i} (plan {tuple(p[i].tolist())}, offset {int(off[i])})")


JITTER_STEPS = ("brightness", "contrast", "saturation", "hue")  # step code k + 1 in a plan entry, column k of factors
JITTER_GRAY_BIT = 1 << 12
_JITTER_IDENTITY = (1.0, 1.0, 1.0, 0.0)


def _jitter_ranges(color_jitter):
    """torchvision's ``ColorJitter._check_input`` for (brightness, contrast, saturation, hue): each entry a float v -- [max(0, 1 - v), 1 + v] for the
    first three, [-v, v] with 0 <= v <= 0.5 for hue -- or a (min, max) pair; a range that is the identity alone means the step is absent (None)"""
    if color_jitter is None or isinstance(color_jitter, (int, float)) or len(color_jitter) != 4:
        raise ValueError(f"color_jitter must have 4 entries (brightness, contrast, saturation, hue) when color_jitter_prob is set (got {color_jitter!r})")
    ranges = []
    for name, value in zip(JITTER_STEPS, color_jitter):
        hue = name == "hue"
        center, lo_bound, hi_bound = (0.0, -0.5, 0.5) if hue else (1.0, 0.0, math.inf)
        if isinstance(value, (int, float)):
            if value < 0:
                raise ValueError(f"color_jitter: {name} = {value} must not be negative")
            lo, hi = center - float(value), center + float(value)
            if not hue:
                lo = max(lo, 0.0)
        elif len(value) == 2:
            lo, hi = float(value[0]), float(value[1])
        else:
            raise ValueError(f"color_jitter: {name} must be a number or a (min, max) pair (got {value!r})")
        if not (lo_bound <= lo <= hi <= hi_bound):
            raise ValueError(f"color_jitter: {name} range ({lo}, {hi}) must be ordered and lie in [{lo_bound}, {hi_bound}]")
        ranges.append(None if lo == hi == center else (lo, hi))
    return ranges


def color_jitter_plan(B, color_jitter, color_jitter_prob, gray_scale_prob, generator=None):
    """The parameters of ``ops.color_jitter_u8`` for B images, drawn by the rule of torchvision's ``ColorJitter.get_params`` per image, vectorised in
    torch on the CPU: host (factors float32 [B, 4], plan int32 [B]) in the layout of include/openclip_hip.h.  ``color_jitter`` = (brightness, contrast,
    saturation, hue), each a float v (factor uniform in [max(0, 1 - v), 1 + v]; hue uniform in [-v, v], 0 <= v <= 0.5; v = 0: the step is absent) or a
    (min, max) pair; the present steps run in a uniformly random order; the jitter as a whole is applied with probability ``color_jitter_prob`` (an
    image without it has four zero step codes) and grayscale with probability ``gray_scale_prob`` (None or 0: never).  As in the reference
    (transform.py:442-443) a truthy ``color_jitter_prob`` needs a 4-entry ``color_jitter``, and without it ``color_jitter`` is ignored.  The factor of
    a step that is not in an image's plan is the identity (1, 1, 1, 0).  Reproducible under ``generator``; it does NOT reproduce torchvision's or
    Python's random streams (other draws, other order)."""
    ranges = _jitter_ranges(color_jitter) if color_jitter_prob else [None] * 4
    u = torch.rand((10, B), dtype=torch.float64, generator=generator)  # 0-3 factors, 4-7 order keys, 8 jitter or not, 9 grayscale or not
    applied = u[8] < float(color_jitter_prob or 0.0)
    factors = torch.empty((B, 4), dtype=torch.float64)
    keys = u[4:8].t().clone()
    for k, rng in enumerate(ranges):
        if rng is None:
            factors[:, k] = _JITTER_IDENTITY[k]
            keys[:, k] = 2.0  # behind every present step
        else:
            factors[:, k] = torch.where(applied, rng[0] + (rng[1] - rng[0]) * u[k], torch.tensor(_JITTER_IDENTITY[k], dtype=torch.float64))
    order = torch.argsort(keys, dim=1, stable=True)  # the present steps first, in the order of their keys: a uniform permutation
    present = torch.tensor([r is not None for r in ranges])
    codes = torch.where(present[order] & applied[:, None], order + 1, torch.zeros_like(order))
    plan = (codes << (3 * torch.arange(4))[None, :]).sum(dim=1)
    plan = plan + JITTER_GRAY_BIT * (u[9] < float(gray_scale_prob or 0.0)).long()
    return factors.to(torch.float32), plan.to(torch.int32)


def check_jitter(factors, plan):
    """host-side check of colour jitter parameters (factors float32 [B, 4], plan int32 [B]; layout in include/openclip_hip.h): ValueError for a wrong
    shape or dtype, a non-finite factor, a negative brightness / contrast / saturation factor, |hue| > 0.5, a step code above 4, a step that appears
    twice, or bits above the grayscale bit -- naming the image"""
    if factors.is_cuda or plan.is_cuda:
        raise ValueError("check_jitter: a host-side check (the parameters of a device tensor are never read back)")
    if factors.dtype != torch.float32 or factors.dim() != 2 or factors.shape[1] != 4:
        raise ValueError(f"check_jitter: expected float32 factors [B, 4] = (brightness, contrast, saturation, hue), got {factors.dtype} {tuple(factors.shape)}")
    if plan.dtype != torch.int32 or tuple(plan.shape) != (factors.shape[0],):
        raise ValueError(f"check_jitter: expected an int32 plan [B = {factors.shape[0]}], got {plan.dtype} {tuple(plan.shape)}")
    p = plan.long()
    codes = torch.stack([(p >> (3 * k)) & 7 for k in range(4)], dim=1)
    twice = torch.zeros(plan.shape[0], dtype=torch.bool)
    for c in range(1, 5):
        twice |= (codes == c).sum(dim=1) > 1
    _raise_first(((~torch.isfinite(factors).all(dim=1), "has a factor that is not finite"),
                  ((factors[:, :3] < 0).any(dim=1), "has a negative brightness, contrast or saturation factor"),
                  (factors[:, 3].abs() > 0.5, "has a hue shift outside [-0.5, 0.5]"),
                  ((codes > 4).any(dim=1), "has a step code above 4"),
                  (twice, "has a step twice"),
                  ((p < 0) | (p >= 2 * JITTER_GRAY_BIT), "has bits above the grayscale bit")),
                 "check_jitter: image ", lambda i: f"{i} (factors {tuple(factors[i].tolist())}, plan {int(p[i]):#x})")


class HostTextPlan:
    """The packed layout of one text batch (``model._TextPack``: only the tokens up to the pooled EOT exist in the text tower) computed on
    the HOST, where the tokens come from anyway (the tokenizer's output in the loader), so that the step never has to read the packed row
    count back from the device: index plumbing only (argmax / cumsum / a stable sort of B small integers), the tensors travel with the batch.
    ``device_views()`` are views of ONE int32 buffer + the packed token ids."""

    def __init__(self, text_host: torch.Tensor, vocab_size=None, buckets=True):
        B, L = text_host.shape
        eot = text_host.argmax(dim=-1)  # first maximum, as torch.argmax on the device (transformer.py:941-944)
        lens = eot + 1
        seq_off = torch.zeros(B + 1, dtype=torch.int64)
        seq_off[1:] = lens.cumsum(0)
        self.B, self.L, self.M = B, L, int(seq_off[-1])
        self.n_bad = int(((text_host < 0) | (text_host >= vocab_size)).sum()) if vocab_size is not None else 0
        keep = torch.arange(L)[None, :] < lens[:, None]
        self.tokens = text_host[keep]                                  # [M] int64
        posidx = torch.arange(L, dtype=torch.int32).expand(B, L)[keep]  # [M] int32
        nbk = (L + 31) // 32
        if buckets:
            nb = (lens + 31) // 32
            order = torch.sort(nb, stable=True).indices
            self.counts = torch.bincount(nb - 1, minlength=nbk).tolist()
        else:
            order, self.counts = torch.zeros(0, dtype=torch.int64), None
        # one int32 image: eot [B] | seq_off [B+1] | last_row [B] | order [B or 0] | posidx [M]
        self.ints = torch.cat([eot.int(), seq_off.int(), (seq_off[1:] - 1).int(), order.int(), posidx])
        self.has_order = bool(buckets)

    @staticmethod
    def capacity(B, L):
        return 4 * B + 1 + B * L

    def device_views(self, ints_dev, tokens_dev):
        B, M = self.B, self.M
        o = 0
        eot = ints_dev[o:o + B]; o += B
        seq_off = ints_dev[o:o + B + 1]; o += B + 1
        last_row = ints_dev[o:o + B]; o += B
        order = None
        if self.has_order:
            order = ints_dev[o:o + B]; o += B
        posidx = ints_dev[o:o + M]
        return {"eot": eot, "seq_off": seq_off, "last_row": last_row, "order": order, "posidx": posidx, "tokens": tokens_dev[:M],
                "M": M, "counts": self.counts, "n_bad": self.n_bad}


class DeviceBatchPipeline:
    def __init__(self, device, image_shape, text_shape, depth: int = 2, image_dtype=torch.uint8, plan_text_vocab=None, attn_buckets=True,
                 crop_size=None, crop_scale=(0.9, 1.0), crop_ratio=(3 / 4, 4 / 3), crop_generator=None,
                 color_jitter=None, color_jitter_prob=None, gray_scale_prob=None, jitter_generator=None, ragged=None):
        """``plan_text_vocab`` = the model's vocab_size: every submitted batch also carries its packed text layout computed on the host
        (``HostTextPlan``), attached to the device text tensor; ``NativeCLIP`` then runs the step without any host synchronisation.
        ``crop_size`` (int or (Ho, Wo)): ``image_shape`` is the SOURCE shape [B, Hs, Ws, 3] and every batch is cropped and resized to
        ``crop_size`` on the device, one box per image drawn by ``random_resized_crop_boxes(B, Hs, Ws, crop_scale, crop_ratio, crop_generator)``
        (a host ``torch.Generator``) unless ``submit(boxes=...)`` brings its own.
        ``color_jitter_prob`` / ``gray_scale_prob`` (either one truthy; with or without ``crop_size``): every batch also goes through the train
        transform's colour jitter and grayscale on the device, behind the crop (transform.py:442-450), with per-image parameters drawn by
        ``color_jitter_plan(B, color_jitter, color_jitter_prob, gray_scale_prob, jitter_generator)`` unless ``submit(jitter=...)`` brings its own.
        ``ragged``: set by the ``ragged()`` classmethod, which documents that form; ``image_shape`` is then the OUTPUT shape [B, Ho, Wo, 3]."""
        self.device = torch.device(device)
        self.depth = depth
        self.ragged_cfg = ragged
        if ragged is not None and crop_size is not None:
            raise ValueError("DeviceBatchPipeline: a ragged pipeline resamples by plan; crop_size belongs to the fixed-size form")
        self.crop_size, self.crop_scale, self.crop_ratio, self.crop_generator = crop_size, crop_scale, crop_ratio, crop_generator
        if crop_size is not None and (len(image_shape) != 4 or image_shape[3] != 3 or image_dtype != torch.uint8):
            raise ValueError(f"DeviceBatchPipeline: crop_size needs uint8 source images [B, Hs, Ws, 3] (got {image_dtype} {tuple(image_shape)})")
        self.color_jitter, self.color_jitter_prob, self.gray_scale_prob, self.jitter_generator = color_jitter, color_jitter_prob, gray_scale_prob, jitter_generator
        self.jitter = bool(color_jitter_prob) or bool(gray_scale_prob)
        if self.jitter and (len(image_shape) != 4 or image_shape[3] != 3 or image_dtype != torch.uint8):
            raise ValueError(f"DeviceBatchPipeline: colour jitter / grayscale need uint8 images [B, H, W, 3] (got {image_dtype} {tuple(image_shape)})")
        if color_jitter_prob:
            _jitter_ranges(color_jitter)  # a bad color_jitter is refused here, not at the first submit
        self.plan_text_vocab, self.attn_buckets = plan_text_vocab, attn_buckets
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self.slots = []
        for _ in range(depth):
            self.slots.append({
                "text": torch.empty(text_shape, dtype=torch.int64, device=self.device),
                "h_text": torch.empty(text_shape, dtype=torch.int64).pin_memory(),
                "ready": torch.cuda.Event(), "free": torch.cuda.Event(), "host_done": None, "plan": None,
            })
            if ragged is None:
                self.slots[-1].update(image=torch.empty(image_shape, dtype=image_dtype, device=self.device),
                                      h_image=torch.empty(image_shape, dtype=image_dtype).pin_memory())
            else:  # the sources of a batch, one behind the other, with where each lies and what to resample of it
                self.slots[-1].update(arena=torch.empty(ragged["arena_bytes"], dtype=torch.uint8, device=self.device),
                                      h_arena=torch.empty(ragged["arena_bytes"], dtype=torch.uint8).pin_memory(),
                                      offsets=torch.empty(image_shape[0], dtype=torch.int64, device=self.device),
                                      h_offsets=torch.empty(image_shape[0], dtype=torch.int64).pin_memory(),
                                      rplan=torch.empty((image_shape[0], 10), dtype=torch.int32, device=self.device),
                                      h_rplan=torch.empty((image_shape[0], 10), dtype=torch.int32).pin_memory())
            if plan_text_vocab is not None:
                cap = HostTextPlan.capacity(*text_shape)
                self.slots[-1].update(plan_ints=torch.empty(cap, dtype=torch.int32, device=self.device), h_plan_ints=torch.empty(cap, dtype=torch.int32).pin_memory(),
                                      plan_tokens=torch.empty(text_shape[0] * text_shape[1], dtype=torch.int64, device=self.device),
                                      h_plan_tokens=torch.empty(text_shape[0] * text_shape[1], dtype=torch.int64).pin_memory())
            if crop_size is not None:
                self.slots[-1].update(boxes=torch.empty((image_shape[0], 4), dtype=torch.int32, device=self.device),
                                      h_boxes=torch.empty((image_shape[0], 4), dtype=torch.int32).pin_memory())
            if self.jitter:
                self.slots[-1].update(jit_factors=torch.empty((image_shape[0], 4), dtype=torch.float32, device=self.device),
                                      jit_plan=torch.empty((image_shape[0],), dtype=torch.int32, device=self.device),
                                      h_jit_factors=torch.empty((image_shape[0], 4), dtype=torch.float32).pin_memory(),
                                      h_jit_plan=torch.empty((image_shape[0],), dtype=torch.int32).pin_memory())
        self._w = 0      # next slot to fill
        self._r = 0      # next slot to hand out
        self._queued = 0

    @classmethod
    def from_aug_cfg(cls, device, image_shape, text_shape, image_size, aug_cfg, **kw):
        """the pipeline of the reference's non-timm train transform (``image_transform(is_train=True, aug_cfg=...)``, transform.py:431-455) for
        ``aug_cfg`` = a dict or any object with the fields of its ``AugmentationCfg`` (transform.py:63-75): ``scale`` and ``ratio`` become the crop to
        ``image_size`` (``image_shape`` is the SOURCE shape), ``color_jitter`` / ``color_jitter_prob`` / ``gray_scale_prob`` the jitter and grayscale
        behind it; ``kw`` goes to the constructor (depth, plan_text_vocab, crop_generator, jitter_generator, ...).  ``use_timm``, ``naflex``,
        ``re_prob`` and ``re_count`` are not implemented and are refused by name.  One difference: the reference's non-timm branch silently ignores
        ``ratio`` (RandomResizedCrop's default 3/4 - 4/3 is used); here a ``ratio`` that is set is honoured."""
        fields = ("scale", "ratio", "color_jitter", "re_prob", "re_count", "naflex", "use_timm", "color_jitter_prob", "gray_scale_prob")
        if isinstance(aug_cfg, dict):
            unknown = sorted(set(aug_cfg) - set(fields))
            if unknown:
                raise TypeError(f"from_aug_cfg: unknown aug_cfg field(s) {unknown} (AugmentationCfg has {list(fields)})")
            get = aug_cfg.get
        else:
            get = lambda k: getattr(aug_cfg, k, None)  # noqa: E731
        for name in ("use_timm", "naflex", "re_prob", "re_count"):
            if get(name):
                raise NotImplementedError(f"from_aug_cfg: aug_cfg.{name} = {get(name)!r} (the timm augmentations) is not implemented on the device path")
        return cls(device, image_shape, text_shape, crop_size=image_size, crop_scale=tuple(get("scale") or (0.9, 1.0)),
                   crop_ratio=tuple(get("ratio") or (3 / 4, 4 / 3)), color_jitter=get("color_jitter"), color_jitter_prob=get("color_jitter_prob"),
                   gray_scale_prob=get("gray_scale_prob"), **kw)

    @classmethod
    def ragged(cls, device, batch_size, text_shape, image_size, arena_bytes, train=False, resize_mode="shortest", fill_color=0,
               interpolation="bicubic", **kw):
        """the pipeline for decoded images of their OWN sizes: ``submit(images, text_host)`` takes a list of ``batch_size`` uint8 HWC host tensors or
        arrays, packs them into the slot's pinned arena of ``arena_bytes`` (``pack_images``), makes one plan per image, checks it
        (``check_resample_plan``) and copies the used prefix of the arena; ``next()`` runs ``ops.resample_u8`` to ``image_size`` (int or (Ho, Wo)).
          ``train=False``: the reference's validation transform ``image_transform(is_train=False, resize_mode=..., fill_color=...)``
          (``eval_resample_plan``; ``fill_color`` an int 0..255, the padding of 'longest');
          ``train=True``: its RandomResizedCrop, one box per image by ``train_resample_plan`` with ``crop_scale`` / ``crop_ratio`` / ``crop_generator``
          from ``kw``; the colour jitter / grayscale options of the constructor work behind either;
          ``submit(plan=...)``: the caller's host int32 [B, 10] instead.
        ``interpolation``: 'bicubic', or 'random', which the reference treats as bicubic outside timm (transform.py:387); 'bilinear' is not
        implemented.  The result is torch's antialiased bicubic rounded once; it is not PIL-compatible.  ``kw`` goes to the constructor."""
        if interpolation == "bilinear":
            raise NotImplementedError("DeviceBatchPipeline.ragged: interpolation='bilinear' is not implemented on the device path (bicubic only)")
        if interpolation not in ("bicubic", "random"):
            raise ValueError(f"DeviceBatchPipeline.ragged: interpolation must be 'bicubic', 'bilinear' or 'random' (got {interpolation!r})")
        if resize_mode not in RESIZE_MODES:
            raise ValueError(f"DeviceBatchPipeline.ragged: resize_mode must be one of {RESIZE_MODES} (got {resize_mode!r})")
        if isinstance(fill_color, bool) or not isinstance(fill_color, int) or not 0 <= fill_color <= 255:
            raise ValueError(f"DeviceBatchPipeline.ragged: fill_color must be an int in [0, 255] (got {fill_color!r})")
        arena_bytes = int(arena_bytes)
        if arena_bytes < RESAMPLE_ALIGN or arena_bytes % RESAMPLE_ALIGN:
            raise ValueError(f"DeviceBatchPipeline.ragged: arena_bytes must be a positive multiple of {RESAMPLE_ALIGN} (got {arena_bytes})")
        Ho, Wo = _size2(image_size)
        cfg = {"arena_bytes": arena_bytes, "size": (Ho, Wo), "train": bool(train), "resize_mode": resize_mode, "fill": fill_color}
        return cls(device, (int(batch_size), Ho, Wo, 3), text_shape, ragged=cfg, **kw)

    def staging(self):
        """the pinned host buffers of the slot the next ``submit`` will use -- a loader can decode straight into them and
        then call ``submit()`` without arguments (no extra host copy)"""
        if self.ragged_cfg is not None:
            raise RuntimeError("DeviceBatchPipeline: a ragged pipeline packs its arena in submit(images, text_host); it has no image staging buffer")
        s = self.slots[self._w]
        self._wait_host(s)
        return s["h_image"], s["h_text"]

    @staticmethod
    def _wait_host(s):
        """before the host writes any pinned buffer of slot ``s``: the slot's PREVIOUS transfer (``depth`` batches ago) may still read it -- rare"""
        if s["host_done"] is not None and not s["host_done"].query():
            s["host_done"].synchronize()

    def _submit_ragged(self, s, images, text_host, sizes, plan):
        """the host side of a ragged batch: pack, plan, check -- everything that can refuse the batch, before anything is enqueued"""
        cfg, B = self.ragged_cfg, s["offsets"].shape[0]
        if images is None or text_host is None or torch.is_tensor(images) and images.dim() != 4 or len(images) != B:
            raise ValueError(f"DeviceBatchPipeline: a ragged submit takes B = {B} images (uint8 [Hs, Ws, 3] each) and their text")
        self._wait_host(s)
        used = pack_images(images, s["h_arena"], s["h_offsets"])
        packed = torch.tensor([tuple(torch.as_tensor(im).shape[:2]) for im in images])
        if sizes is not None and not torch.equal(_sizes(sizes), packed):
            raise ValueError("DeviceBatchPipeline: sizes= must be the (Hs, Ws) of the images, in order")
        if plan is None:
            plan = train_resample_plan(packed, cfg["size"], self.crop_scale, self.crop_ratio, self.crop_generator) if cfg["train"] \
                else eval_resample_plan(packed, cfg["size"], cfg["resize_mode"])
        elif tuple(plan.shape) != (B, 10):
            raise ValueError(f"DeviceBatchPipeline: plan must be [B = {B}, 10] (got {tuple(plan.shape)})")
        check_resample_plan(plan, s["h_offsets"], cfg["arena_bytes"], cfg["size"])
        if not torch.equal(plan[:, :2].long(), packed):  # a caller's plan: the sizes it states are the sizes that were packed
            i = int((plan[:, :2].long() != packed).any(dim=1).int().argmax())
            raise ValueError(f"DeviceBatchPipeline: plan {i} states a {tuple(plan[i, :2].tolist())} source, the image is {tuple(packed[i].tolist())}")
        s["h_rplan"].copy_(plan)
        return used

    def submit(self, image_host=None, text_host=None, boxes=None, jitter=None, sizes=None, plan=None):
        """enqueue host -> device of one batch on the copy stream.  ``image_host`` / ``text_host`` = any host tensors (copied into
        the slot's pinned staging buffers first) or None when the caller filled ``staging()`` in place.  ``boxes`` (with ``crop_size`` only):
        the caller's crop boxes, host integers [B, 4] = (top, left, height, width), checked by ``check_boxes`` -- fixed boxes for evaluation;
        None draws them.  ``jitter`` (with ``color_jitter_prob`` / ``gray_scale_prob`` only): the caller's (factors float32 [B, 4], plan int32 [B])
        on the host, checked by ``check_jitter``; None draws them.  A ``ragged()`` pipeline: ``image_host`` is the list of B images, ``sizes`` their
        (Hs, Ws) when the caller has them at hand (they are checked against the images) and ``plan`` the caller's plan (None makes one)."""
        if self._queued == self.depth:
            raise RuntimeError("DeviceBatchPipeline: all slots are in flight; call next() / release() first")
        s = self.slots[self._w]
        if (sizes is not None or plan is not None) and self.ragged_cfg is None:
            raise ValueError("DeviceBatchPipeline: sizes= / plan= need a pipeline built with DeviceBatchPipeline.ragged")
        if boxes is not None and self.crop_size is None:
            raise ValueError("DeviceBatchPipeline: boxes= needs a pipeline built with crop_size")
        if self.crop_size is not None:
            B, Hs, Ws = s["image"].shape[:3]
            if boxes is None:
                boxes = random_resized_crop_boxes(B, Hs, Ws, self.crop_scale, self.crop_ratio, self.crop_generator)
            elif tuple(boxes.shape) != (B, 4):
                raise ValueError(f"DeviceBatchPipeline: boxes must be [B = {B}, 4] (got {tuple(boxes.shape)})")
            check_boxes(boxes, Hs, Ws, self.crop_size)
        if jitter is not None and not self.jitter:
            raise ValueError("DeviceBatchPipeline: jitter= needs a pipeline built with color_jitter_prob or gray_scale_prob")
        if self.jitter:
            B = s["text"].shape[0]
            if jitter is None:
                jitter = color_jitter_plan(B, self.color_jitter, self.color_jitter_prob, self.gray_scale_prob, self.jitter_generator)
            check_jitter(*jitter)
            if jitter[0].shape[0] != B:
                raise ValueError(f"DeviceBatchPipeline: jitter must be (factors [B = {B}, 4], plan [B = {B}]) (got {tuple(jitter[0].shape)}, {tuple(jitter[1].shape)})")
        used = self._submit_ragged(s, image_host, text_host, sizes, plan) if self.ragged_cfg is not None else None
        src_i, src_t = s.get("h_image"), s["h_text"]
        if used is not None:
            if text_host.is_pinned():
                src_t = text_host
            else:
                src_t.copy_(text_host)
        elif image_host is not None:
            if image_host.is_pinned() and text_host.is_pinned():
                src_i, src_t = image_host, text_host  # already page-locked (DataLoader(pin_memory=True)): DMA straight out of it
            else:
                hi, ht = self.staging()
                hi.copy_(image_host)
                ht.copy_(text_host)
        plan = None
        if self.plan_text_vocab is not None:
            self._wait_host(s)
            plan = HostTextPlan(src_t, self.plan_text_vocab, self.attn_buckets)
            s["h_plan_ints"][:plan.ints.numel()].copy_(plan.ints)
            s["h_plan_tokens"][:plan.M].copy_(plan.tokens)
        s["plan"] = plan
        if self.crop_size is not None:
            self._wait_host(s)
            s["h_boxes"].copy_(boxes)
        if self.jitter:
            self._wait_host(s)
            s["h_jit_factors"].copy_(jitter[0])
            s["h_jit_plan"].copy_(jitter[1])
        with torch.cuda.stream(self.copy_stream):
            self.copy_stream.wait_event(s["free"])  # the forward that read this slot last has consumed it
            if used is None:
                s["image"].copy_(src_i, non_blocking=True)
            else:  # only the used prefix of the arena travels; what lies behind it on the device is left as it is
                s["arena"][:used].copy_(s["h_arena"][:used], non_blocking=True)
                s["offsets"].copy_(s["h_offsets"], non_blocking=True)
                s["rplan"].copy_(s["h_rplan"], non_blocking=True)
            s["text"].copy_(src_t, non_blocking=True)
            if plan is not None:
                n = plan.ints.numel()
                s["plan_ints"][:n].copy_(s["h_plan_ints"][:n], non_blocking=True)
                s["plan_tokens"][:plan.M].copy_(s["h_plan_tokens"][:plan.M], non_blocking=True)
            if self.crop_size is not None:
                s["boxes"].copy_(s["h_boxes"], non_blocking=True)
            if self.jitter:
                s["jit_factors"].copy_(s["h_jit_factors"], non_blocking=True)
                s["jit_plan"].copy_(s["h_jit_plan"], non_blocking=True)
            s["ready"].record(self.copy_stream)
            s["host_done"] = s["ready"]
        self._w = (self._w + 1) % self.depth
        self._queued += 1

    def next(self):
        """device batch ``{'image': uint8 [B,H,W,3], 'text': int64 [B,L]}`` of the oldest submitted slot; the current stream is made
        to wait for its copy (no host synchronisation).  With ``crop_size``, 'image' is the cropped and resized batch uint8 [B,Ho,Wo,3], a tensor
        of this step written by ``ops.resized_crop_u8`` on the current stream, and 'boxes' the device int32 [B,4] it was cut with.  With colour jitter /
        grayscale, 'image' has gone through ``ops.color_jitter_u8`` (in place on the crop's fresh output; into a new tensor without ``crop_size``: the
        slot's pixels are never modified) and 'jitter' is the device (factors float32 [B,4], plan int32 [B]) it was run with.  A ``ragged()`` pipeline:
        'image' is uint8 [B,Ho,Wo,3] written by ``ops.resample_u8`` on the current stream, 'plan' (int32 [B,10]) and 'offsets' (int64 [B]) the device
        tensors it was run with."""
        if self._queued == 0:
            raise RuntimeError("DeviceBatchPipeline: nothing submitted")
        s = self.slots[self._r]
        torch.cuda.current_stream(self.device).wait_event(s["ready"])
        self._r = (self._r + 1) % self.depth
        self._queued -= 1
        # What the BACKWARD reads again -- the token ids (embedding backward) and, with a host plan, the whole addressing layout of the packed text
        # tower (seq_off / order / last_row / posidx / packed ids: varlen attention backward, embedding backward, every recomputed block under grad
        # checkpointing) -- is copied out of the slot here, on the compute stream, into tensors of this step (a few MB): the slot then holds nothing
        # that outlives the forward, and ``release()`` right after the forward can never let the copy stream overwrite addressing data under a
        # running backward.  Only the pixels are read in place (by the patch kernel, forward only).
        text = s["text"].clone()
        if s["plan"] is not None:  # rides on the tensor object (prepare_batch leaves a device int64 tensor as it is): model._TextPack picks it up
            plan = s["plan"]
            text._ocn_host_plan = plan.device_views(s["plan_ints"][:plan.ints.numel()].clone(), s["plan_tokens"][:plan.M].clone())
        if self.crop_size is not None:  # reads the slot's pixels and boxes on the compute stream, ahead of any release(): the slot's 'free' event orders
            boxes = s["boxes"].clone()  # the copy stream's next overwrite behind it
            batch = {"image": ops.resized_crop_u8(s["image"], boxes, self.crop_size), "text": text, "boxes": boxes, "_slot": s}
        elif self.ragged_cfg is not None:  # as the crop: reads the slot's arena, offsets and plan on the compute stream, ahead of any release()
            offsets, rplan = s["offsets"].clone(), s["rplan"].clone()
            image = ops.resample_u8(s["arena"], offsets, rplan, self.ragged_cfg["size"], fill=self.ragged_cfg["fill"])
            batch = {"image": image, "text": text, "plan": rplan, "offsets": offsets, "_slot": s}
        else:
            batch = {"image": s["image"], "text": text, "_slot": s}
        fresh = self.crop_size is not None or self.ragged_cfg is not None  # 'image' is this step's own tensor: the jitter may run in place
        if self.jitter:  # the reference's order: crop, jitter, grayscale.  The parameters leave the slot like the boxes
            factors, plan = s["jit_factors"].clone(), s["jit_plan"].clone()
            batch["image"] = ops.color_jitter_u8(batch["image"], factors, plan, out=batch["image"] if fresh else None)
            batch["jitter"] = (factors, plan)
        return batch

    def release(self, batch):
        """call once the forward that reads ``batch`` has been enqueued: the slot's pixels are read by the patch kernel only, and everything
        the backward reads again (token ids, the packed text layout) was copied out of the slot by ``next()``"""
        batch["_slot"]["free"].record(torch.cuda.current_stream(self.device))
