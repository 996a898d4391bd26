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

PyTorch is plumbing here (pinned allocations, streams, events); the only arithmetic in this file is the box sampling, B small integers per batch."""
import math

import torch

from . import ops

MAX_CROP_RATIO = 4  # largest box side / output side ocn_resized_crop_u8 resamples as given (17 taps per axis); the kernel clamps a larger side


def random_resized_crop_boxes(B, Hs, Ws, scale=(0.9, 1.0), ratio=(3 / 4, 4 / 3), generator=None):
    """The sampling rule of torchvision's ``RandomResizedCrop.get_params`` for B images of one source size, vectorised in torch on the CPU:
    host int32 [B, 4] = (top, left, height, width).  Up to 10 attempts per image, each an area ``Hs * Ws * U(scale)`` and an aspect ratio
    log-uniform in ``ratio`` with ``w = round(sqrt(area * r))``, ``h = round(sqrt(area / r))``; the first attempt with ``0 < w <= Ws`` and
    ``0 < h <= Hs`` wins and the corner is uniform in the room left; an image without one gets the centre crop with the source's ratio clamped
    into ``ratio``.  Reproducible under ``generator``; it does NOT reproduce torchvision's random stream (other draws, other order)."""
    area = float(Hs * Ws)
    u = torch.rand((4, B, 10), dtype=torch.float64, generator=generator)
    target = area * (scale[0] + (scale[1] - scale[0]) * u[0])
    lr0, lr1 = math.log(ratio[0]), math.log(ratio[1])
    r = torch.exp(lr0 + (lr1 - lr0) * u[1])
    w = torch.round(torch.sqrt(target * r)).long()
    h = torch.round(torch.sqrt(target / r)).long()
    ok = (w > 0) & (w <= Ws) & (h > 0) & (h <= Hs)
    first = ok.int().argmax(dim=1, keepdim=True)  # the first maximum: the first attempt that fits
    w, h, found = w.gather(1, first)[:, 0], h.gather(1, first)[:, 0], ok.any(dim=1)
    top = torch.floor(u[2, :, 0] * (Hs - h + 1).clamp(min=1)).long()
    left = torch.floor(u[3, :, 0] * (Ws - w + 1).clamp(min=1)).long()
    in_ratio = Ws / Hs  # the fallback: one box for every image that found none
    if in_ratio < min(ratio):
        fw, fh = Ws, min(Hs, int(round(Ws / min(ratio))))
    elif in_ratio > max(ratio):
        fh, fw = Hs, min(Ws, int(round(Hs * max(ratio))))
    else:
        fw, fh = Ws, Hs
    fallback = torch.tensor([(Hs - fh) // 2, (Ws - fw) // 2, fh, fw])
    return torch.where(found[:, None], torch.stack([top, left, h, w], dim=1), fallback[None, :]).to(torch.int32)


def check_boxes(boxes, Hs, Ws, size):
    """host-side check of crop boxes [B, 4] = (top, left, height, width) against the source size and the output ``size`` (int or (Ho, Wo)):
    ValueError for an empty box, one that leaves the source, or a side of more than ``MAX_CROP_RATIO`` x the output side"""
    Ho, Wo = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    if boxes.is_cuda:
        raise ValueError("check_boxes: a host-side check (the boxes of a device tensor are never read back)")
    if boxes.dim() != 2 or boxes.shape[1] != 4 or boxes.is_floating_point():
        raise ValueError(f"check_boxes: expected integer boxes [B, 4] = (top, left, height, width), got {boxes.dtype} {tuple(boxes.shape)}")
    b = boxes.long()
    top, left, h, w = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    for bad, what in (((h <= 0) | (w <= 0), "is empty"),
                      ((top < 0) | (left < 0) | (top + h > Hs) | (left + w > Ws), f"lies outside the {Hs} x {Ws} source"),
                      ((h > MAX_CROP_RATIO * Ho) | (w > MAX_CROP_RATIO * Wo), f"has a side of more than {MAX_CROP_RATIO} x the {Ho} x {Wo} output")):
        if bool(bad.any()):
            i = int(bad.int().argmax())
            raise ValueError(f"check_boxes: box {i} = {tuple(b[i].tolist())} (top, left, height, width) {what}")


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
                 crop_size=None, crop_scale=(0.9, 1.0), crop_ratio=(3 / 4, 4 / 3), crop_generator=None):
        """``plan_text_vocab`` = the model's vocab_size: every submitted batch also carries its packed text layout computed on the host
        (``HostTextPlan``), attached to the device text tensor; ``NativeCLIP`` then runs the step without any host synchronisation.
        ``crop_size`` (int or (Ho, Wo)): ``image_shape`` is the SOURCE shape [B, Hs, Ws, 3] and every batch is cropped and resized to
        ``crop_size`` on the device, one box per image drawn by ``random_resized_crop_boxes(B, Hs, Ws, crop_scale, crop_ratio, crop_generator)``
        (a host ``torch.Generator``) unless ``submit(boxes=...)`` brings its own."""
        self.device = torch.device(device)
        self.depth = depth
        self.crop_size, self.crop_scale, self.crop_ratio, self.crop_generator = crop_size, crop_scale, crop_ratio, crop_generator
        if crop_size is not None and (len(image_shape) != 4 or image_shape[3] != 3 or image_dtype != torch.uint8):
            raise ValueError(f"DeviceBatchPipeline: crop_size needs uint8 source images [B, Hs, Ws, 3] (got {image_dtype} {tuple(image_shape)})")
        self.plan_text_vocab, self.attn_buckets = plan_text_vocab, attn_buckets
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self.slots = []
        for _ in range(depth):
            self.slots.append({
                "image": torch.empty(image_shape, dtype=image_dtype, device=self.device),
                "text": torch.empty(text_shape, dtype=torch.int64, device=self.device),
                "h_image": torch.empty(image_shape, dtype=image_dtype).pin_memory(),
                "h_text": torch.empty(text_shape, dtype=torch.int64).pin_memory(),
                "ready": torch.cuda.Event(), "free": torch.cuda.Event(), "host_done": None, "plan": None,
            })
            if plan_text_vocab is not None:
                cap = HostTextPlan.capacity(*text_shape)
                self.slots[-1].update(plan_ints=torch.empty(cap, dtype=torch.int32, device=self.device), h_plan_ints=torch.empty(cap, dtype=torch.int32).pin_memory(),
                                      plan_tokens=torch.empty(text_shape[0] * text_shape[1], dtype=torch.int64, device=self.device),
                                      h_plan_tokens=torch.empty(text_shape[0] * text_shape[1], dtype=torch.int64).pin_memory())
            if crop_size is not None:
                self.slots[-1].update(boxes=torch.empty((image_shape[0], 4), dtype=torch.int32, device=self.device),
                                      h_boxes=torch.empty((image_shape[0], 4), dtype=torch.int32).pin_memory())
        self._w = 0      # next slot to fill
        self._r = 0      # next slot to hand out
        self._queued = 0

    def staging(self):
        """the pinned host buffers of the slot the next ``submit`` will use -- a loader can decode straight into them and
        then call ``submit()`` without arguments (no extra host copy)"""
        s = self.slots[self._w]
        if s["host_done"] is not None and not s["host_done"].query():
            s["host_done"].synchronize()  # the previous transfer out of this pinned buffer has finished
        return s["h_image"], s["h_text"]

    def submit(self, image_host=None, text_host=None, boxes=None):
        """enqueue host -> device of one batch on the copy stream.  ``image_host`` / ``text_host`` = any host tensors (copied into
        the slot's pinned staging buffers first) or None when the caller filled ``staging()`` in place.  ``boxes`` (with ``crop_size`` only):
        the caller's crop boxes, host integers [B, 4] = (top, left, height, width), checked by ``check_boxes`` -- fixed boxes for evaluation;
        None draws them."""
        if self._queued == self.depth:
            raise RuntimeError("DeviceBatchPipeline: all slots are in flight; call next() / release() first")
        s = self.slots[self._w]
        if boxes is not None and self.crop_size is None:
            raise ValueError("DeviceBatchPipeline: boxes= needs a pipeline built with crop_size")
        if self.crop_size is not None:
            B, Hs, Ws = s["image"].shape[:3]
            if boxes is None:
                boxes = random_resized_crop_boxes(B, Hs, Ws, self.crop_scale, self.crop_ratio, self.crop_generator)
            elif tuple(boxes.shape) != (B, 4):
                raise ValueError(f"DeviceBatchPipeline: boxes must be [B = {B}, 4] (got {tuple(boxes.shape)})")
            check_boxes(boxes, Hs, Ws, self.crop_size)
        src_i, src_t = s["h_image"], s["h_text"]
        if image_host is not None:
            if image_host.is_pinned() and text_host.is_pinned():
                src_i, src_t = image_host, text_host  # already page-locked (DataLoader(pin_memory=True)): DMA straight out of it
            else:
                hi, ht = self.staging()
                hi.copy_(image_host)
                ht.copy_(text_host)
        plan = None
        if self.plan_text_vocab is not None:
            if s["host_done"] is not None and not s["host_done"].query():
                s["host_done"].synchronize()  # the slot's PREVIOUS transfer (``depth`` batches ago) still reads the pinned plan buffers: rare
            plan = HostTextPlan(src_t, self.plan_text_vocab, self.attn_buckets)
            s["h_plan_ints"][:plan.ints.numel()].copy_(plan.ints)
            s["h_plan_tokens"][:plan.M].copy_(plan.tokens)
        s["plan"] = plan
        if self.crop_size is not None:
            if s["host_done"] is not None and not s["host_done"].query():
                s["host_done"].synchronize()  # as for the plan: the slot's previous transfer may still read the pinned boxes
            s["h_boxes"].copy_(boxes)
        with torch.cuda.stream(self.copy_stream):
            self.copy_stream.wait_event(s["free"])  # the forward that read this slot last has consumed it
            s["image"].copy_(src_i, non_blocking=True)
            s["text"].copy_(src_t, non_blocking=True)
            if plan is not None:
                n = plan.ints.numel()
                s["plan_ints"][:n].copy_(s["h_plan_ints"][:n], non_blocking=True)
                s["plan_tokens"][:plan.M].copy_(s["h_plan_tokens"][:plan.M], non_blocking=True)
            if self.crop_size is not None:
                s["boxes"].copy_(s["h_boxes"], non_blocking=True)
            s["ready"].record(self.copy_stream)
            s["host_done"] = s["ready"]
        self._w = (self._w + 1) % self.depth
        self._queued += 1

    def next(self):
        """device batch ``{'image': uint8 [B,H,W,3], 'text': int64 [B,L]}`` of the oldest submitted slot; the current stream is made
        to wait for its copy (no host synchronisation).  With ``crop_size``, 'image' is the cropped and resized batch uint8 [B,Ho,Wo,3], a tensor
        of this step written by ``ops.resized_crop_u8`` on the current stream, and 'boxes' the device int32 [B,4] it was cut with."""
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
            return {"image": ops.resized_crop_u8(s["image"], boxes, self.crop_size), "text": text, "boxes": boxes, "_slot": s}
        return {"image": s["image"], "text": text, "_slot": s}

    def release(self, batch):
        """call once the forward that reads ``batch`` has been enqueued: the slot's pixels are read by the patch kernel only, and everything
        the backward reads again (token ids, the packed text layout) was copied out of the slot by ``next()``"""
        batch["_slot"]["free"].record(torch.cuda.current_stream(self.device))
