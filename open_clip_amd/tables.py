"""The host side of every multi-tensor launch of the HIP path: a table of fixed-size records (one per tensor) plus a chunk list of {entry, index}
pairs (one per workgroup), uploaded through pinned buffers and walked by ONE launch over the whole model.  ``NativeAdamW`` / ``NativeNAdamW`` /
``NativeMuon`` (optim.py) and ``NativeModelEma`` (ema.py) are its callers; csrc/optim.hip and csrc/muon.hip hold the kernels.

``PinnedTable`` is the upload, ``chunk_list`` the one builder of chunk lists, ``AdamTables`` the one owner of ``AdamEntry`` tables (csrc/optim.hip):
the static plan (``adam_plan``: a pure host function), the per-step refresh of a record, the clip launch and the update launch (``run``).  ``copies_of``,
``scalars_to_host`` and ``finish`` are what the optimizer families share besides."""
import numpy as np
import torch

from . import ops

CHUNK = 8192  # ADAM_CHUNK of csrc/optim.hip: the elements one workgroup walks outside tile mode
# AdamEntry of csrc/optim.hip; the four per-step floats carry AdamW's names, NAdamW reads them as decay, bc2, c_g, c_m (the unions of AdamEntry)
ADAM_ENTRY = np.dtype([("w", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("w16n", "<u8"), ("w16t", "<u8"), ("numel", "<i8"),
                       ("rows", "<i4"), ("cols", "<i4"), ("mode", "<i4"), ("pad", "<i4"),
                       ("lr", "<f4"), ("wd", "<f4"), ("bc1", "<f4"), ("bc2_sqrt", "<f4")])
assert ADAM_ENTRY.itemsize == 88
_PER_STEP = ("w", "g", "m", "v", "mode", "lr", "wd", "bc1", "bc2_sqrt")


class PinnedTable:
    """a record table that travels host -> device every step through one of TWO pinned buffers used alternately: the buffer a step fills was last
    read by the upload of two steps ago, so the wait never blocks a host that runs a step ahead of the device"""

    def __init__(self, records, dev):
        self.records = records
        nbytes = records.size * records.dtype.itemsize
        self.host = [torch.empty(nbytes, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.dev = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.copied, self.turn = [None, None], 0

    def upload(self):
        turn, self.turn = self.turn, 1 - self.turn
        if self.copied[turn] is not None and not self.copied[turn].query():
            self.copied[turn].synchronize()  # the upload of two steps ago out of this pinned buffer (in practice long finished)
        self.host[turn].numpy()[:] = self.records.view(np.uint8).reshape(-1)
        self.dev.copy_(self.host[turn], non_blocking=True)
        self.copied[turn] = torch.cuda.Event()
        self.copied[turn].record()
        return self.dev


def chunk_list(counts):
    """int32 ``[sum(counts), 2]`` of {entry, index}: entry ``i`` owns ``counts[i]`` consecutive rows with index 0 .. counts[i] - 1 (none for a count
    of 0; shape (0, 2) for no entries at all)"""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    out = np.empty((int(counts.sum()), 2), dtype=np.int32)
    out[:, 0] = np.repeat(np.arange(counts.size), counts)
    out[:, 1] = np.arange(out.shape[0]) - np.repeat(np.cumsum(counts) - counts, counts)
    return out


def copies_of(weight_caches, p):
    """the cached bf16 operand copies (``n``: [rows, cols], ``t``: [cols, rows]) of a GEMM weight in the first cache that holds each, or None"""
    n = t = None
    if p.ndim in (2, 4):
        for c in weight_caches:
            n = c.peek(p, "n") if n is None else n
            t = c.peek(p, "t") if t is None else t
    return n, t


def scalars_to_host(state, kinds):
    """after ``load_state_dict``: torch stores its scalar state (``step``, NAdam's ``mu_product``) as 0-d tensors in its own checkpoints, the native
    optimizers keep host numbers -- accept both.  ``kinds``: key -> int / float"""
    for st in state.values():
        for k, kind in kinds.items():
            if torch.is_tensor(st.get(k)):
                st[k] = kind(st[k].item())


def finish(tensors, copies=(), weight_caches=()):
    """after a launch that wrote ``tensors`` through raw pointers: bump their version counters, and tell the caches which operand copies
    (``copies``: (n16, t16) per tensor) the same launch rewrote"""
    torch.autograd.graph.increment_version(tensors)
    for p, (n16, t16) in zip(tensors, copies):
        for c in weight_caches:
            c.mark_fresh(p, n16, t16)


def adam_state(state, p, scalars):
    """the AdamW-family state of ``p`` (created on first use): ``scalars`` (key -> (zero, type)) and the two moments"""
    st = state[p]
    if not st:
        for k, (zero, _) in scalars.items():
            st[k] = zero
        st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
    return st


def adamw_fill(group, st, shared):
    """the four per-step floats of a record under torch.optim.AdamW's rule; ``shared``: (beta1, beta2, ...)"""
    return group["lr"], group["weight_decay"], 1.0 - shared[0] ** st["step"], (1.0 - shared[1] ** st["step"]) ** 0.5


def adam_plan(params, copies, tiles=True):
    """the static part of an ``AdamEntry`` table, on the host alone (CPU tensors do): ``(records, counts, copies)`` for the tensors ``params`` and
    their cached operand copies ``copies`` ((n16, t16) per tensor, either may be None).  A 2-D / 4-D weight whose transposed copy is cached and whose
    [shape[0], -1] view is 64-divisible both ways runs in tile mode (mode 1: one 64x64 tile per chunk, both copies rewritten in the launch); every
    other tensor in 8192-element chunks (mode 0 / 2, decided per step from the addresses), where only the plain copy is rewritten and a transposed one
    stays on the cast path.  ``tiles=False``: every tensor enters as ``rows = 1, cols = numel``, never in tile mode.  Returns the records, the chunk
    count of each and the copies the launch DOES rewrite."""
    ent = np.zeros(len(params), dtype=ADAM_ENTRY)
    counts, kept = [], []
    for e, p, (n16, t16) in zip(ent, params, copies):
        rows = p.shape[0] if tiles and p.ndim >= 2 else 1
        cols = p.numel() // rows if p.numel() else 0
        tile = tiles and t16 is not None and rows % 64 == 0 and cols % 64 == 0
        if not tile:
            t16 = None
        e["w16n"] = 0 if n16 is None else n16.data_ptr()
        e["w16t"] = 0 if t16 is None else t16.data_ptr()
        e["numel"], e["rows"], e["cols"] = p.numel(), rows, cols
        e["mode"] = 1 if tile else 0
        counts.append((rows // 64) * (cols // 64) if tile else -(-p.numel() // CHUNK))
        kept.append((n16, t16))
    return ent, counts, kept


class AdamTables:
    """The ``AdamEntry`` table of one optimizer over the tensors ``params``, record ``i`` for ``params[i]``: plan, per-step refresh, clip launch and
    update launch.  ``update`` (a bool per tensor, default all) picks the tensors the update launch walks -- the clip always sums over every one;
    ``not_contiguous`` is the message for a strided parameter or moment.  Building it touches no device: ``to(dev)`` allocates the pinned upload
    and the device chunk lists."""

    def __init__(self, not_contiguous, params, copies, tiles=True, update=None):
        self.not_contiguous = not_contiguous
        self.records, counts, self.copies = adam_plan(params, copies, tiles)
        self.tile = (self.records["mode"] == 1).tolist()
        self.update = [True] * len(params) if update is None else list(update)
        self.chunks = chunk_list(counts)
        self.update_chunks = chunk_list([k if u else 0 for k, u in zip(counts, self.update)])

    def to(self, dev):
        self.table = PinnedTable(self.records, dev)
        self.chunks_dev, self.update_dev = torch.from_numpy(self.chunks).to(dev), torch.from_numpy(self.update_chunks).to(dev)
        return self

    def refresh(self, active, state, scalars, fill, shared):
        """every record for this step, in ONE pass over ``active`` (the (group, p) pairs behind ``params``): addresses, mode, the step count and the
        four per-step floats ``fill(group, st, shared)`` of an updated tensor, whose state (``adam_state``) is created on first use.  Returns the
        (contiguous) gradients the records point to: keep them until the launches are queued."""
        # every pointer of the record is re-read every step: load_state_dict(), model.to(), `p.data = ...` replace the
        # parameter / moment tensors behind an unchanged id(p), and a cached address would then update freed memory
        rows, grads = [], []
        for (group, p), tile, update in zip(active, self.tile, self.update):
            g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
            grads.append(g)
            if not update:  # a tensor the clip alone reads: the scalar loop, whatever the mode
                rows.append((p.data_ptr(), g.data_ptr(), 0, 0, 0 if g.data_ptr() % 16 == 0 else 2, 0.0, 0.0, 0.0, 0.0))
                continue
            st = state[p] or adam_state(state, p, scalars)
            st["step"] += 1
            m, v = st["exp_avg"], st["exp_avg_sq"]
            if not (m.is_contiguous() and v.is_contiguous() and p.is_contiguous()):
                raise RuntimeError(self.not_contiguous)
            if m.device != p.device or m.dtype != torch.float32 or v.dtype != torch.float32:
                st["exp_avg"], st["exp_avg_sq"] = m, v = m.to(p.device, torch.float32), v.to(p.device, torch.float32)
            ptrs = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr())
            # the 16-byte vector path needs all four on the 16-byte grid (a gradient may be a view into a DDP bucket at any 4-byte offset)
            rows.append(ptrs + (1 if tile else 0 if (ptrs[0] | ptrs[1] | ptrs[2] | ptrs[3]) % 16 == 0 else 2,) + fill(group, st, shared))
        for name, column in zip(_PER_STEP, zip(*rows)):  # one assignment per field: far cheaper than nine per record
            self.records[name] = column
        return grads

    def run(self, launch, scalars, max_norm=None, fixed_order=False):
        """upload the table, then -- ``max_norm`` given -- sum the squared gradient norm over EVERY tensor into an fp32 device scalar (``fixed_order``:
        per-chunk partials folded by one workgroup instead of fp32 atomics, bit-reproducible), then ``launch`` (``ops.adamw_multi`` /
        ``ops.nadamw_multi`` with the float arguments ``scalars``) over the update chunk list, which applies the clip.  Returns the scalar or None."""
        entries = self.table.upload()
        acc = None
        if max_norm is not None:
            acc = torch.zeros(1, dtype=torch.float32, device=entries.device)
            ws = torch.empty(self.chunks.shape[0], dtype=torch.float32, device=acc.device) if fixed_order else None
            ops.sumsq_multi(entries, self.chunks_dev, self.chunks.shape[0], acc, ws)
        if any(self.update):
            launch(entries, self.update_dev, self.update_chunks.shape[0], *scalars, acc, 0.0 if acc is None else float(max_norm))
        return acc
