"""The cases behind tests/golden/optim_parent.npz: three optimizer steps (or three EMA updates) on inputs drawn from a seeded CPU generator, through
the public interface only -- ``NativeAdamW``, ``NativeNAdamW``, ``NativeMuon``, ``NativeModelEma``, ``ema_plan`` + ``ops.ema_lerp_multi`` and
``_WeightCache`` -- on the smallest shapes that reach every path of the table kernels (tile mode with an unaligned gradient, vector path with a tail
in a second chunk, scalar path, 0-d; Muon's batch of two, tall, ragged and 4-D matrices with its AdamW side; EMA slots on and off the 16-byte grid).

``run_golden_case`` returns EVERY array a case leaves behind: parameters, state tensors, the cached ``n`` / ``t`` operand copies as the next forward
would read them, ``last_grad_norm_sq`` where a clip is set.  Only bit-stable configurations are in: AdamW / NAdamW clip with ``deterministic=True``
(the other form sums with fp32 atomics), Muon is always fixed-order.

The fixture holds one SHA-256 per array (``digest``: over dtype, shape and bytes), not the bytes themselves: the arrays of all cases are 3 MB of
full-mantissa floats that no compressor shrinks, against the 1 MiB a committed file may have.  A digest misses no changed byte; what it cannot say is
how many changed -- ``tools/optim_golden.py --full`` writes the bytes themselves for that comparison."""
import hashlib
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optim_parent.npz")

# tile mode, gradient a view at a 4-byte offset | tile mode | 4-D weight as a [64, 64] tile | not 64-divisible: `n` refreshed in place, `t` re-cast |
# vector path, second chunk = one vector + a 3-element tail | scalar path (gradient at a 4-byte offset), two chunks | 0-d | below one chunk
ADAM_SHAPES = [(64, 128), (128, 64), (64, 1, 8, 8), (50, 72), (8199,), (8197,), (), (40,)]
ADAM_OFFSET_GRADS = (0, 5)
ADAM_HYPER = dict(betas=(0.9, 0.98), eps=1e-6)
# a batch of two | tall, both copies | ragged, padded to 32 | 4-D || the AdamW side: vector path with an offset gradient, below one chunk, 0-d
MUON_SHAPES = [(64, 128), (64, 128), (128, 64), (96, 40), (64, 1, 8, 8), (8199,), (40,), ()]
MUON_COPIES, MUON_OFFSET_GRADS, MUON_N_MATRICES = (2,), (5,), 5
EMA_NUMELS = [1, 4, 8191, 8192, 8193]
EMA_WEIGHTS = (0.25, 1e-4, 1.0)
EMA_GAP = 8
CLIP = 0.7


def digest(a):
    a = np.ascontiguousarray(a)
    h = hashlib.sha256(f"{a.dtype.str}{a.shape}".encode())
    h.update(a.tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def adam_groups(params):
    """every parameter a group of its own, alternating ``lr``, weight decay by dimension (as tests/test_nadamw_gpu.py::_groups)"""
    return [{"params": [p], "weight_decay": 0.0 if p.ndim <= 1 else 0.2, "lr": 1e-2 * (1 + i % 2)} for i, p in enumerate(params)]


def golden_cases():
    return [{"name": "adamw", "kind": "adam", "opt": "NativeAdamW", "clip": None},
            {"name": "adamw_clip", "kind": "adam", "opt": "NativeAdamW", "clip": CLIP},
            {"name": "nadamw_clip", "kind": "adam", "opt": "NativeNAdamW", "clip": CLIP},
            {"name": "muon", "kind": "muon"},
            {"name": "ema_aligned", "kind": "ema_slots", "shift": 0},
            {"name": "ema_offset", "kind": "ema_slots", "shift": 1},
            {"name": "ema_module", "kind": "ema_module"}]


def _np(t):
    t = t.detach()
    return (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy().copy()


def _set_grads(params, offset, gen, dev, step):
    for i, p in enumerate(params):
        gr = torch.randn(p.shape, generator=gen).to(dev) * (0.1 + step)
        if i in offset:  # a view at a 4-byte offset (a DDP bucket view)
            buf = torch.empty(gr.numel() + 1, device=dev)
            buf[1:].copy_(gr.flatten())
            p.grad = buf[1:].view(p.shape)
        else:
            p.grad = gr.clone()


def _collect(out, opt, params, cache, held):
    for i, p in enumerate(params):
        out[f"p{i}"] = _np(p)
        for k, v in sorted(opt.state[p].items()):
            out[f"p{i}/{k}"] = _np(v) if torch.is_tensor(v) else np.asarray(v, dtype=np.float64)
        for kind in "nt":
            if held[i][kind] is not None:
                got = cache.get(p, kind)  # what the next forward reads: the copy the step rewrote, or a new cast
                out[f"p{i}/{kind}"] = _np(got)
                out[f"p{i}/{kind}_in_place"] = np.asarray(got is held[i][kind], dtype=np.uint8)
    if opt.grad_clip_norm is not None:
        out["last_grad_norm_sq"] = _np(opt.last_grad_norm_sq)
    return out


def _run_steps(shapes, copies, offset, make_opt, dev, seed):
    from open_clip_amd.model import _WeightCache
    gen = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(sh, generator=gen).to(dev)) for sh in shapes]
    cache = _WeightCache()
    held = [{kind: (cache.get(p, kind) if i in copies else None) for kind in "nt"} for i, p in enumerate(params)]
    opt = make_opt(params, cache)
    for step in range(3):
        _set_grads(params, offset, gen, dev, step)
        opt.step()
    torch.cuda.synchronize()
    return _collect({}, opt, params, cache, held)


def _run_adam(case, dev):
    from open_clip_amd import optim
    extra = {} if case["clip"] is None else dict(grad_clip_norm=case["clip"], deterministic=True)
    make = lambda params, cache: getattr(optim, case["opt"])(adam_groups(params), lr=1e-2, weight_caches=[cache], **ADAM_HYPER, **extra)
    return _run_steps(ADAM_SHAPES, [i for i, sh in enumerate(ADAM_SHAPES) if len(sh) in (2, 4)], ADAM_OFFSET_GRADS, make, dev, seed=5)


def _run_muon(case, dev):
    from open_clip_amd.optim import NativeMuon

    def make(params, cache):
        groups = [{"params": params[:MUON_N_MATRICES], "weight_decay": 0.1}, {"params": params[MUON_N_MATRICES:], "weight_decay": 0.0, "lr": 0.01, "use_fallback": True}]
        return NativeMuon(groups, lr=0.02, nesterov=True, fallback_lr_scale=0.5, grad_clip_norm=CLIP, weight_caches=[cache], _backend="batched",
                          **ADAM_HYPER)
    return _run_steps(MUON_SHAPES, MUON_COPIES, MUON_OFFSET_GRADS, make, dev, seed=6)


def ema_slots(shift):
    """(offset, numel) of every slot inside one flat buffer, in floats: starts on the 16-byte grid plus ``shift`` floats, EMA_GAP canaries between"""
    slots, pos = [], EMA_GAP
    for n in EMA_NUMELS:
        pos = (pos + 3) // 4 * 4
        slots.append((pos + shift, n))
        pos += shift + n + EMA_GAP
    return slots, pos


def _run_ema_slots(case, dev):
    from open_clip_amd import ops
    from open_clip_amd.ema import ema_plan
    gen = torch.Generator().manual_seed(11)
    slots, total = ema_slots(case["shift"])
    e, s = torch.randn(total, generator=gen).to(dev), torch.randn(total, generator=gen).to(dev)
    assert e.data_ptr() % 16 == 0 and s.data_ptr() % 16 == 0
    ent, chunks = ema_plan([(e.data_ptr() + 4 * o, s.data_ptr() + 4 * o, n) for o, n in slots])
    assert ent["mode"].tolist() == [2 if case["shift"] else 0] * len(slots) and chunks.shape[0] == 6
    entries, chunks_dev = torch.from_numpy(ent.view(np.uint8).reshape(-1).copy()).to(dev), torch.from_numpy(chunks).to(dev)
    out = {}
    for k, weight in enumerate(EMA_WEIGHTS):  # the whole buffer after every update: the slots and the floats between them
        ops.ema_lerp_multi(entries, chunks_dev, int(chunks.shape[0]), weight)
        torch.cuda.synchronize()
        out[f"ema{k}"] = _np(e)
    out["src"] = _np(s)
    return out


def _run_ema_module(case, dev):
    from open_clip_amd import NativeModelEma
    gen = torch.Generator().manual_seed(12)
    model = torch.nn.Linear(72, 50)
    draw = lambda: {k: torch.randn(v.shape, generator=gen) for k, v in model.state_dict().items()}
    model.load_state_dict(draw())
    model = model.to(dev)
    ema = NativeModelEma(model, decay=0.9)
    out = {}
    for k, step in enumerate((1, 2, None)):  # update(step=1): the copy; update(step=2): decay 0.9; set()
        model.load_state_dict(draw())
        ema.update(model, step=step) if step is not None else ema.set(model)
        torch.cuda.synchronize()
        for name, v in ema.module.state_dict().items():
            out[f"{name}{k}"] = _np(v)
    return out


def run_golden_case(case, dev):
    """one case of ``golden_cases()`` on device ``dev`` -> {array name: numpy array}"""
    return {"adam": _run_adam, "muon": _run_muon, "ema_slots": _run_ema_slots, "ema_module": _run_ema_module}[case["kind"]](case, dev)


def run_all(dev):
    """{"<case>/<array>": array} over every case"""
    return {f"{case['name']}/{k}": v for case in golden_cases() for k, v in run_golden_case(case, dev).items()}
