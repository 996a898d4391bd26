"""The optimizers of the HIP path: the optimizer step of ``train.py:181-182`` -- gradient clipping, the update and the refresh
of the bf16 GEMM-operand copies of the weights -- as ONE launch over the whole model, and the reference's ``create_optimizer`` seam in front of them.

``NativeAdamW`` is a ``torch.optim.Optimizer`` with torch.optim.AdamW's semantics (decoupled weight decay, bias
correction; verified against it in tests/test_kernels_gpu.py).  Every step it describes the parameters to the device
as a table of 88-byte records (``ocn_adamw_multi``, include/openclip_hip.h) -- gradient pointers and per-group
learning rates change from step to step, the chunk list that cuts the tensors into 8192-element ranges / 64x64 tiles
does not -- and launches one kernel.  When the model's ``_WeightCache`` objects are passed (``weight_caches=``), the
kernel also rewrites the cached bf16 copies ([out,in] and the transposed [in,out]) in the same pass, so no cast
kernels run in the next forward.  ``grad_clip_norm`` fuses ``torch.nn.utils.clip_grad_norm_`` (train.py:181): one
multi-tensor sum of squares, the coefficient is applied inside the AdamW kernel (``.grad`` is left unscaled).

``NativeNAdamW`` is the reference's second built-in optimizer (optim.py:449-453: ``torch.optim.NAdam(decoupled_weight_decay=True)``) over the same
tables and the same kernel walk with another element update (``ocn_nadamw_multi``); ``nadam_schedule`` is its host-side momentum schedule.

``NativeMuon`` (below) is the third optimizer: momentum + Newton-Schulz orthogonalisation for the matrices (csrc/muon.hip), this file's AdamW tables for
every other parameter.

``create_optimizer(model, cfg)`` / ``OptimizerCfg`` mirror ``open_clip_train.optim.create_optimizer`` (optim.py:336-472) for a ``NativeCLIP``: the
reference's parameter groups -- ``make_wd_exclude`` (1-D parameters, ``no_weight_decay()`` names, ``--wd-exclude`` patterns), ``wd_param_groups``
(two / four buckets) and ``layer_decay_param_groups`` (layer-wise LR decay over the towers' ``layer_groups()``) -- restated here, then the native
optimizer that ``cfg.opt`` names.  ``param_groups_like_reference`` and ``muon_param_groups`` are the two fixed-shape callers of those builders."""
import fnmatch
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch

from . import ops, tables

DEFAULT_FALLBACK = ("token_embedding.weight", "positional_embedding", "visual.positional_embedding", "visual.class_embedding", "logit_scale", "logit_bias")


# ---- parameter groups (open_clip_train/optim.py:67-323) -----------------------------------------------------------------------------------
def unwrap_model(model):
    """the module behind DDP's ``.module`` and torch.compile's ``._orig_mod``, in any nesting: parameter names and tower discovery need the real one"""
    while True:
        inner = getattr(model, "_orig_mod", None)
        inner = getattr(model, "module", None) if inner is None else inner
        if inner is None:
            return model
        model = inner


def make_wd_exclude(model, extra_patterns=None):
    """``(name, param) -> bool``: does the parameter skip weight decay (optim.py:136-157)?  Yes for every parameter with at most one dimension, for
    the names any submodule declares through ``no_weight_decay()`` (taken relative to that submodule's path) and for full names that match one of
    ``extra_patterns`` (``--wd-exclude``; ``fnmatch.fnmatchcase``, so ``*`` spans dots)."""
    declared = set()
    for path, module in model.named_modules():
        names = getattr(module, "no_weight_decay", None)
        if callable(names):
            declared |= {(path + "." if path else "") + n for n in names()}
    patterns = tuple(extra_patterns or ())
    return lambda name, p: p.ndim <= 1 or name in declared or any(fnmatch.fnmatchcase(name, pat) for pat in patterns)


def make_fallback_fn(fallback_list):
    """``name -> bool`` from ``--opt-fallback-list``-style patterns (optim.py:392-394), or None for an empty list"""
    patterns = tuple(fallback_list or ())
    return (lambda name: any(fnmatch.fnmatchcase(name, pat) for pat in patterns)) if patterns else None


def _bucket_groups(model, weight_decay, exclude_fn, fallback_fn, scales):
    """the trainable parameters in ``named_parameters()`` order, bucketed by (lr_scale, no weight decay, fallback); ``scales``: None (no layer decay:
    the groups carry no ``lr_scale``) or ``{id(param): lr_scale}`` with 1.0 for whatever it does not list"""
    exclude_fn = exclude_fn or make_wd_exclude(model)
    buckets = {}
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        no_wd, fb = bool(exclude_fn(name, p)), bool(fallback_fn(name)) if fallback_fn else False
        scale = None if scales is None else scales.get(id(p), 1.0)
        key = (None if scale is None else round(scale, 8), no_wd, fb)
        if key not in buckets:
            group = {"params": [], "weight_decay": 0.0 if no_wd else weight_decay}
            label = ("no_wd" if no_wd else "wd") + ("/fallback" if fb else "")
            if scale is not None:
                group["lr_scale"], label = scale, f"lr_scale={scale:.4g}/{label}"
            group["group_name"] = label
            if fb:
                group["use_fallback"] = True
            buckets[key] = group
        buckets[key]["params"].append(p)
    return list(buckets.values())


def wd_param_groups(model, weight_decay, exclude_fn=None, fallback_fn=None):
    """optim.py:178-208: "no_wd" / "wd" in order of first appearance; with ``fallback_fn`` each splits again into a "/fallback" twin flagged
    ``use_fallback=True`` (the parameters a hybrid optimizer hands to its AdamW side)"""
    return _bucket_groups(model, weight_decay, exclude_fn, fallback_fn, None)


def layer_decay_param_groups(model, weight_decay, text_layer_decay=None, image_layer_decay=None, pooler_in_head=True, exclude_fn=None,
                             fallback_fn=None):
    """optim.py:247-323: layer-wise LR decay.  A tower with a decay gives group ``idx`` of its ``n`` ordered layer groups (``text_layer_groups`` /
    ``visual.layer_groups``: embeddings, blocks, projection) ``lr_scale = decay ** (n - 1 - idx)``; every other parameter keeps 1.0.  Inside each
    scale the weight-decay (and fallback) split holds; groups are named "lr_scale=<scale:.4g>/<wd|no_wd>[/fallback]" and sorted head first
    (``-lr_scale``, then name).  The scheduler multiplies a group's LR by its ``lr_scale`` (scheduler.py:6-15)."""
    scales = {}
    for decay, groups in ((text_layer_decay, model.text_layer_groups), (image_layer_decay, model.visual.layer_groups)):
        if not decay:
            continue
        groups = groups(pooler_in_head)
        for idx, (_, members) in enumerate(groups):
            for member in members:
                for p in ([member] if isinstance(member, torch.nn.Parameter) else member.parameters()):
                    scales[id(p)] = decay ** (len(groups) - 1 - idx)
    return sorted(_bucket_groups(model, weight_decay, exclude_fn, fallback_fn, scales), key=lambda g: (-g["lr_scale"], g["group_name"]))


def param_groups_like_reference(model, weight_decay=0.2):
    """the reference's default split (optim.py:67-77,178-208) in a fixed shape: [no weight decay, weight decay], either possibly empty"""
    model = unwrap_model(model)
    by_name = {g["group_name"]: g["params"] for g in wd_param_groups(model, weight_decay)}
    return [{"params": by_name.get("no_wd", []), "weight_decay": 0.0}, {"params": by_name.get("wd", []), "weight_decay": weight_decay}]


def muon_param_groups(model, weight_decay, fallback_list=DEFAULT_FALLBACK):
    """the reference's ``wd_param_groups(model, weight_decay, exclude_fn, fallback_fn)`` (optim.py:178-208) with ``fallback_fn`` built from
    ``--opt-fallback-list``-style patterns (optim.py:392-394: ``fnmatch.fnmatchcase`` on the full parameter name): up to four groups keyed by
    (no weight decay, fallback), named "no_wd" / "wd" (+ "/fallback"), the matched ones flagged ``use_fallback=True``.  The no-decay rule is
    ``param_groups_like_reference``'s (1-D parameters and ``no_weight_decay()`` names)."""
    model = unwrap_model(model)
    return wd_param_groups(model, weight_decay, None, make_fallback_fn(fallback_list))


def weight_caches_of(model):
    """the ``_WeightCache`` objects of a NativeCLIP (both towers), for ``NativeAdamW(weight_caches=...)``"""
    m = model.module if hasattr(model, "module") else model
    return [c for c in (getattr(m, "_cache", None), getattr(getattr(m, "visual", None), "_cache", None)) if c is not None]


# ---- AdamW / NAdamW: one launch over the whole model --------------------------------------------------------------------------------------
class _TableAdam(torch.optim.Optimizer):
    """what NativeAdamW and NativeNAdamW share: the per-parameter state, the plan (``tables.AdamTables``: records, modes, chunk list, operand copies,
    pinned upload), the fused clip and the launch.  A subclass names its entry point (``_LAUNCH``), its scalar state (``_SCALARS``: key -> (zero, type)),
    the group values every group must agree on because they are kernel arguments (``_shared_of``: (beta1, beta2, eps, ...)), and gives the four
    per-step floats of a record (``_fill``)."""
    _LAUNCH = _WHO = None
    _SCALARS = {"step": (0, int)}
    _SHARED_TEXT = "betas and eps"

    def _setup(self, grad_clip_norm, weight_caches, deterministic):
        self.grad_clip_norm = grad_clip_norm
        # the squared gradient norm of ``grad_clip_norm`` summed in a fixed order (per-chunk partials folded by one workgroup) instead of with
        # fp32 atomics: the optimizer's share of NativeCLIP(deterministic=True) -- the clipped update is then bit-reproducible too
        self.deterministic = bool(deterministic)
        self.weight_caches = list(weight_caches)
        self._plan_key = None
        self._plan = None
        self.last_grad_norm_sq = None  # device scalar of the most recent step when grad_clip_norm is set

    def _shared_of(self, group):
        b1, b2 = group["betas"]
        return float(b1), float(b2), float(group["eps"])

    def _kernel_scalars(self, shared):
        """the entry point's float arguments between ``n_chunks`` and ``gnorm_sq``"""
        return shared[:3]

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._plan = self._plan_key = None  # the moments are new tensors: rebuild the device table on the next step
        tables.scalars_to_host(self.state, {k: kind for k, (_, kind) in self._SCALARS.items()})

    @torch.no_grad()
    def _step_tables(self):
        active = [(g, p) for g in self.param_groups for p in g["params"] if p.grad is not None]
        if not active:
            return
        params = [p for _, p in active]
        copies = [tables.copies_of(self.weight_caches, p) for p in params]
        # the static part of the step (rebuilt when the set of tensors with a gradient, or the set of cached operand copies, changes)
        key = tuple((id(p), tuple(p.shape)) + (tuple(map(id, c)) if p.ndim in (2, 4) else ()) for p, c in zip(params, copies))
        if key != self._plan_key:
            self._plan, self._plan_key = tables.AdamTables(f"{self._WHO}: parameters and their moments must be contiguous", params, copies), key
            self._plan.to(params[0].device)
        plan = self._plan
        shared = self._shared_of(active[0][0])
        if any(self._shared_of(group) != shared for group in {id(g): g for g, _ in active}.values()):
            raise RuntimeError(f"{self._WHO}: all param groups must share {self._SHARED_TEXT}")
        grads = plan.refresh(active, self.state, self._SCALARS, self._fill, shared)  # held until the launches are queued
        acc = plan.run(self._LAUNCH, self._kernel_scalars(shared), self.grad_clip_norm, self.deterministic)
        if acc is not None:
            self.last_grad_norm_sq = acc
        tables.finish(params, plan.copies, self.weight_caches)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        self._step_tables()
        return loss


class NativeAdamW(_TableAdam):
    _LAUNCH, _WHO, _fill = staticmethod(ops.adamw_multi), "NativeAdamW (fused)", staticmethod(tables.adamw_fill)

    def __init__(self, params, lr=5e-4, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.2, grad_clip_norm=None, weight_caches=(),
                 fused=True, deterministic=False):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._setup(grad_clip_norm, weight_caches, deterministic)
        self.fused = fused

    # ---- per-tensor reference path (one ocn_adamw_step launch per tensor) ------------------------------------------
    @torch.no_grad()
    def _step_per_tensor(self):
        coef = None
        if self.grad_clip_norm is not None:
            acc = None
            for group in self.param_groups:
                for p in group["params"]:
                    if p.grad is not None:
                        acc = torch.zeros(1, dtype=torch.float32, device=p.device) if acc is None else acc
                        ops.sumsq_accum(p.grad.contiguous().view(-1), acc)
            if acc is not None:
                self.last_grad_norm_sq = acc
                coef = torch.clamp(self.grad_clip_norm / (acc.sqrt() + 1e-6), max=1.0)
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = tables.adam_state(self.state, p, self._SCALARS)
                st["step"] += 1
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                ops.adamw_step(p.view(-1), g.view(-1), st["exp_avg"].view(-1), st["exp_avg_sq"].view(-1), group["lr"], b1, b2,
                               group["eps"], group["weight_decay"], st["step"], clip_coef=coef)
                torch.autograd.graph.increment_version(p)  # raw-pointer update: let the bf16 weight cache see it

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        if self.fused:
            self._step_tables()
        else:
            self._step_per_tensor()
        return loss


def nadam_schedule(step, mu_product, lr, beta1, beta2, momentum_decay):
    """the host side of one NAdam step (torch/optim/nadam.py::_single_tensor_nadam), in Python floats: ``step`` is the 1-based number of the step
    being taken, ``mu_product`` the running product after the step before (1.0 at the start).  Returns ``(mu_product, c_g, c_m, bc2)``: the new
    product, the coefficients of ``g / den`` and ``m / den`` in the update, and ``1 - beta2^step`` (what ocn_nadamw_multi's record carries)."""
    mu = beta1 * (1.0 - 0.5 * 0.96 ** (step * momentum_decay))
    mu_next = beta1 * (1.0 - 0.5 * 0.96 ** ((step + 1) * momentum_decay))
    mu_product = mu_product * mu
    return mu_product, lr * (1.0 - mu) / (1.0 - mu_product), lr * mu_next / (1.0 - mu_product * mu_next), 1.0 - beta2 ** step


class NativeNAdamW(_TableAdam):
    """``torch.optim.NAdam(decoupled_weight_decay=True)`` -- the reference's ``--opt nadamw`` (optim.py:449-453) -- in NativeAdamW's one launch: fused
    clip, refreshed operand copies, bit-reproducible with ``deterministic=True``.  The defaults are torch's; state keys are torch's (``step``,
    ``mu_product``, ``exp_avg``, ``exp_avg_sq``; the two scalars are host numbers, a torch checkpoint's 0-d tensors are accepted).  ``lr`` is re-read
    every step, a group's extra keys (``lr_scale``, ``group_name``, ...) are carried untouched; ``betas``, ``eps`` and ``momentum_decay`` are kernel
    arguments and must agree across groups.  Only the decoupled form exists: the L2-coupled one is refused."""
    _LAUNCH, _WHO = staticmethod(ops.nadamw_multi), "NativeNAdamW"
    _SCALARS = {"step": (0, int), "mu_product": (1.0, float)}
    _SHARED_TEXT = "betas, eps and momentum_decay"

    def __init__(self, params, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, momentum_decay=4e-3, decoupled_weight_decay=True,
                 grad_clip_norm=None, weight_caches=(), deterministic=False):
        if not decoupled_weight_decay:
            raise ValueError("NativeNAdamW: decoupled_weight_decay=False (L2-coupled NAdam) is not implemented; the reference's nadamw is the decoupled form")
        if not (lr >= 0.0 and eps >= 0.0 and weight_decay >= 0.0 and momentum_decay >= 0.0 and 0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"NativeNAdamW: invalid hyper-parameters (lr={lr}, betas={betas}, eps={eps}, weight_decay={weight_decay}, "
                             f"momentum_decay={momentum_decay})")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, momentum_decay=momentum_decay,
                                      decoupled_weight_decay=True))
        self._setup(grad_clip_norm, weight_caches, deterministic)
        self._schedule = (None, None)  # (step, mu_product, lr) -> nadam_schedule's result, the most recent one

    def _shared_of(self, group):
        if not group.get("decoupled_weight_decay", True):  # a loaded torch checkpoint of the L2-coupled form
            raise RuntimeError("NativeNAdamW: a param group asks for decoupled_weight_decay=False, which is not implemented")
        return super()._shared_of(group) + (float(group["momentum_decay"]),)

    def _kernel_scalars(self, shared):
        b1, b2, eps = shared[:3]
        return 1.0 - b1, b2, 1.0 - b2, eps  # 1 - beta formed in double, as torch forms it (include/openclip_hip.h says what the fp32 difference costs)

    def _fill(self, group, st, shared):
        """decay, bc2, c_g, c_m: the record's four floats as ocn_nadamw_multi reads them"""
        lr = group["lr"]
        key = (st["step"], st["mu_product"], lr)
        if key != self._schedule[0]:  # the parameters of a group (usually of the whole model) are at the same point of the schedule: evaluate it once
            self._schedule = (key, nadam_schedule(*key, shared[0], shared[1], shared[3]))
        st["mu_product"], c_g, c_m, bc2 = self._schedule[1]
        return 1.0 - lr * group["weight_decay"], bc2, c_g, c_m


# ---- Muon -------------------------------------------------------------------------------------------------------------------------------
# Momentum + Newton-Schulz orthogonalisation for the 2-D hidden weights, AdamW for everything else (csrc/muon.hip states the arithmetic).
NS_COEFFS = (3.4445, -4.7750, 2.0315)
ADJUST_LR = ("match_rms_adamw", "original")
_MUON_ENTRY = np.dtype([("g", "<u8"), ("buf", "<u8"), ("w", "<u8"), ("w16n", "<u8"), ("w16t", "<u8"), ("xn", "<u8"), ("xt", "<u8"), ("xfin", "<u8"),
                        ("rows", "<i4"), ("cols", "<i4"), ("ldn", "<i4"), ("ldt", "<i4"), ("chunk0", "<i4"), ("nchunks", "<i4"),
                        ("step", "<f4"), ("decay", "<f4")])
assert _MUON_ENTRY.itemsize == 96


def takes_muon(group, p):
    """the routing rule: a parameter of a group without a truthy ``use_fallback`` takes the Muon update if it has at least two dimensions"""
    return not group.get("use_fallback") and p.ndim >= 2


def muon_lr_scale(adjust_lr, rows, cols):
    if adjust_lr == "match_rms_adamw":
        return 0.2 * max(rows, cols) ** 0.5
    if adjust_lr == "original":
        return max(1.0, rows / cols) ** 0.5
    raise ValueError(f"NativeMuon: adjust_lr must be one of {ADJUST_LR} (got {adjust_lr!r})")


def _pad32(n):
    return (n + 31) // 32 * 32


class NativeMuon(torch.optim.Optimizer):
    """Muon for the matrices, AdamW for the rest, in a fixed number of launches per step.

    Routing (``takes_muon``): a parameter with ``ndim >= 2`` in a group without a truthy ``use_fallback`` takes the Muon update -- a 4-D weight as
    ``[shape[0], -1]``, ``in_proj_weight`` as one ``[3C, C]`` matrix; every other parameter takes AdamW through the tables of ``NativeAdamW``
    (``ocn_adamw_multi``) with the group's ``lr * fallback_lr_scale``, ``betas``, ``eps`` and ``weight_decay``.  Group keys such as ``group_name`` and
    ``lr_scale`` are carried and ignored; ``lr`` is re-read every step.  ``grad_clip_norm`` is the coefficient of the global norm over ALL parameters,
    summed in a fixed order; ``.grad`` stays unscaled.  Nothing on the Muon path uses an fp32 atomic: a step is bit-reproducible.

    The Newton-Schulz products of all equal-shape matrices run as three ``ocn_gemm_nt_batched`` launches per iteration (``_backend="batched"``);
    ``_backend="per_matrix"`` sends one matrix at a time through ``ocn_gemm_nt`` (cross-check and timing comparison)."""

    def __init__(self, params, lr=0.02, weight_decay=0.0, momentum=0.95, nesterov=True, ns_steps=5, adjust_lr="match_rms_adamw", betas=(0.9, 0.95),
                 eps=1e-8, fallback_lr_scale=1.0, grad_clip_norm=None, weight_caches=(), _backend="batched"):
        if adjust_lr not in ADJUST_LR:
            raise ValueError(f"NativeMuon: adjust_lr must be one of {ADJUST_LR} (got {adjust_lr!r})")
        if int(ns_steps) != ns_steps or ns_steps < 1:
            raise ValueError(f"NativeMuon: ns_steps must be an integer >= 1 (got {ns_steps!r})")
        if not 0.0 <= momentum < 1.0:
            raise ValueError(f"NativeMuon: momentum must lie in [0, 1) (got {momentum!r})")
        if _backend not in ("batched", "per_matrix"):
            raise ValueError(f"NativeMuon: unknown backend {_backend!r}")
        super().__init__(params, dict(lr=lr, weight_decay=weight_decay, momentum=momentum, nesterov=bool(nesterov), ns_steps=int(ns_steps),
                                      adjust_lr=adjust_lr, betas=tuple(betas), eps=eps, fallback_lr_scale=fallback_lr_scale))
        self.grad_clip_norm = grad_clip_norm
        self.weight_caches = list(weight_caches)
        self._backend = _backend
        self._plan = self._plan_key = None
        self.last_grad_norm_sq = None  # device scalar of the most recent step when grad_clip_norm is set

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._plan = self._plan_key = None
        tables.scalars_to_host(self.state, {"step": int})

    @staticmethod
    def _adam_tables(active, copies):
        """AdamEntry records of EVERY active parameter, flat (never in tile mode): the squared gradient norm runs over all of them, AdamW over the
        fallback ones, whose transposed copies stay on the cast path; a Muon matrix's copies are rewritten by ocn_muon_apply_multi instead"""
        is_muon = [takes_muon(g, p) for g, p in active]
        return tables.AdamTables("NativeMuon: the AdamW moments must be contiguous", [p for _, p in active],
                                 [(None, None) if m else c for m, c in zip(is_muon, copies)], tiles=False, update=[not m for m in is_muon])

    @staticmethod
    def _fallback_fill(group, st, shared):
        return tables.adamw_fill({"lr": group["lr"] * group["fallback_lr_scale"], "weight_decay": group["weight_decay"]}, st, shared)

    def _build_plan(self, active, copies, ns_steps):
        """static part of the step: the AdamW-side tables, the Newton-Schulz workspace per padded shape, chunk lists, which operand copies are rewritten"""
        dev = active[0][1].device
        muon = [i for i, (g, p) in enumerate(active) if takes_muon(g, p)]
        adam = self._adam_tables(active, copies).to(dev)
        plan = {"muon": muon, "adam": adam, "copies": list(adam.copies)}
        if not muon:
            return plan
        # Muon: matrices stacked by padded [min, max] shape; X and its transpose ping-pong between two buffers (a product reads one while it writes the other)
        by_shape = {}
        for j, i in enumerate(muon):
            p = active[i][1]
            rows, cols = p.shape[0], p.numel() // p.shape[0]
            by_shape.setdefault((_pad32(min(rows, cols)), _pad32(max(rows, cols))), []).append(j)
        ment = np.zeros(len(muon), dtype=_MUON_ENTRY)
        bf = lambda *s: torch.empty(s, dtype=torch.bfloat16, device=dev)
        groups = []
        for (mp, np_), members in by_shape.items():
            b = len(members)
            ws = {"X": [bf(b, mp, np_), bf(b, mp, np_)], "Xt": [bf(b, np_, mp), bf(b, np_, mp)], "A": bf(b, mp, mp), "B": bf(b, mp, mp), "tall": False}
            if self._backend == "per_matrix":
                ws["acc_mm"] = torch.empty(mp, mp, dtype=torch.float32, device=dev)
                ws["acc_mn"] = torch.empty(mp, np_, dtype=torch.float32, device=dev)
            for slot, j in enumerate(members):
                p = active[muon[j]][1]
                rows, cols = p.shape[0], p.numel() // p.shape[0]
                tall = rows > cols
                ws["tall"] = ws["tall"] or tall
                nat, tr = (ws["Xt"], ws["X"]) if tall else (ws["X"], ws["Xt"])  # the weight-oriented image and the other one
                n16, t16 = copies[muon[j]]
                if t16 is not None and not (rows % 64 == 0 and cols % 64 == 0):  # odd-shaped weight: keep its transposed copy on the cast path
                    t16 = None
                plan["copies"][muon[j]] = (n16, t16)
                e = ment[j]
                e["w16n"] = 0 if n16 is None else n16.data_ptr()
                e["w16t"] = 0 if t16 is None else t16.data_ptr()
                e["xn"], e["xt"], e["xfin"] = nat[0][slot].data_ptr(), tr[0][slot].data_ptr(), nat[ns_steps % 2][slot].data_ptr()
                e["rows"], e["cols"], e["ldn"], e["ldt"] = rows, cols, _pad32(cols), _pad32(rows)
                e["nchunks"] = -(-rows // 64) * -(-cols // 64)
            groups.append(ws)
        chunks = tables.chunk_list(ment["nchunks"])
        ment["chunk0"] = np.cumsum(ment["nchunks"]) - ment["nchunks"]
        plan.update(table=tables.PinnedTable(ment, dev), groups=groups, chunks=torch.from_numpy(chunks).to(dev), n_chunks=int(chunks.shape[0]),
                    chunk_ws=torch.empty(chunks.shape[0], dtype=torch.float32, device=dev),
                    inv_norm=torch.empty(len(muon), dtype=torch.float32, device=dev))
        return plan

    def _newton_schulz(self, ws, ns_steps):
        a, b, c = NS_COEFFS
        X, Xt, A, B = ws["X"], ws["Xt"], ws["A"], ws["B"]
        for it in range(ns_steps):
            cur, nxt = it % 2, 1 - it % 2
            want_t = it + 1 < ns_steps or ws["tall"]  # the last iterate's transposed image is read only by tall weights (ocn_muon_apply_multi)
            if self._backend == "batched":
                ops.gemm_nt_batched(X[cur], X[cur], A)                                     # A = X X^T
                ops.gemm_nt_batched(A, A, B, resid=A, alpha=c, beta=b)                     # B = b A + c A A   (A is symmetric to the bit)
                ops.gemm_nt_batched(B, Xt[cur], X[nxt], resid=X[cur], out_t=Xt[nxt] if want_t else None, alpha=1.0, beta=a)  # X = a X + B X
                continue
            for i in range(A.shape[0]):
                ops.gemm_nt(ops.EPI_BF16, X[cur][i], X[cur][i], A[i])
                ops.gemm_nt(ops.EPI_F32, A[i], A[i], ws["acc_mm"], alpha=c)
                ops.muon_axpby(ws["acc_mm"], A[i], B[i], None, beta=b)
                ops.gemm_nt(ops.EPI_F32, B[i], Xt[cur][i], ws["acc_mn"])
                ops.muon_axpby(ws["acc_mn"], X[cur][i], X[nxt][i], Xt[nxt][i] if want_t else None, beta=a)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        active = [(g, p) for g in self.param_groups for p in g["params"] if p.grad is not None]
        if not active:
            return loss
        mgroups = [g for g, p in active if takes_muon(g, p)]
        momentum, nesterov, ns_steps = (mgroups[0]["momentum"], mgroups[0]["nesterov"], mgroups[0]["ns_steps"]) if mgroups else (0.0, False, 1)
        copies = [tables.copies_of(self.weight_caches, p) for _, p in active]
        key = (ns_steps,) + tuple((id(p), tuple(p.shape), takes_muon(g, p)) + tuple(map(id, c)) for (g, p), c in zip(active, copies))
        if key != self._plan_key:
            self._plan, self._plan_key = self._build_plan(active, copies, ns_steps), key
        plan = self._plan
        fb_hyper = None
        for group, p in active:
            if not p.is_contiguous() or p.grad.dtype != torch.float32 or p.dtype != torch.float32:
                raise RuntimeError("NativeMuon: parameters must be contiguous fp32 tensors with fp32 gradients")
            if not takes_muon(group, p):
                hyper = (*group["betas"], group["eps"])
                if fb_hyper is not None and fb_hyper != hyper:
                    raise RuntimeError("NativeMuon: all AdamW (fallback) parameters must share betas and eps")
                fb_hyper = hyper
        adam = plan["adam"]
        grads = adam.refresh(active, self.state, {"step": (0, int)}, self._fallback_fill, fb_hyper)
        acc = adam.run(ops.adamw_multi, fb_hyper or (), self.grad_clip_norm, True)  # the norm over all, AdamW over the fallback ones (if any)
        max_norm = 0.0 if acc is None else float(self.grad_clip_norm)
        if acc is not None:
            self.last_grad_norm_sq = acc
        if plan["muon"]:
            ment = plan["table"].records
            for j, i in enumerate(plan["muon"]):
                group, p = active[i]
                if (group["momentum"], group["nesterov"], group["ns_steps"]) != (momentum, nesterov, ns_steps):
                    raise RuntimeError("NativeMuon: all Muon groups must share momentum, nesterov and ns_steps")
                buf = self.state[p].get("momentum_buffer")
                if buf is None:
                    buf = self.state[p]["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                if buf.device != p.device or buf.dtype != torch.float32 or not buf.is_contiguous():
                    buf = self.state[p]["momentum_buffer"] = buf.to(p.device, torch.float32).contiguous()
                e = ment[j]
                e["g"], e["buf"], e["w"] = grads[i].data_ptr(), buf.data_ptr(), p.data_ptr()
                e["step"] = group["lr"] * muon_lr_scale(group["adjust_lr"], int(e["rows"]), int(e["cols"]))
                e["decay"] = 1.0 - group["lr"] * group["weight_decay"]
            mdev = plan["table"].upload()
            ops.muon_momentum_multi(mdev, len(plan["muon"]), plan["chunks"], plan["n_chunks"], momentum, nesterov, acc, max_norm, plan["chunk_ws"],
                                    plan["inv_norm"])
            ops.muon_normalize_multi(mdev, plan["chunks"], plan["n_chunks"], momentum, nesterov, acc, max_norm, plan["inv_norm"])
            for ws in plan["groups"]:
                self._newton_schulz(ws, ns_steps)
            ops.muon_apply_multi(mdev, plan["chunks"], plan["n_chunks"])
        tables.finish([p for _, p in active], plan["copies"], self.weight_caches)
        return loss


# ---- create_optimizer (open_clip_train/optim.py:24-64, 336-472) ---------------------------------------------------------------------------
@dataclass
class OptimizerCfg:
    """the reference's typed optimizer configuration, field for field (optim.py:51-64); ``create_optimizer`` reads it by attribute, so the
    reference's own instance serves as well.  ``opt``: "adamw", "nadamw" or "muon"."""
    opt: str = "adamw"
    lr: float = 5e-4
    weight_decay: float = 0.2
    beta1: Optional[float] = None
    beta2: Optional[float] = None
    eps: Optional[float] = None
    momentum: Optional[float] = None
    opt_kwargs: dict = field(default_factory=dict)
    text_layer_decay: Optional[float] = None
    image_layer_decay: Optional[float] = None
    audio_layer_decay: Optional[float] = None
    pooler_in_head: bool = True
    wd_exclude_patterns: List[str] = field(default_factory=list)
    fallback_list: Optional[List[str]] = None


def create_optimizer(model, cfg, device=None, tensorize=False, *, grad_clip_norm=None, deterministic=False):
    """``open_clip_train.optim.create_optimizer(model, cfg, device, tensorize)`` for a ``NativeCLIP`` (possibly behind DDP / torch.compile): the
    reference's parameter groups, the native optimizer ``cfg.opt`` names -- "adamw" -> NativeAdamW, "nadamw" -> NativeNAdamW, "muon" -> NativeMuon
    (``cfg.fallback_list``, default ``DEFAULT_FALLBACK``, names its AdamW side) -- wired to the model's operand-copy caches, and every group's
    initial ``lr = cfg.lr * lr_scale``.  ``grad_clip_norm`` / ``deterministic`` are native extras: the clip of train.py:181 fused into the step, and
    the fixed-order norm.  Whatever the native path does not build raises by name."""
    from .model import NativeCLIP
    model = unwrap_model(model)
    if not isinstance(model, NativeCLIP):
        raise TypeError(f"open_clip_amd.create_optimizer groups a NativeCLIP (got {type(model).__name__}); other models go through "
                        "open_clip_train.optim.create_optimizer")
    if tensorize:
        raise NotImplementedError("open_clip_amd.create_optimizer: tensorize=True (learning rates as device tensors, for torch.compile's step "
                                  "strategy) is not implemented: the native optimizers read `lr` as a host float every step")
    opt = cfg.opt.lower()
    decays = {"text": getattr(cfg, "text_layer_decay", None), "image": getattr(cfg, "image_layer_decay", None),
              "audio": getattr(cfg, "audio_layer_decay", None)}
    for name, decay in decays.items():
        if decay is not None and not (0.0 < decay <= 1.0):
            raise ValueError(f"--{name}-layer-decay must be in (0, 1], got {decay}.")
    decays = {name: (decay if decay and decay != 1.0 else None) for name, decay in decays.items()}
    if decays["audio"] is not None:
        raise ValueError(f"audio_layer_decay={decays['audio']}: a NativeCLIP has no audio tower (--audio-layer-decay applies to CLAP models)")
    extra = dict(getattr(cfg, "opt_kwargs", None) or {})
    fallback_list = getattr(cfg, "fallback_list", None) or extra.pop("fallback_list", None)
    if opt.startswith("timm/"):
        raise NotImplementedError(f"open_clip_amd.create_optimizer: the timm optimizer '{cfg.opt}' has no native counterpart (adamw, nadamw and muon "
                                  "do); build it with open_clip_train.optim.create_optimizer")
    if opt not in ("adamw", "nadamw", "muon"):
        raise ValueError(f"Unknown optimizer {opt}")
    if fallback_list and opt != "muon":
        raise ValueError(f"fallback_list (--opt-fallback-list) only applies to a hybrid optimizer (muon), not '{cfg.opt}'.")
    if opt == "muon":
        fallback_list = fallback_list or DEFAULT_FALLBACK
    exclude_fn = make_wd_exclude(model, getattr(cfg, "wd_exclude_patterns", None))
    fallback_fn = make_fallback_fn(fallback_list)
    if decays["text"] or decays["image"]:
        groups = layer_decay_param_groups(model, cfg.weight_decay, decays["text"], decays["image"], getattr(cfg, "pooler_in_head", True), exclude_fn,
                                          fallback_fn)
    else:
        groups = wd_param_groups(model, cfg.weight_decay, exclude_fn, fallback_fn)
    if (cfg.beta1 is None) != (cfg.beta2 is None):
        raise ValueError("BOTH beta1 and beta2 must be specified (or neither).")
    kwargs = {"lr": cfg.lr}
    if cfg.beta1 is not None:
        kwargs["betas"] = (cfg.beta1, cfg.beta2)
    if cfg.eps is not None:
        kwargs["eps"] = cfg.eps
    if opt == "muon" and getattr(cfg, "momentum", None) is not None:
        kwargs["momentum"] = cfg.momentum
    if opt != "muon":  # NativeMuon has no switch: its norm is always summed in a fixed order
        kwargs["deterministic"] = deterministic
    kwargs.update(weight_caches=weight_caches_of(model), grad_clip_norm=grad_clip_norm)
    kwargs.update(extra)  # merged last, as the reference does
    optimizer = {"adamw": NativeAdamW, "nadamw": NativeNAdamW, "muon": NativeMuon}[opt](groups, **kwargs)
    for group in optimizer.param_groups:  # optim.py:461 / scheduler.py:6-15: layer decay holds before the first scheduler step
        group["lr"] = cfg.lr * group.get("lr_scale", 1.0)
    return optimizer
