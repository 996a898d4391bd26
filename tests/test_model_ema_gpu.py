"""MI355X: ``ocn_ema_lerp_multi`` against the float64 oracle of tests/model_ema_util.py (bound 2^-22 (|e| + |p|) per element, derived there), its exact
limits, and ``NativeModelEma`` / ``setup_ema`` on the tiny model: the trajectory of three training steps, the twin's operand caches, moved parameter
storage, and the reference's ``CLIPTask`` evaluating and checkpointing the twin."""
import numpy as np
import pytest
import torch

from open_clip_amd.configs import get_model_config
from open_clip_amd.synth import init_state_dict, synthetic_batch
from oracle.ref_shim import import_reference, reference_importable
from tests.model_ema_util import assert_within, lerp_bound, lerp_oracle
from tests.test_kernels_gpu import dev  # noqa: F401  (the module fixture that loads the library)

pytestmark = pytest.mark.gpu

# vector path: below one vector, the numel % 4 tails, around the chunk edge, several chunks with a tail | the last pair sits one float off the
# 16-byte grid on both sides (scalar path, more than one chunk)
NUMELS = [1, 3, 4, 5, 8191, 8192, 8193, 3 * 8192 + 2]
OFFSET_NUMEL = 8197
CANARY_E, CANARY_S, GAP = 12345.0, -54321.0, 8


class _Arena:
    """every tensor of the table inside ONE buffer per side, 16-byte aligned slots (the last one a float further) with canary floats between, in
    front and behind; ``fresh()`` gives new device copies of the same values and the launch tables for them"""

    def __init__(self, dev):  # noqa: F811
        g = torch.Generator().manual_seed(11)
        self.dev, self.slots, pos = dev, [], GAP
        for i, n in enumerate(NUMELS + [OFFSET_NUMEL]):
            pos = (pos + 3) // 4 * 4 + (1 if i == len(NUMELS) else 0)
            self.slots.append((pos, n))
            pos += n + GAP
        self.total = pos
        self.e0 = torch.full((self.total,), CANARY_E)
        self.s0 = torch.full((self.total,), CANARY_S)
        self.inside = torch.zeros(self.total, dtype=torch.bool)
        for o, n in self.slots:
            self.e0[o:o + n] = torch.randn(n, generator=g)
            self.s0[o:o + n] = torch.randn(n, generator=g)
            self.inside[o:o + n] = True

    def fresh(self):
        from open_clip_amd.ema import ema_plan
        e, s = self.e0.to(self.dev), self.s0.to(self.dev)
        assert e.data_ptr() % 16 == 0 and s.data_ptr() % 16 == 0
        ent, chunks = ema_plan([(e.data_ptr() + 4 * o, s.data_ptr() + 4 * o, n) for o, n in self.slots])
        assert ent["mode"].tolist() == [0] * len(NUMELS) + [2] and chunks.shape[0] == 6 + 2 + 4 + 2
        entries = torch.from_numpy(ent.view(np.uint8).reshape(-1).copy()).to(self.dev)
        return e, s, entries, torch.from_numpy(chunks).to(self.dev), int(chunks.shape[0])

    def run(self, weight):
        from open_clip_amd import ops
        e, s, entries, chunks, n = self.fresh()
        ops.ema_lerp_multi(entries, chunks, n, weight)
        torch.cuda.synchronize()
        return e.cpu(), s.cpu()


@pytest.fixture(scope="module")
def arena(dev):  # noqa: F811
    return _Arena(dev)


@pytest.mark.parametrize("weight", [1e-4, 0.48, 0.63])
def test_kernel_against_the_float64_oracle(arena, weight):
    got, src = arena.run(weight)
    assert torch.equal(src, arena.s0), "the source side was written"
    assert torch.equal(got[~arena.inside], arena.e0[~arena.inside]), "a canary between / behind the tensors was overwritten"
    w32 = float(np.float32(weight))
    for o, n in arena.slots:
        e, p = arena.e0[o:o + n], arena.s0[o:o + n]
        assert_within(f"ema_lerp_multi weight {weight} numel {n}", got[o:o + n], lerp_oracle(e, p, 1.0 - weight), lerp_bound(e, p))
        # and the update is an update: the mean step is weight * |p - e|, far above the bound
        assert float((got[o:o + n] - e).abs().sum()) >= 0.5 * w32 * float((p - e).abs().sum())


def test_exact_limits_and_reproducible_bits(arena):
    got, _ = arena.run(1.0)
    for o, n in arena.slots:
        assert torch.equal(got[o:o + n], arena.s0[o:o + n]), n
    assert torch.equal(got[~arena.inside], arena.e0[~arena.inside])
    got, _ = arena.run(0.0)
    assert torch.equal(got, arena.e0)
    for weight in (1e-4, 0.63):
        a, b = arena.run(weight)[0], arena.run(weight)[0]
        assert torch.equal(a, b), weight


# ---- NativeModelEma on the tiny model -------------------------------------------------------------------------------------------------------
def _tiny(state, cfg):
    from open_clip_amd.model import NativeCLIP
    m = NativeCLIP(cfg["embed_dim"], cfg["vision_cfg"], cfg["text_cfg"], output_dict=True, deterministic=True)
    m.load_state_dict(state, strict=True)
    return m.cuda().train()


@pytest.fixture(scope="module")
def tiny(dev):  # noqa: F811
    cfg = get_model_config("tiny-test")
    return cfg, init_state_dict(cfg, seed=4, perturb=True), [synthetic_batch(cfg, 8, seed=12 + i, device="cuda") for i in range(4)]


def _train_step(model, opt, batch):
    from open_clip_amd.loss import NativeClipLoss
    model.zero_grad(set_to_none=True)
    NativeClipLoss(deterministic=True)(**model(image=batch["image"], text=batch["text"])).backward()
    opt.step()


def _adamw(model, lr=1e-3):
    from open_clip_amd.optim import NativeAdamW, param_groups_like_reference, weight_caches_of
    return NativeAdamW(param_groups_like_reference(model, 0.2), lr=lr, betas=(0.9, 0.98), eps=1e-6, weight_caches=weight_caches_of(model))


def _features(model, batch):
    with torch.no_grad():
        out = model(image=batch["image"], text=batch["text"])
    return out["image_features"].clone(), out["text_features"].clone()


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_trajectory_over_three_training_steps(tiny):
    from open_clip_amd import NativeModelEma
    cfg, state, batches = tiny
    model = _tiny(state, cfg)
    opt = _adamw(model)
    ema = NativeModelEma(model, decay=0.9999, use_warmup=True)
    assert not ema.module.training and model.training
    assert [round(ema.get_decay(k), 3) for k in (1, 2, 3)] == [0.0, 0.37, 0.519]
    oracle = {k: v.detach().double() for k, v in ema.module.state_dict().items()}
    bound = {k: torch.zeros_like(v) for k, v in oracle.items()}
    for step in (1, 2, 3):
        _train_step(model, opt, batches[step])
        snap = {k: v.detach().clone() for k, v in model.state_dict().items()}
        ema.update(model, step=step)
        decay = ema.get_decay(step)
        twin = ema.module.state_dict()
        assert list(twin) == list(snap)
        for k, p in snap.items():
            assert p.dtype == torch.float32, k
            bound[k] = bound[k] + lerp_bound(oracle[k], p)  # an earlier step's error enters the next one scaled by decay <= 1
            oracle[k] = lerp_oracle(oracle[k], p, decay)
            assert_within(f"trajectory step {step} {k}", twin[k], oracle[k], bound[k].clamp_min(1e-300))
            if step == 1:
                assert torch.equal(twin[k], p), k
        moved = [k for k, p in snap.items() if p.ndim >= 2 and not torch.equal(twin[k], p)]
        assert (not moved) if step == 1 else len(moved) == sum(p.ndim >= 2 for p in snap.values()), (step, moved[:4])


def test_update_drops_the_twins_operand_caches(tiny):
    from open_clip_amd import NativeModelEma
    from open_clip_amd.optim import weight_caches_of
    cfg, state, batches = tiny
    model = _tiny(state, cfg)
    ema = NativeModelEma(model, decay=0.5)
    before = _features(ema.module, batches[0])  # fills the twin's caches
    assert any(c.peek(p, "n") is not None for c in weight_caches_of(ema.module) for p in ema.module.parameters() if p.ndim == 2)
    _train_step(model, _adamw(model, lr=1e-2), batches[1])
    ema.update(model, step=7)
    after = _features(ema.module, batches[0])
    fresh = _tiny(ema.module.state_dict(), cfg).eval()
    assert _same(after, _features(fresh, batches[0])), "the twin ran on stale bf16 operand copies"
    assert not _same(after, before)
    ema.set(model)  # and the copy: the twin's forward is the model's
    assert _same(_features(ema.module, batches[0]), _features(_tiny(model.state_dict(), cfg).eval(), batches[0]))


def test_update_follows_moved_parameter_storage(tiny):
    from open_clip_amd import NativeModelEma
    cfg, state, batches = tiny
    model = _tiny(state, cfg)
    ema = NativeModelEma(model, decay=0.5)
    ema.update(model, step=5)  # builds the pointer table
    key = "transformer.resblocks.1.mlp.c_fc.weight"
    p = dict(model.named_parameters())[key]
    old = p.data
    new = torch.randn_like(old)
    p.data = new
    old.fill_(float("nan"))  # still alive: a stale table would read NaN out of it, not fault
    e0 = ema.module.state_dict()[key].clone()
    ema.update(model, step=6)
    twin = ema.module.state_dict()
    assert all(bool(torch.isfinite(v).all()) for v in twin.values()), "the update read the parameter's old storage"
    assert_within("moved parameter", twin[key].cpu(), lerp_oracle(e0.cpu(), new.cpu(), 0.5), lerp_bound(e0.cpu(), new.cpu()))
    assert float((twin[key] - e0).abs().mean()) > 0.1
    # the other side: the twin's own storage replaced
    q = dict(ema.module.named_parameters())[key]
    kept = q.data
    q.data = kept.clone()
    kept.fill_(float("nan"))
    e0 = q.data.clone()
    ema.update(model, step=7)
    assert_within("moved twin", q.data.cpu(), lerp_oracle(e0.cpu(), new.cpu(), 0.5), lerp_bound(e0.cpu(), new.cpu()))
    assert bool(torch.isnan(kept).all()), "the update wrote into the twin's old storage"


@pytest.mark.skipif(not reference_importable(), reason="reference packages not available")
def test_through_the_reference_task(tiny):
    import_reference()
    from open_clip.task import CLIPTask
    from open_clip_amd import NativeModelEma, setup_ema
    from open_clip_amd.loss import NativeClipLoss
    cfg, state, batches = tiny

    def make(st):
        model = _tiny(st, cfg)
        task = CLIPTask(model, loss=NativeClipLoss(deterministic=True), rank=0, world_size=1, device=torch.device("cuda"), verbose=False)
        return model, setup_ema(task, decay=0.5)

    model, task = make(state)
    ema = task.trainable_module_ema
    assert task.has_ema and type(ema) is NativeModelEma
    opt = _adamw(model, lr=1e-2)
    task.train()
    assert not ema.module.training
    losses, _ = task.training_forward(batches[1])
    losses["loss"].backward()
    opt.step()
    start = {k: v.clone() for k, v in ema.module.state_dict().items()}
    task.update_ema(step=2)
    for k, v in ema.module.state_dict().items():
        p = model.state_dict()[k]
        assert_within(f"task.update_ema {k}", v, lerp_oracle(start[k], p, 0.5), lerp_bound(start[k], p).clamp_min(1e-300))
    task.eval()
    with torch.no_grad():
        out = task.eval_forward(batches[0])
    got = (out["image_features"], out["text_features"])
    assert _same(got, _features(ema.module, batches[0]))
    assert not _same(got, _features(model, batches[0]))
    # state_dict()["state_dict_ema"] into a second task whose twin has run (its caches are filled)
    model2, task2 = make(init_state_dict(cfg, seed=5, perturb=True))
    task2.eval()
    with torch.no_grad():
        other = task2.eval_forward(batches[0])
    assert not _same(got, (other["image_features"], other["text_features"]))
    sd = task.state_dict()
    assert list(sd["state_dict_ema"]) == list(sd["state_dict"])
    task2.load_state_dict(sd)
    with torch.no_grad():
        out2 = task2.eval_forward(batches[0])
    assert _same(got, (out2["image_features"], out2["text_features"]))
    assert _same(_features(model2, batches[0]), _features(model, batches[0]))
