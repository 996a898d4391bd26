"""CPU: the float64 restatement of the position-table resampling (tests/pos_resample_util.py) against ``F.interpolate`` in float64, its power to see
the defects the GPU bound must catch, the reference's own results (tests/golden/pos_resize.npz (a)), and the host behaviour of
``resize_pos_embed`` / ``resize_text_pos_embed`` / ``create_model(force_image_size=, force_context_length=)``.  No kernel runs here."""
import numpy as np
import pytest
import torch

from tests import pos_resample_util as U


@pytest.mark.parametrize("mode,antialias,src_hw,dst_hw", U.cases(), ids=lambda v: str(v).replace(" ", ""))
def test_restatement_matches_interpolate_in_float64(mode, antialias, src_hw, dst_hw):
    """(the grid (2, 3) -> (7, 1) is left out: torch's antialiased CPU path disagrees with its own rule there)"""
    for prefix in (0, 1):
        table = U.noise_table(3, prefix, src_hw, 5).astype(np.float64)
        got = U.resample64(table, prefix, src_hw, dst_hw, mode, antialias)
        want = U.torch_interpolate(table, prefix, src_hw, dst_hw, mode, antialias, torch.float64)
        assert got.shape == want.shape == (prefix + dst_hw[0] * dst_hw[1], 5)
        assert float(np.abs(got - want).max()) <= 1e-13
        if src_hw == dst_hw:
            assert np.array_equal(got, table)  # equal lengths: the identity, exactly


def test_transposed_map_is_the_adjoint():
    """<W x, y> == <x, W^T y> in float64 for every case: transpose64 is the gradient of resample64"""
    rng = np.random.default_rng(4)
    for mode, antialias, src_hw, dst_hw in U.cases():
        x = rng.standard_normal((1 + src_hw[0] * src_hw[1], 3))
        y = rng.standard_normal((1 + dst_hw[0] * dst_hw[1], 3))
        a = float((U.resample64(x, 1, src_hw, dst_hw, mode, antialias) * y).sum())
        b = float((x * U.transpose64(y, 1, src_hw, dst_hw, mode, antialias)).sum())
        assert abs(a - b) <= 1e-12 * max(1.0, abs(a))


@pytest.mark.parametrize("defect", U.DEFECTS)
def test_the_oracle_sees_each_defect(defect):
    """a = -0.75 in the antialiased rule, a dropped border tap, an unnormalised window, a centre half a pixel off: each moves some output of the noise
    cases by more than 1e-3 max|src| -- ten times the 1e-4 max|src| the GPU tests require their bound to stay under"""
    moved = 0.0
    for mode, antialias, src_hw, dst_hw in U.cases():
        table = U.noise_table(1, 1, src_hw, 6).astype(np.float64)
        diff = np.abs(U.resample64(table, 1, src_hw, dst_hw, mode, antialias, defect) - U.resample64(table, 1, src_hw, dst_hw, mode, antialias))
        moved = max(moved, float(diff.max() / np.abs(table).max()))
    print(f"defect {defect}: moves an output by {moved:.3e} max|src|")
    assert moved > 1e-3


def test_the_derived_bound_stays_under_the_condition():
    """the bound of the module's docstring, forward and backward, on every case and C = 6: below 1e-4 max|src| (the GPU tests assert it again on
    their own tables)"""
    for mode, antialias, src_hw, dst_hw in U.cases():
        table = U.noise_table(1, 1, src_hw, 6)
        dout = U.noise_table(2, 1, dst_hw, 6)
        assert float(U.forward_bound(table, 1, src_hw, dst_hw, mode, antialias).max()) < 1e-4 * float(np.abs(table).max())
        assert float(U.backward_bound(dout, 1, src_hw, dst_hw, mode, antialias).max()) < 1e-4 * float(np.abs(dout).max())


@pytest.mark.parametrize("name", sorted(U.RESIZES))
def test_reference_fixture_agrees_with_the_restatement(name):
    g = U.fixture()[0]
    _, prefix, src_hw, dst_hw, interpolation, antialias = U.RESIZES[name]
    want = U.resample64(U.resize_source(name).numpy(), prefix, src_hw, dst_hw, interpolation, antialias)
    dev = float(np.abs(g["resize/" + name].astype(np.float64) - want).max())
    assert g["resize/" + name].shape == want.shape
    assert dev <= float(g["refdev/" + name]) * (1 + 1e-12) and float(g["refdev/" + name]) <= 1e-6


# ---- host behaviour ------------------------------------------------------------------------------------------------------------------------
def _model(name="tiny-test", **kw):
    from open_clip_amd.configs import get_model_config
    from open_clip_amd.model import NativeCLIP
    cfg = get_model_config(name)
    return NativeCLIP(cfg["embed_dim"], cfg["vision_cfg"], cfg["text_cfg"], **kw), cfg


@pytest.fixture
def no_library(monkeypatch):
    from open_clip_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("the library must not be touched")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(_lib, "call", refuse)


def test_equal_sizes_and_missing_keys_return_without_the_library(no_library):
    import open_clip_amd
    from open_clip_amd.synth import init_state_dict
    model, cfg = _model()
    sd = init_state_dict(cfg, 3)
    before = {k: v.clone() for k, v in sd.items()}
    open_clip_amd.resize_pos_embed(sd, model)
    open_clip_amd.resize_text_pos_embed(sd, model)
    assert all(torch.equal(sd[k], before[k]) for k in before)
    custom = {"text.positional_embedding": sd["positional_embedding"].clone()}  # the CustomTextCLIP layout: the key is found, and fits
    open_clip_amd.resize_text_pos_embed(custom, model)
    empty = {}
    open_clip_amd.resize_pos_embed(empty, model)
    open_clip_amd.resize_text_pos_embed(empty, model)
    assert empty == {}


def test_bad_tables_and_modes_raise(no_library):
    from open_clip_amd.model import resize_pos_embed, resize_text_pos_embed
    model, _ = _model()  # a 2 x 2 grid, width 128, context 16
    with pytest.raises(ValueError, match="no perfect square.*old_grid_size"):
        resize_pos_embed({"visual.positional_embedding": torch.zeros(1 + 6, 128)}, model)
    with pytest.raises(ValueError, match=r"old_grid_size \(2, 4\) does not hold"):
        resize_pos_embed({"visual.positional_embedding": torch.zeros(1 + 6, 128)}, model, old_grid_size=(2, 4))
    with pytest.raises(ValueError, match="width"):
        resize_pos_embed({"visual.positional_embedding": torch.zeros(1 + 9, 64)}, model)
    with pytest.raises(ValueError, match="width changed"):
        resize_text_pos_embed({"positional_embedding": torch.zeros(8, 64)}, model)
    for fn in (resize_pos_embed, resize_text_pos_embed):
        with pytest.raises(NotImplementedError, match="nearest"):
            fn({}, model, interpolation="nearest")


def test_ops_refuse_an_unknown_mode_and_a_cpu_table(no_library):
    from open_clip_amd import ops
    with pytest.raises(NotImplementedError, match="area"):
        ops.pos_resample(torch.zeros(5, 8), 1, (2, 2), (3, 3), "area")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.pos_resample(torch.zeros(5, 8), 1, (2, 2), (3, 3))
    with pytest.raises(RuntimeError, match=r"not \[prefix"):
        ops.pos_resample(torch.zeros(6, 8), 1, (2, 2), (3, 3))


def test_entry_points_refuse_bad_arguments_on_the_host():
    """checked before any launch, the argument named: safe without a GPU (the operands are fake and never dereferenced)"""
    from open_clip_amd import _lib, build
    build.build()
    p = 4096
    for fn in ("ocn_pos_resample_fwd", "ocn_pos_resample_bwd"):
        with pytest.raises(RuntimeError, match=fn + r".*Hs=65"):
            _lib.call(fn, p, p, 1, 65, 7, 7, 7, 8, 1, 1, 0)
        with pytest.raises(RuntimeError, match=fn + r".*Wo=0"):
            _lib.call(fn, p, p, 1, 7, 7, 7, 0, 8, 1, 1, 0)
        with pytest.raises(RuntimeError, match=fn + r".*antialias=1 is not defined for a 1-D linear call"):
            _lib.call(fn, p, p, 0, 1, 77, 1, 32, 8, 0, 1, 0)
        with pytest.raises(RuntimeError, match=fn + r".*mode=2"):
            _lib.call(fn, p, p, 1, 7, 7, 7, 7, 8, 2, 0, 0)
        with pytest.raises(RuntimeError, match=fn + r".*C=0"):
            _lib.call(fn, p, p, 1, 7, 7, 7, 7, 0, 1, 1, 0)
        with pytest.raises(RuntimeError, match=fn + r".*null operand"):
            _lib.call(fn, 0, p, 1, 7, 7, 7, 7, 8, 1, 1, 0)
    with pytest.raises(RuntimeError, match=r"1-D lengths Ws=4097"):
        _lib.call("ocn_pos_resample_fwd", p, p, 0, 1, 4097, 1, 32, 8, 0, 0, 0)
    with pytest.raises(RuntimeError, match=r"ocn_pos_resample_bwd.*Ws=77"):  # the backward takes grid sides only
        _lib.call("ocn_pos_resample_bwd", p, p, 0, 1, 77, 1, 32, 8, 0, 0, 0)


def test_force_arguments_reach_the_config():
    from open_clip_amd.model import create_model
    m = create_model("tiny-test", device="cpu", force_image_size=96, force_context_length=40)
    assert m.visual.image_size == (96, 96) and m.visual.grid_size == (3, 3) and m.visual.preprocess_cfg["size"] == (96, 96)
    assert tuple(m.visual.positional_embedding.shape) == (10, 128)
    assert m.context_length == 40 and tuple(m.positional_embedding.shape) == (40, 128) and m.attn_mask.shape == (40, 40)
    assert m.pack_text and not m.visual.dynamic_img_size
    r = create_model("tiny-test", device="cpu", force_image_size=(96, 64), dynamic_img_size=True)
    assert r.visual.image_size == (96, 64) and r.visual.grid_size == (3, 2) and r.visual.preprocess_cfg["size"] == (96, 64)
    assert tuple(r.visual.positional_embedding.shape) == (7, 128) and r.visual.live_tokens() == 7 and r.visual.dynamic_img_size
    assert create_model("tiny-test", device="cpu", force_image_size=[96]).visual.image_size == (96, 96)  # main.py hands a list on
    long = create_model("tiny-test", device="cpu", force_context_length=400)
    assert long.context_length == 400 and not long.pack_text  # the packed text tower's length rule follows the forced length
    plain = create_model("tiny-test", device="cpu")
    assert plain.visual.image_size == (64, 64) and plain.context_length == 16


def test_lazy_names():
    import open_clip_amd
    from open_clip_amd import model
    assert open_clip_amd.resize_pos_embed is model.resize_pos_embed and open_clip_amd.resize_text_pos_embed is model.resize_text_pos_embed
