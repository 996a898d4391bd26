"""Position tables at another size on a real MI355X: ``ocn_pos_resample_fwd`` / ``_bwd`` against the float64 restatement of tests/pos_resample_util.py
under the bound derived there from the kernel's stated arithmetic (never fitted to what was observed), their exact cases, the state-dict functions and a
whole training step against the reference's own (tests/golden/pos_resize.npz), and calls at another image size (``dynamic_img_size``).  Measured values go
to the parity report of tests/test_kernels_gpu.py (``_report``)."""
import numpy as np
import pytest
import torch

from tests import pos_resample_util as U
from tests.golden_util import check_grad, grad_keys
from tests.test_clipa_gpu import _grad_bound
from tests.test_kernels_gpu import _report, dev  # noqa: F401  (dev: module fixture)

pytestmark = pytest.mark.gpu

F32 = torch.float32
SENTINEL = 12345.0
WIDTHS = (6, 8, 768, 1280)  # a scalar-only row, two float4 lanes, a ViT-B and a ViT-H row (more lanes than one pass of the workgroup)
RULE_IDS = [f"{m}{'-aa' if a else ''}" for m, a in U.RULES]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(fn, table, prefix, src_hw, dst_hw, mode, antialias, dev):
    """``ops.pos_resample`` / ``pos_resample_bwd`` on a numpy table -> numpy"""
    from open_clip_amd import ops
    return getattr(ops, fn)(torch.from_numpy(np.ascontiguousarray(table)).to(dev), prefix, src_hw, dst_hw, mode, antialias).cpu().numpy()


def _rule_cases(mode, antialias):
    return [(s, d) for m, a, s, d in U.cases() if (m, a) == (mode, antialias)]


@pytest.mark.parametrize("mode,antialias", U.RULES, ids=RULE_IDS)
def test_forward_against_float64(dev, mode, antialias):
    """every grid / length of the rule, C in WIDTHS, prefix in {0, 1}: |kernel - float64| <= the derived bound element by element, and the bound itself
    below 1e-4 max|src| (ten times under what the defects of tests/test_pos_resample.py move).  Reported: the worst error / bound, and the worst error
    as a multiple of torch-fp32-on-CPU's own deviation from float64 (not gated)."""
    worst, worst_torch, worst_cond = 0.0, 0.0, 0.0
    for src_hw, dst_hw in _rule_cases(mode, antialias):
        for C in WIDTHS:
            for prefix in (0, 1):
                table = U.noise_table(C + prefix, prefix, src_hw, C)
                want = U.resample64(table, prefix, src_hw, dst_hw, mode, antialias)
                bound = U.forward_bound(table, prefix, src_hw, dst_hw, mode, antialias)
                cond = float(bound.max()) / float(np.abs(table).max())
                got = _run("pos_resample", table, prefix, src_hw, dst_hw, mode, antialias, dev)
                assert got.shape == want.shape and got.dtype == np.float32
                err = np.abs(got.astype(np.float64) - want)
                ratio = float((err / np.maximum(bound, 1e-300))[prefix:].max())
                tdev = float(np.abs(U.torch_interpolate(table, prefix, src_hw, dst_hw, mode, antialias, torch.float32).astype(np.float64) - want).max())
                worst, worst_cond = max(worst, ratio), max(worst_cond, cond)
                if tdev > 0:
                    worst_torch = max(worst_torch, float(err.max()) / tdev)
                print(f"pos_resample_fwd[{mode} aa={int(antialias)} {src_hw}->{dst_hw} C={C} prefix={prefix}]: max err {float(err.max()):.3e} "
                      f"err/bound {ratio:.3f} bound/max|src| {cond:.2e} torch fp32 dev {tdev:.3e}")
                assert cond < 1e-4, (src_hw, dst_hw, C, cond)
                assert bool((err <= bound).all()), (src_hw, dst_hw, C, prefix, ratio)
                assert np.array_equal(got[:prefix].view(np.int32), table[:prefix].view(np.int32))
    _report(f"pos_resample_fwd[{mode} aa={int(antialias)}]: worst err/bound {worst:.3f}, worst bound {worst_cond:.2e} max|src|, "
            f"worst err / torch-fp32-CPU deviation {worst_torch:.2f}")


@pytest.mark.parametrize("mode,antialias", U.RULES, ids=RULE_IDS)
def test_equal_sizes_give_back_the_source_bits(dev, mode, antialias):
    """identity axes under every rule, signed zeros included; one axis equal and the other not: still within the bound (covered above), here the equal
    case alone -- bit for bit, with a sentinel behind the result"""
    from open_clip_amd import _lib
    # (a grid of one row IS the 1-D call, Hs = Ho = 1: the antialiased linear rule is refused there, so its one-element case is 2 x 1)
    shapes = [((1, 77), (1, 77)), ((1, 1), (1, 1))] if mode == "linear" else [((7, 7), (7, 7)), ((5, 9), (5, 9)), ((2, 1), (2, 1)), ((64, 3), (64, 3))]
    for hw, _ in shapes:
        for C in (6, 768):
            table = torch.from_numpy(U.noise_table(7, 1, hw, C))
            table[1, 0], table[1, 1] = -0.0, 0.0
            n = table.numel()
            buf = torch.full((n + 64,), SENTINEL, dtype=F32, device=dev)
            _lib.call("ocn_pos_resample_fwd", table.to(dev).data_ptr(), buf.data_ptr(), 1, hw[0], hw[1], hw[0], hw[1], C, int(mode == "bicubic"),
                      int(antialias), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert torch.equal(_bits(buf[:n].cpu()), _bits(table.reshape(-1))), (hw, C)
            assert bool((buf[n:] == SENTINEL).all()), "store behind the result"


@pytest.mark.parametrize("src_hw,dst_hw,mode", [((6, 6), (12, 12), "bilinear"), ((5, 3), (10, 6), "bilinear"), ((1, 16), (1, 32), "linear")])
def test_forward_is_exact_on_integers_at_2x(dev, src_hw, dst_hw, mode):
    """integer tables with |v| <= 64 under the non-antialiased linear rule at 2x: every weight is 0.25, 0.75 or 1, every product and partial sum a
    multiple of 1/16 below 2^7 -- exact in fp32 in any order: bit-equal to the float64 result, twice, with prefix rows (a NaN among them) copied"""
    for C in (6, 8, 772):
        rng = np.random.default_rng(C)
        table = rng.integers(-64, 65, (1 + src_hw[0] * src_hw[1], C)).astype(np.float32)
        table[0, 0], table[0, 1] = np.nan, -0.0
        want = U.resample64(table, 1, src_hw, dst_hw, mode, False).astype(np.float32)
        got = _run("pos_resample", table, 1, src_hw, dst_hw, mode, False, dev)
        again = _run("pos_resample", table, 1, src_hw, dst_hw, mode, False, dev)
        assert np.array_equal(got[1:].view(np.int32), want[1:].view(np.int32))
        assert np.array_equal(got[:1].view(np.int32), table[:1].view(np.int32)), "the prefix row is a bit copy"
        assert np.array_equal(got.view(np.int32), again.view(np.int32))


def test_two_forward_runs_give_the_same_bits(dev):
    for mode, antialias, src_hw, dst_hw in [("bicubic", True, (16, 16), (24, 24)), ("bicubic", True, (24, 24), (7, 7)), ("bicubic", False, (7, 5), (4, 9))]:
        table = U.noise_table(11, 1, src_hw, 1280)
        a = _run("pos_resample", table, 1, src_hw, dst_hw, mode, antialias, dev)
        b = _run("pos_resample", table, 1, src_hw, dst_hw, mode, antialias, dev)
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_a_table_that_starts_on_no_16_byte_boundary(dev):
    """C % 4 == 0 but the table 4 bytes into its allocation: the scalar lanes run, same bits as the aligned call"""
    from open_clip_amd import ops
    src_hw, dst_hw, C = (7, 7), (12, 12), 8
    table = torch.from_numpy(U.noise_table(12, 1, src_hw, C))
    buf = torch.zeros(table.numel() + 1, dtype=F32, device=dev)
    view = buf[1:].view(table.shape)
    view.copy_(table)
    assert view.data_ptr() % 16 == 4
    assert torch.equal(_bits(ops.pos_resample(view, 1, src_hw, dst_hw)), _bits(ops.pos_resample(table.to(dev), 1, src_hw, dst_hw)))


# ---- backward (the transposed map) ------------------------------------------------------------------------------------------------------------
def _bwd_cases(mode, antialias):
    """the rule's grids; of the 1-D lengths those the backward takes (sides up to 64)"""
    return [(s, d) for s, d in _rule_cases(mode, antialias) if max(s + d) <= 64]


@pytest.mark.parametrize("mode,antialias", U.RULES, ids=RULE_IDS)
def test_backward_against_float64(dev, mode, antialias):
    """dsrc against W^T ddst in float64 under the bound derived for the transposed sums; the bound below 1e-4 max|ddst|; two runs the same bits; the
    prefix gradient a bit copy"""
    worst = 0.0
    for src_hw, dst_hw in _bwd_cases(mode, antialias):
        for C in WIDTHS:
            for prefix in (0, 1):
                dout = U.noise_table(3 * C + prefix, prefix, dst_hw, C)
                want = U.transpose64(dout, prefix, src_hw, dst_hw, mode, antialias)
                bound = U.backward_bound(dout, prefix, src_hw, dst_hw, mode, antialias)
                cond = float(bound.max()) / float(np.abs(dout).max())
                got = _run("pos_resample_bwd", dout, prefix, src_hw, dst_hw, mode, antialias, dev)
                again = _run("pos_resample_bwd", dout, prefix, src_hw, dst_hw, mode, antialias, dev)
                assert got.shape == want.shape and got.dtype == np.float32
                err = np.abs(got.astype(np.float64) - want)
                ratio = float((err / np.maximum(bound, 1e-300))[prefix:].max()) if err[prefix:].max() > 0 else 0.0
                worst = max(worst, ratio)
                print(f"pos_resample_bwd[{mode} aa={int(antialias)} {src_hw}->{dst_hw} C={C} prefix={prefix}]: max err {float(err.max()):.3e} "
                      f"err/bound {ratio:.3f} bound/max|ddst| {cond:.2e}")
                assert cond < 1e-4, (src_hw, dst_hw, C, cond)
                assert bool((err <= bound).all()), (src_hw, dst_hw, C, prefix, ratio)
                assert np.array_equal(got.view(np.int32), again.view(np.int32))
                assert np.array_equal(got[:prefix].view(np.int32), dout[:prefix].view(np.int32))
    _report(f"pos_resample_bwd[{mode} aa={int(antialias)}]: worst err/bound {worst:.3f}")


@pytest.mark.parametrize("src_hw,dst_hw,mode", [((6, 6), (12, 12), "bilinear"), ((5, 3), (10, 6), "bilinear"), ((1, 16), (1, 32), "linear")])
def test_backward_is_exact_on_integers_at_2x(dev, src_hw, dst_hw, mode):
    """integer ddst with |v| <= 64 and the weights 0.25 / 0.75 / 1: every coefficient, product and partial sum is a multiple of 1/16 far below 2^24"""
    for C in (6, 8, 772):
        dout = np.random.default_rng(C + 1).integers(-64, 65, (1 + dst_hw[0] * dst_hw[1], C)).astype(np.float32)
        want = U.transpose64(dout, 1, src_hw, dst_hw, mode, False).astype(np.float32)
        got = _run("pos_resample_bwd", dout, 1, src_hw, dst_hw, mode, False, dev)
        assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_autograd_function(dev):
    """_PosResampleFn: forward = ops.pos_resample (bicubic, antialiased), backward = ops.pos_resample_bwd, into the leaf's .grad"""
    from open_clip_amd import ops
    from open_clip_amd.model import _PosResampleFn
    pos = torch.from_numpy(U.noise_table(5, 1, (6, 6), 256)).to(dev).requires_grad_(True)
    out = _PosResampleFn.apply(pos, 1, (6, 6), (10, 10))
    assert torch.equal(out, ops.pos_resample(pos.detach(), 1, (6, 6), (10, 10), "bicubic", True))
    d = torch.from_numpy(U.noise_table(6, 1, (10, 10), 256)).to(dev)
    out.backward(d)
    assert torch.equal(pos.grad, ops.pos_resample_bwd(d, 1, (6, 6), (10, 10), "bicubic", True))


# ---- the state-dict functions against the reference's results --------------------------------------------------------------------------------
class _Shape:
    """what the two functions read of a model"""

    def __init__(self, grid, num_pos, width):
        self.visual = type("V", (), {"grid_size": grid, "positional_embedding": torch.empty(grid[0] * grid[1] + 1, width)})()
        self.positional_embedding = torch.empty(num_pos, width)

    def parameters(self):
        return iter(())


@pytest.mark.parametrize("name", sorted(U.RESIZES))
def test_state_dict_functions_against_the_reference(dev, name):
    """fixture (a): |ours - the reference's| <= the forward bound + the reference's own recorded deviation from float64, element by element; the
    entry keeps its dtype and device (an fp16 CPU entry stays one)"""
    import open_clip_amd
    g = U.fixture()[0]
    _, prefix, src_hw, dst_hw, interpolation, antialias = U.RESIZES[name]
    table = U.resize_source(name)
    if prefix:
        key, model, fn = "visual.positional_embedding", _Shape(dst_hw, 1, table.shape[1]), open_clip_amd.resize_pos_embed
    else:
        key, model, fn = "positional_embedding", _Shape((1, 1), dst_hw[1], table.shape[1]), open_clip_amd.resize_text_pos_embed
    sd = {key: table.clone()}
    fn(sd, model)  # the defaults are the rule of the fixture
    got = sd[key]
    assert got.dtype == F32 and got.device.type == "cpu" and tuple(got.shape) == g["resize/" + name].shape
    bound = U.forward_bound(table.numpy(), prefix, src_hw, dst_hw, interpolation, antialias) + float(g["refdev/" + name])
    err = np.abs(got.numpy().astype(np.float64) - g["resize/" + name].astype(np.float64))
    _report(f"resize[{name}] against the reference: max err {float(err.max()):.3e}, worst err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    half = {key: table.half()}
    fn(half, model, device=dev)
    assert half[key].dtype == torch.float16 and half[key].device.type == "cpu"
    assert float((half[key].float() - got).abs().max()) <= 2.0 ** -10 * float(got.abs().max()) + 1e-7  # the fp16 table's own rounding, in and out
    on_dev = {key: table.to(dev)}
    fn(on_dev, model)
    assert on_dev[key].device.type == "cuda" and torch.equal(on_dev[key].cpu(), got)
    if prefix:  # a rectangular source needs its grid named
        rect = {key: torch.from_numpy(U.noise_table(8, 1, (4, 9), table.shape[1]))}
        before = rect[key].clone()
        fn(rect, model, old_grid_size=(4, 9))
        want = U.resample64(before.numpy(), 1, (4, 9), dst_hw, "bicubic", True)
        assert bool((np.abs(rect[key].numpy() - want) <= U.forward_bound(before.numpy(), 1, (4, 9), dst_hw, "bicubic", True)).all())


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
def _load(tmp_path, state, **kw):
    from open_clip_amd.model import create_model
    path = str(tmp_path / "small_96_77.pt")
    torch.save(state, path)
    return create_model("small-test", pretrained=path, output_dict=True, **kw).train()


@pytest.mark.parametrize("image_stream", ["fp32", "bf16"])
def test_step_at_another_size_against_the_reference(tmp_path, image_stream):
    """fixture (b): the seeded 96 / 77 checkpoint loaded at image 160 and context 32, one training step with NativeClipLoss against the reference's
    own step on its own resized tables: features max-abs <= 4e-3, loss <= 2e-2, every gradient inside tests/test_clipa_gpu.py's ``_grad_bound``,
    the full gradients of both position tables inside the same bound"""
    from open_clip_amd.loss import NativeClipLoss
    g, cfg, big, state, batch = U.fixture()
    model = _load(tmp_path, state, force_image_size=U.IMAGE, force_context_length=U.CONTEXT, image_stream=image_stream)
    assert model.visual.grid_size == (10, 10) and model.context_length == U.CONTEXT and model.pack_text
    out = model(image=batch["image"].cuda(), text=batch["text"].cuda())
    loss = NativeClipLoss()(**out)
    loss.backward()
    torch.cuda.synchronize()
    tag = f"resized step [{image_stream}]"
    fi = float((out["image_features"].float().cpu() - torch.from_numpy(g["out/image_features"])).abs().max())
    ft = float((out["text_features"].float().cpu() - torch.from_numpy(g["out/text_features"])).abs().max())
    dl = abs(float(loss.detach()) - float(g["out/loss"]))
    grads = {k: p.grad for k, p in model.named_parameters()}
    assert set(grads) == set(grad_keys(g)) and all(v is not None for v in grads.values())
    rows = sorted(((check_grad(g, k, grads[k], 0)[0], k) for k in grad_keys(g)), reverse=True)
    _report(f"{tag}: image_features max_abs={fi:.3e} text_features max_abs={ft:.3e} loss={float(loss.detach()):.6f} ref={float(g['out/loss']):.6f}")
    for rel, k in rows[:6]:
        _report(f"{tag}:   grad rel_l2={rel:.3e} bound={_grad_bound(g, k, grads[k].ndim, image_stream):.2e} |g|={float(g['gnorm/' + k]):.3e} {k}")
    full = {}
    for k in ("visual.positional_embedding", "positional_embedding"):
        ref = torch.from_numpy(g["fullgrad/" + k]).double()
        full[k] = float((grads[k].double().cpu() - ref).norm() / ref.norm())
        _report(f"{tag}:   full grad rel_l2={full[k]:.3e} {k}")
    assert fi <= 4e-3 and ft <= 4e-3, (fi, ft)
    assert dl <= 2e-2, dl
    bad = [(k, rel, _grad_bound(g, k, grads[k].ndim, image_stream)) for rel, k in rows if not rel <= _grad_bound(g, k, grads[k].ndim, image_stream)]
    assert not bad, bad
    assert all(rel <= _grad_bound(g, k, 2, image_stream) for k, rel in full.items()), full


def test_rectangular_image_size_against_the_elementary_forward(tmp_path):
    """``force_image_size=(160, 96)`` on the square 6 x 6 checkpoint (no ``old_grid_size`` needed): a 10 x 6 grid.  Image features against the
    elementary-torch forward (oracle.clip_oracle) on the float64-resampled table, max-abs <= 4e-3, on both image streams; a training step leaves
    finite gradients of the right shapes."""
    from oracle import clip_oracle as O
    from open_clip_amd.loss import NativeClipLoss
    _, cfg, big, state, batch = U.fixture()
    image = torch.randn(U.BATCH, 3, 160, 96, generator=torch.Generator().manual_seed(7)).half().float()
    p = dict(state)
    p["visual.positional_embedding"] = torch.from_numpy(U.resample64(state["visual.positional_embedding"].numpy(), 1, (6, 6), (10, 6), "bicubic", True)).float()
    want = O.encode_image(image, p, big)
    for image_stream in ("fp32", "bf16"):
        model = _load(tmp_path, state, force_image_size=(160, 96), force_context_length=U.CONTEXT, image_stream=image_stream)
        assert model.visual.image_size == (160, 96) and model.visual.grid_size == (10, 6) and tuple(model.visual.positional_embedding.shape) == (61, 256)
        with torch.no_grad():
            got = model.eval().encode_image(image.cuda(), normalize=True)
        err = float((got.float().cpu() - want).abs().max())
        _report(f"rectangular 160 x 96 [{image_stream}]: image_features max_abs={err:.3e}")
        assert err <= 4e-3
        with pytest.raises(RuntimeError, match="image size"):
            model.encode_image(batch["image"].cuda())  # 160 x 160
    out = model.train()(image=image.cuda(), text=batch["text"].cuda())
    NativeClipLoss()(**out).backward()
    torch.cuda.synchronize()
    assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for q in model.parameters())
    assert float(model.visual.positional_embedding.grad.abs().sum()) > 0


# ---- a call at another size -----------------------------------------------------------------------------------------------------------------
def _small(state, **kw):
    from open_clip_amd.configs import get_model_config
    from open_clip_amd.model import NativeCLIP
    cfg = get_model_config(U.CFG)
    m = NativeCLIP(cfg["embed_dim"], cfg["vision_cfg"], cfg["text_cfg"], output_dict=True, deterministic=True, **kw)
    m.load_state_dict(state, strict=True)
    return m.cuda().train()


def test_dynamic_call_equals_the_resized_twin(tmp_path):
    """'small-test' at 96 with dynamic_img_size, called at 160, against the twin loaded with force_image_size=160 through resize_pos_embed (the same
    kernel on the same inputs): image features bit-identical; the gradient of the 6 x 6 + 1 table = W^T (float64) applied to the twin's gradient of its
    10 x 10 + 1 table, within the backward's derived bound"""
    _, cfg, big, state, batch = U.fixture()
    image = batch["image"].cuda()
    dyn = _small(state, dynamic_img_size=True)
    twin = _load(tmp_path, state, force_image_size=U.IMAGE, deterministic=True)
    assert dyn.visual.dynamic_img_size and dyn.visual.grid_size == (6, 6) and twin.visual.grid_size == (10, 10)
    a = dyn.encode_image(image, normalize=True)
    b = twin.encode_image(image, normalize=True)
    assert torch.equal(_bits(a.float()), _bits(b.float()))
    w = torch.randn(a.shape, generator=torch.Generator().manual_seed(3)).cuda()
    (a * w).sum().backward()
    (b * w).sum().backward()
    torch.cuda.synchronize()
    dtwin = twin.visual.positional_embedding.grad.cpu().numpy()
    want = U.transpose64(dtwin, 1, (6, 6), (10, 10), "bicubic", True)
    bound = U.backward_bound(dtwin, 1, (6, 6), (10, 10), "bicubic", True)
    got = dyn.visual.positional_embedding.grad.cpu().numpy()
    err = np.abs(got.astype(np.float64) - want)
    _report(f"dynamic 96 -> 160: table gradient against W^T of the twin's: max err {float(err.max()):.3e}, worst err/bound "
            f"{float((err[1:] / np.maximum(bound[1:], 1e-300)).max()):.3f}")
    assert tuple(got.shape) == (37, 256) and bool((err <= bound).all())
    for k in ("visual.conv1.weight", "visual.class_embedding", "visual.proj"):  # everything behind the table saw the same bits
        assert torch.equal(dict(dyn.named_parameters())[k].grad, dict(twin.named_parameters())[k].grad), k


def test_dynamic_switch_leaves_the_configured_size_alone():
    """a call at 96 with the switch on is the call with it off, bit for bit, features and gradients; with it off a 160 px call raises as before; sizes
    that are no multiple of the patch size, or too large, raise with it on"""
    _, cfg, big, state, batch = U.fixture()
    image96 = torch.randn(U.BATCH, 3, 96, 96, generator=torch.Generator().manual_seed(5)).cuda()
    text = torch.from_numpy(U.fixture()[0]["text"])
    res = []
    for on in (True, False):
        m = _small(state, dynamic_img_size=on)
        f = m.encode_image(image96, normalize=True)
        f.square().sum().backward()
        res.append((f.detach().clone(), {k: p.grad.clone() for k, p in m.visual.named_parameters()}))
    assert torch.equal(res[0][0], res[1][0])
    assert all(torch.equal(res[0][1][k], res[1][1][k]) for k in res[0][1])
    with pytest.raises(RuntimeError, match="image size"):
        m.encode_image(batch["image"].cuda())
    on = _small(state, dynamic_img_size=True)
    for shape in ((100, 96), (96, 16 * 65)):
        with pytest.raises(RuntimeError, match="dynamic_img_size"):
            on.encode_image(torch.zeros(1, 3, *shape, device="cuda"))
    assert text.shape[1] == U.CONTEXT  # (the text tower has no per-call form: its length is the model's)


def test_dynamic_call_with_patch_dropout():
    """one training step at 160 px with patch dropout 0.5: the plan keeps num_keep(100) of the call's 100 patches, the step runs, the learned 6 x 6 + 1
    table receives a finite, non-zero gradient; block recompute and the bf16 stream work at the call's grid as well"""
    from open_clip_amd.configs import get_model_config
    from open_clip_amd.loss import NativeClipLoss
    from open_clip_amd.model import NativeCLIP
    _, _, big, state, batch = U.fixture()
    cfg = get_model_config(U.CFG)
    text96 = torch.zeros(U.BATCH, 77, dtype=torch.int64)
    text96[:, :U.CONTEXT] = batch["text"]
    for image_stream, recompute in (("fp32", False), ("bf16", True)):
        m = NativeCLIP(cfg["embed_dim"], dict(cfg["vision_cfg"], patch_dropout=0.5), cfg["text_cfg"], output_dict=True, dynamic_img_size=True,
                       image_stream=image_stream)
        m.load_state_dict(state, strict=True)
        m = m.cuda().train()
        m.set_grad_checkpointing(recompute)
        out = m(image=batch["image"].cuda(), text=text96.cuda())
        keep = m.visual.patch_dropout.last_keep
        assert tuple(keep.shape) == (U.BATCH, m.visual.patch_dropout.num_keep(100)) == (U.BATCH, 50) and int(keep.max()) < 100 and int(keep.max()) >= 36
        NativeClipLoss()(**out).backward()
        torch.cuda.synchronize()
        grad = m.visual.positional_embedding.grad
        assert tuple(grad.shape) == (37, 256) and bool(torch.isfinite(grad).all()) and float(grad.abs().sum()) > 0
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
