"""CPU: the rank rule of the retrieval metrics against the reference's recorded and live results, the host-side refusals of the C ABI, and the public
surface of open_clip_amd.metrics."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from oracle.ref_shim import reference_available
from tests import retrieval_util as ru

needs_reference = pytest.mark.skipif(not reference_available(), reason="reference tree not present")


@pytest.fixture(scope="module")
def golden():
    return ru.load_golden()


def test_fixture_is_the_recipe(golden):
    image, text = ru.golden_features()
    assert golden["image"].dtype == np.int8 and golden["image"].shape == (ru.GOLDEN_N, ru.GOLDEN_E)
    assert np.array_equal(golden["image"], image.numpy()) and np.array_equal(golden["text"], text.numpy())
    # the planted rows are there: duplicates, zero rows, a query whose scores are all negative
    s = ru.int_scores(image, text)
    assert (s[2] < 0).all() and (image[0] == 0).all() and (image[5] == 0).all() and (text[12] == text[11]).all()


def test_rule_equals_the_reference_fixture(golden):
    image, text = torch.from_numpy(golden["image"]).long(), torch.from_numpy(golden["text"]).long()
    paired = torch.arange(image.shape[0])
    i2t = ru.rule_ranks(ru.int_scores(image, text), paired)
    t2i = ru.rule_ranks(ru.int_scores(text, image), paired)
    assert np.array_equal(i2t.numpy(), golden["image_to_text"])
    assert np.array_equal(t2i.numpy(), golden["text_to_image"])
    for key, value in ru.rule_metrics(i2t, t2i).items():
        assert value == float(golden["metric/" + key]), key


@needs_reference
@pytest.mark.parametrize("n", [300, 301])
def test_rule_equals_the_live_reference(n):
    """a second seed, an even and an odd count (numpy's median averages the two middle ranks of an even one)"""
    from oracle.ref_shim import import_reference
    import_reference()
    from open_clip_train import metrics as ref

    image, text = ru.golden_features(seed=77, n=n)
    # uncorrelated rows on top: ranks spread over the whole range, so the median is not pinned at 1
    gen = torch.Generator().manual_seed(5)
    text[n // 3:] = torch.randint(-3, 4, text[n // 3:].shape, generator=gen)
    paired = torch.arange(n)
    i2t, t2i = ru.rule_ranks(ru.int_scores(image, text), paired), ru.rule_ranks(ru.int_scores(text, image), paired)
    for chunk in (64, 0):
        ri, rt = ref._paired_retrieval_ranks(image.float(), text.float(), 100.0, chunk, retrieval_dtype=torch.float32)
        assert np.array_equal(ri, i2t.numpy()) and np.array_equal(rt, t2i.numpy())
    want = ref.get_clip_metrics(image.float(), text.float(), 100.0, retrieval_chunk_size=64)
    got = ru.rule_metrics(i2t, t2i)
    assert set(got) == set(want) and len(got) == 10
    for key in want:
        assert got[key] == float(want[key]), key
    assert got["image_to_text_median_rank"] > 1


# ---- host-side refusals through the C ABI: every check precedes any launch, so no GPU is needed -------------------------------------------------------
@pytest.fixture(scope="module")
def lib_call():
    from open_clip_amd import _lib, build
    build.build()
    return _lib.call


@pytest.fixture(scope="module")
def host_buffer():
    buf = ctypes.create_string_buffer(4096 + 64)
    return (ctypes.addressof(buf) + 63) // 64 * 64, buf  # an aligned non-null address that is never dereferenced (the calls below are refused first)


def test_label_ranks_refusals(lib_call, host_buffer):
    p = host_buffer[0]
    with pytest.raises(RuntimeError, match="ocn_label_ranks.*null operand"):
        lib_call("ocn_label_ranks", 0, p, 0, p, p, 4, 4, 32, 0)
    with pytest.raises(RuntimeError, match="ocn_label_ranks.*null operand"):
        lib_call("ocn_label_ranks", p, p, 0, p, 0, 4, 4, 32, 0)
    with pytest.raises(RuntimeError, match="K=48 must be a multiple of 32"):
        lib_call("ocn_label_ranks", p, p, 0, p, p, 4, 4, 48, 0)
    with pytest.raises(RuntimeError, match="K=0 must be a multiple of 32"):
        lib_call("ocn_label_ranks", p, p, 0, p, p, 4, 4, 0, 0)
    with pytest.raises(RuntimeError, match=r"label 4 lies outside \[0, N=4\)"):  # paired labels are r itself: the host sees them
        lib_call("ocn_label_ranks", p, p, 0, p, p, 5, 4, 32, 0)
    with pytest.raises(RuntimeError, match="R=0 and N=4 must be at least 1"):
        lib_call("ocn_label_ranks", p, p, 0, p, p, 0, 4, 32, 0)
    with pytest.raises(RuntimeError, match="R=4 and N=0 must be at least 1"):
        lib_call("ocn_label_ranks", p, p, p, p, p, 4, 0, 32, 0)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        lib_call("ocn_label_ranks", p + 2, p, 0, p, p, 4, 4, 32, 0)


def test_split_refusals(lib_call, host_buffer):
    p = host_buffer[0]
    with pytest.raises(RuntimeError, match="ocn_split_bf16x3.*null operand"):
        lib_call("ocn_split_bf16x3", 0, p, 4, 32, 0, 0)
    with pytest.raises(RuntimeError, match="R=0 and E=32 must be positive"):
        lib_call("ocn_split_bf16x3", p, p, 0, 32, 0, 0)
    with pytest.raises(RuntimeError, match="role=2 must be 0"):
        lib_call("ocn_split_bf16x3", p, p, 4, 32, 2, 0)


def test_cpu_tensors_have_no_path():
    from open_clip_amd import metrics, ops
    x = torch.zeros(4, 32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.split_bf16x3(x, "query")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.pad_cast_bf16(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.label_ranks(x.bfloat16(), x.bfloat16())
    with pytest.raises(RuntimeError, match="no CPU path"):
        metrics.label_ranks(x, x, None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        metrics.paired_retrieval_ranks(x, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        metrics.paired_retrieval_ranks(x, x, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        metrics.get_clip_metrics([x, x], [x, x], 100.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        metrics.zero_shot_accuracy(x, x.t(), torch.zeros(4, dtype=torch.long))


def test_shape_checks_and_the_empty_case():
    from open_clip_amd import metrics
    with pytest.raises(ValueError, match="matching shape"):
        metrics.paired_retrieval_ranks(torch.zeros(4, 32), torch.zeros(5, 32))
    with pytest.raises(ValueError, match="2D feature tensors"):
        metrics.paired_retrieval_ranks(torch.zeros(4), torch.zeros(4))
    with pytest.raises(ValueError, match="consistent feature dimension"):
        metrics.paired_retrieval_ranks([torch.zeros(2, 32), torch.zeros(2, 16)], [torch.zeros(2, 32), torch.zeros(2, 32)])
    with pytest.raises(ValueError, match="Unsupported retrieval dtype"):
        metrics._resolve_precision("fp8", torch.float32)
    i2t, t2i = metrics.paired_retrieval_ranks([], [])  # metrics.py:110-113
    assert i2t.numel() == 0 and t2i.numel() == 0 and i2t.dtype == torch.int64
    assert [metrics._resolve_precision(p, torch.bfloat16) for p in ("fp32", torch.float32, "bf16", "model", None)] == ["fp32", "fp32", "bf16", "bf16", "bf16"]
    # the reference takes any torch.dtype (metrics.py:19-20): fp16 features or torch.float16 rank on the split, which holds an fp16 value exactly
    assert metrics._resolve_precision("model", torch.float16) == "fp32" and metrics._resolve_precision(torch.float16, torch.float32) == "fp32"
    assert metrics._resolve_precision("model", torch.float32) == "fp32"


def test_metric_arithmetic_is_the_rules():
    """_add_rank_metrics on plain tensors (torch on the CPU is allowed for the [N] reductions) against the restated arithmetic, even and odd counts"""
    from open_clip_amd import metrics
    gen = torch.Generator().manual_seed(3)
    for n in (1, 2, 7, 10, 301):
        a, b = torch.randint(0, 40, (n,), generator=gen), torch.randint(0, 40, (n,), generator=gen)
        got = {}
        metrics._add_rank_metrics(got, "image_to_text", a)
        metrics._add_rank_metrics(got, "text_to_image", b)
        assert got == ru.rule_metrics(a, b)


def test_public_names_and_signatures():
    import open_clip_amd
    from open_clip_amd import metrics
    for name in ("get_clip_metrics", "zero_shot_accuracy", "paired_retrieval_ranks", "label_ranks"):
        assert getattr(open_clip_amd, name) is getattr(metrics, name)
    sig = inspect.signature(metrics.get_clip_metrics)
    assert list(sig.parameters) == ["image_features", "text_features", "logit_scale", "image_key", "text_key", "retrieval_chunk_size", "retrieval_device",
                                    "retrieval_dtype"]
    assert sig.parameters["image_key"].default == "image" and sig.parameters["text_key"].default == "text"
    assert sig.parameters["retrieval_chunk_size"].default == 4096 and sig.parameters["retrieval_device"].default is None
    assert sig.parameters["retrieval_dtype"].default is torch.float32
    assert list(inspect.signature(metrics.paired_retrieval_ranks).parameters) == ["image_features", "text_features", "precision", "device"]
    assert list(inspect.signature(metrics.label_ranks).parameters) == ["queries", "candidates", "labels", "precision"]
    zs = inspect.signature(metrics.zero_shot_accuracy)
    assert list(zs.parameters) == ["image_features", "classifier", "target", "topk", "precision"] and zs.parameters["topk"].default == (1, 5)


@needs_reference
def test_signature_is_the_references():
    from oracle.ref_shim import import_reference
    import_reference()
    from open_clip_train import metrics as ref
    from open_clip_amd import metrics
    ours, theirs = inspect.signature(metrics.get_clip_metrics), inspect.signature(ref.get_clip_metrics)
    assert [(p.name, p.default) for p in ours.parameters.values()] == [(p.name, p.default) for p in theirs.parameters.values()]
