"""GPU: open_clip_amd.metrics (ocn_label_ranks / ocn_split_bf16x3) against the rank rule restated in tests/retrieval_util.py -- exactly on integer
features, inside the band that the number formats allow on real-valued ones."""
import functools

import numpy as np
import pytest
import torch

from tests import retrieval_util as ru

pytestmark = pytest.mark.gpu

DEV = "cuda"
EXACT_E = (32, 64, 96, 20, 80)  # 20 and 80: padded to 32 / 96 columns per segment
EXACT_SHAPES = ((1, 1), (5, 3), (127, 127), (129, 129), (300, 300), (257, 1000), (1000, 257))
PRECISIONS = ("fp32", "bf16")


@pytest.fixture(scope="module")
def metrics():
    from open_clip_amd import metrics as m
    return m


def _dev(t):
    return t.float().to(DEV)


# ---- 1. exact -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,N", EXACT_SHAPES)
def test_integer_features_rank_exactly(metrics, R, N):
    """integer features are exact in bf16, their lo parts are zero and every fp32 sum is exact: both precisions must EQUAL the int64 rule.  One tile
    and many, ragged R and N, padded E; duplicated candidates on both sides of the label, all-zero queries, a query whose scores are all negative"""
    for E in EXACT_E:
        q, c, labels = ru.exact_case(R, N, E, seed=1000 * R + N + E)
        want = ru.rule_ranks(ru.int_scores(q, c), labels)
        if R >= 4 and N >= 8:
            assert (ru.int_scores(q, c)[2] < 0).all()
        for precision in PRECISIONS:
            got = metrics.label_ranks(_dev(q), _dev(c), labels.to(DEV), precision)
            assert got.dtype == torch.int64 and got.shape == (R,) and got.is_cuda
            assert torch.equal(got.cpu(), want), (E, precision, (got.cpu() != want).nonzero().flatten()[:8].tolist())
            if R == N:  # paired: labels=None is arange
                assert torch.equal(metrics.label_ranks(_dev(q), _dev(c), None, precision).cpu(), want), (E, precision)


def test_many_candidate_tiles_per_workgroup(metrics):
    """few queries, N beyond 1024 candidate tiles: the launch gives every workgroup SEVERAL tiles to walk (its counts carry over from tile to tile) and the
    last tile is ragged -- the only shape at which that loop runs more than once"""
    R, N, E = 5, 2 * 262144 + 77, 32
    q, c, labels = ru.exact_case(R, N, E, seed=4)
    want = ru.rule_ranks(ru.int_scores(q, c), labels)
    for precision in PRECISIONS:
        assert torch.equal(metrics.label_ranks(_dev(q), _dev(c), labels.to(DEV), precision).cpu(), want), precision


def test_bf16_features_and_model_precision(metrics):
    """bf16 features with precision 'model' take the one-segment path without a cast (E % 32 == 0) or with a padded one"""
    for E in (64, 20):
        q, c, labels = ru.exact_case(129, 300, E, seed=9)
        want = ru.rule_ranks(ru.int_scores(q, c), labels)
        got = metrics.label_ranks(_dev(q).bfloat16(), _dev(c).bfloat16(), labels.to(DEV), "model")
        assert torch.equal(got.cpu(), want), E


@pytest.mark.parametrize("precision", PRECISIONS)
def test_fixture_ranks_and_metrics(metrics, precision):
    g = ru.load_golden()
    image, text = torch.from_numpy(g["image"]), torch.from_numpy(g["text"])
    dtype = torch.float32 if precision == "fp32" else "bf16"
    i2t, t2i = metrics.paired_retrieval_ranks(_dev(image), _dev(text), precision=precision)
    assert np.array_equal(i2t.cpu().numpy(), g["image_to_text"]) and np.array_equal(t2i.cpu().numpy(), g["text_to_image"])
    got = metrics.get_clip_metrics(_dev(image), _dev(text), 100.0, retrieval_dtype=dtype)
    assert len(got) == 10
    for key, value in got.items():
        assert isinstance(value, float) and value == float(g["metric/" + key]), key
    named = metrics.get_clip_metrics(_dev(image), _dev(text), torch.tensor(14.3), image_key="a", text_key="b", retrieval_chunk_size=0, retrieval_dtype=dtype)
    assert named == {k.replace("image", "a").replace("text", "b"): v for k, v in got.items()}


def test_split_bf16x3_layout():
    """[hi | lo | hi] for queries, [hi | hi | lo] for candidates, zero padding per segment; hi = bf16(x), lo = bf16(x - hi)"""
    from open_clip_amd import ops
    x, _ = ru.real_pair(80, n=37)
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    for role, order in (("query", (hi, lo, hi)), ("candidate", (hi, hi, lo))):
        out = ops.split_bf16x3(x.to(DEV), role).cpu()
        assert out.shape == (37, 3 * 96) and out.dtype == torch.bfloat16
        for s, part in enumerate(order):
            assert torch.equal(out[:, 96 * s:96 * s + 80], part), (role, s)
            assert (out[:, 96 * s + 80:96 * (s + 1)] == 0).all()


# ---- 2. / 3. real values inside the band -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _real(E):
    x, y = ru.real_pair(E)
    return x, y, x.to(DEV), y.to(DEV)


@functools.lru_cache(maxsize=None)
def _bands(E, precision):
    """(lo, hi) of both directions from float64 scores: of the fp32 inputs (fp32 mode) or of the bf16-rounded operands (bf16 mode)"""
    x, y, _, _ = _real(E)
    if precision == "bf16":
        x, y = x.bfloat16(), y.bfloat16()
    delta = ru.delta_fp32(E) if precision == "fp32" else ru.delta_bf16(E)
    s = x.double() @ y.double().t()
    paired = torch.arange(x.shape[0])
    return ru.rank_band(s, paired, delta), ru.rank_band(s.t().contiguous(), paired, delta)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("E", [64, 80])
def test_real_features_rank_inside_the_band(metrics, E, precision):
    """every row: #{s > t + delta} <= rank <= #{s >= t - delta} - 1 with float64 s; fp32 mode: delta = 3 * 2^-18 + 3 Ep 2^-24 (dropped lo.lo and residuals of
    unit vectors + worst-case fp32 accumulation of 3 Ep terms); bf16 mode: delta = Ep 2^-24 against the bf16-rounded operands (exact products)"""
    _, _, xd, yd = _real(E)
    got = metrics.paired_retrieval_ranks(xd, yd, precision=precision)
    for name, ranks, (lo, hi) in zip(("image_to_text", "text_to_image"), got, _bands(E, precision)):
        ranks = ranks.cpu()
        wide = int((hi > lo).sum())
        print(f"E={E} {precision} {name}: rows with hi > lo: {wide} of {len(lo)}; rows outside the band: {int(((ranks < lo) | (ranks > hi)).sum())}")
        assert wide <= 0.02 * len(lo)  # a condition on the inputs: the band decides all but a few rows
        assert bool(((ranks >= lo) & (ranks <= hi)).all()), (name, ((ranks < lo) | (ranks > hi)).nonzero().flatten()[:8].tolist())


def test_target_scores_and_classifier_reuse(metrics):
    """ops.label_ranks(return_target=True): t[r] is within the fp32-mode delta (the bound on one score) of the float64 label score and EQUALS the score the rank launch
    sees for the label column (rank 0 for a query whose label scores best, strictly); zero_shot_accuracy prepares a classifier once and again after an
    in-place update"""
    from open_clip_amd import ops
    E = 80
    x, y, xd, yd = _real(E)
    labels = torch.arange(777).flip(0).contiguous()
    rank, t = ops.label_ranks(ops.split_bf16x3(xd, "query"), ops.split_bf16x3(yd, "candidate"), labels.int().to(DEV), return_target=True)
    s = x.double() @ y.double().t()
    err = (t.cpu().double() - s.gather(1, labels[:, None])[:, 0]).abs().max()
    print(f"target scores: max |t - float64| = {float(err):.3e} (delta = {ru.delta_fp32(E):.3e})")
    assert float(err) <= ru.delta_fp32(E)
    lo, hi = ru.rank_band(s, labels, ru.delta_fp32(E))
    assert bool(((rank.cpu() >= lo) & (rank.cpu() <= hi)).all())
    cls = yd.t().contiguous()  # [E, C]
    target = torch.arange(777, device=DEV)
    first = metrics.zero_shot_accuracy(xd, cls, target)
    assert metrics.zero_shot_accuracy(xd, cls, target) == first and len(metrics._classifier_operand) == 1
    cls.neg_()  # in place: the cached operand must not be used again
    flipped = metrics.zero_shot_accuracy(xd, cls, target)
    assert flipped == metrics.zero_shot_accuracy(xd, cls.clone(), target) and flipped != first


# ---- 4. bit-identical duplicates on real values --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_duplicated_candidates_tie_exactly(metrics, precision):
    """copies of candidate i at rows that did not beat it: the rank of query i rises by exactly the number of copies BELOW i (equal scores, smaller index),
    whatever tile, lane or register the copies land in -- the target and every other score leave one routine"""
    E, i = 64, 400
    x, y, xd, yd = _real(E)
    s = (x.double() @ y.double().t())[i]
    losers = (s < s[i] - 0.05).nonzero().flatten()
    below, above = losers[losers < i], losers[losers > i]
    below = torch.stack([below[0], below[len(below) // 2], below[-1]])  # rows 0.., mid, i-1..: other tiles of 256 and the label's own
    above = torch.stack([above[0], above[-1]])
    base = metrics.label_ranks(xd, yd, None, precision)
    y2 = yd.clone()
    y2[torch.cat([below, above]).to(DEV)] = yd[i]
    got = metrics.label_ranks(xd, y2, None, precision)
    assert int(got[i]) == int(base[i]) + len(below)


# ---- 5. input forms ----------------------------------------------------------------------------------------------------------------------------------------
def test_input_forms_agree(metrics):
    E = 80
    x, y, xd, yd = _real(E)
    want = [r.cpu() for r in metrics.paired_retrieval_ranks(xd, yd)]
    cuts = (0, 100, 100, 333, 777)  # an empty batch among them
    batches = lambda t: [t[a:b] for a, b in zip(cuts[:-1], cuts[1:])]  # noqa: E731
    forms = {
        "list of batches": metrics.paired_retrieval_ranks(batches(xd), batches(yd)),
        "row-strided view": metrics.paired_retrieval_ranks(torch.cat([xd, yd], dim=1)[:, :E], torch.cat([yd, xd], dim=1)[:, :E]),
        "transposed view": metrics.paired_retrieval_ranks(xd.t().contiguous().t(), yd.t().contiguous().t()),
        "cpu tensors + device": metrics.paired_retrieval_ranks(x, y, device=DEV),
        "cpu batches + device": metrics.paired_retrieval_ranks(batches(x), batches(y), device=torch.device(DEV)),
    }
    for name, got in forms.items():
        assert all(g.is_cuda for g in got)
        assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1]), name
    assert metrics.get_clip_metrics(x, y, 100.0, retrieval_device=DEV) == metrics.get_clip_metrics(xd, yd, 100.0)
    assert not xd.t().contiguous().t().is_contiguous()
    with pytest.raises(ValueError, match=r"every label must lie in \[0, 777\)"):
        metrics.label_ranks(xd, yd, torch.full((777,), 777))


# ---- 6. zero-shot ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes", [257, 1000])
def test_zero_shot_counts_exactly(metrics, classes):
    q, c, target = ru.exact_case(300, classes, 64, seed=classes)
    ranks = ru.rule_ranks(ru.int_scores(q, c), target)
    topk = (1, 5, 10)
    for precision in PRECISIONS:
        got = metrics.zero_shot_accuracy(_dev(q), _dev(c).t(), target.to(DEV), topk=topk, precision=precision)
        assert got == [float((ranks < k).sum()) for k in topk], precision
    assert len(metrics.zero_shot_accuracy(_dev(q), _dev(c).t(), target.to(DEV))) == 2  # topk=(1, 5), like the reference's call


def test_zero_shot_counts_inside_the_band(metrics):
    """real values: the count at k lies in [#(hi < k), #(lo < k)], and equals the top-k count of the float64 scores when no row is ambiguous at k"""
    E = 64
    x, y, xd, yd = _real(E)
    (lo, hi), _ = _bands(E, "fp32")
    s = x.double() @ y.double().t()
    target = torch.arange(x.shape[0])
    topk = (1, 5, 10)
    got = metrics.zero_shot_accuracy(xd, yd.t(), target.to(DEV), topk=topk)
    pred = s.topk(max(topk), dim=1).indices  # zero_shot.py:15-18 restated on the exact scores
    for k, count in zip(topk, got):
        floor, ceil = int((hi < k).sum()), int((lo < k).sum())
        assert floor <= count <= ceil, (k, floor, count, ceil)
        if floor == ceil:
            assert count == float((pred[:, :k] == target[:, None]).any(dim=1).sum()), k
