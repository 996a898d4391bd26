"""Validation metrics on the MI355X: retrieval ranks, R@k and zero-shot top-k (the reference's ``open_clip_train/metrics.py`` and
``open_clip_train/zero_shot.py::accuracy``) from ONE native op, ``ops.label_ranks``: the rank of each query's labelled candidate among all candidates,
counted inside the MFMA tile that forms the scores.  No N x N matrix, no chunk loop, no ATen matmul / compare / sum.

Precision (the reference's ``--val-retrieval-precision``, metrics.py:14-21):
    "fp32" (default; also ``torch.float32``)  every feature is split into bf16 hi + lo parts (``ops.split_bf16x3``) and one K = 3 E product sums
                                              hi.hi + lo.hi + hi.lo in fp32: the fp32 product short of its lo.lo term (relative 2^-18)
    "bf16" (also ``torch.bfloat16``)          the features rounded to bf16, products exact, fp32 accumulation
    "model" / None                            by the dtype of the features: bf16 features -> "bf16", fp32 / fp16 / fp64 features -> "fp32" (an fp16 value is
                                              hi + lo exactly, so fp16 features are ranked on their exact products; ``torch.float16`` is taken the same way)
Only the scores and the counts are native.  Moving, concatenating, widening (``.float()``) and zero-padding the [N, E] operands and the reductions over the
[N] rank vectors are plain torch: O(N E) and O(N) next to the O(N^2 E) product.
Ties are broken as the reference does (metrics.py:156-163): a candidate with the target's score ranks ahead of it only when its index is smaller.  The
target score comes out of the same tile code as every other score, so duplicated captions / images tie exactly.
"""
import torch

from . import ops

DEFAULT_RETRIEVAL_CHUNK_SIZE = 4096  # the reference's default (metrics.py:5); accepted, never used: nothing is chunked here

__all__ = ["label_ranks", "paired_retrieval_ranks", "get_clip_metrics", "zero_shot_accuracy", "DEFAULT_RETRIEVAL_CHUNK_SIZE"]


def _resolve_precision(precision, feature_dtype):
    """'fp32' or 'bf16' from the reference's spellings of retrieval_dtype (metrics.py:14-21)"""
    if precision is None or precision == "model":
        precision = feature_dtype
    if precision in ("fp32", torch.float32, torch.float16, torch.float64):
        return "fp32"  # fp16 features (`--precision amp` with `model`) are exact in the hi + lo split; fp64 is ranked at fp32's precision
    if precision in ("bf16", torch.bfloat16):
        return "bf16"
    raise ValueError(f"Unsupported retrieval dtype: {precision!r} (this package ranks in 'fp32' or 'bf16')")


def _no_cpu_path(what):
    return RuntimeError(f"open_clip_amd: {what} must live on the MI355X (pass a CUDA tensor or a device); there is no CPU path")


def _operand(x, role, precision):
    """fp32 / bf16 features [R, E] on the device -> the bf16 operand of ``ops.label_ranks`` for this precision"""
    if precision == "fp32":
        return ops.split_bf16x3(x.float(), role)
    if x.dtype == torch.bfloat16 and x.shape[1] % 32 == 0:
        return x
    return ops.pad_cast_bf16(x.float())


def _checked_labels(labels, R, N, device):
    """int32 [R] on the device; a label outside [0, N) raises here (one host read), where the reference's gather would"""
    labels = torch.as_tensor(labels)
    if labels.shape != (R,) or labels.is_floating_point():
        raise ValueError(f"label_ranks: labels must be {R} integers")
    labels = labels.to(device=device)
    if bool(((labels < 0) | (labels >= N)).any()):
        raise ValueError(f"label_ranks: every label must lie in [0, {N})")
    return labels.to(torch.int32)


def label_ranks(queries, candidates, labels, precision="fp32"):
    """``rank[r]`` = how many candidates score above query r's labelled one (ties: smaller index first); int64 [R] on the device.

    queries [R, E], candidates [N, E] (device tensors, fp32 or bf16); labels: integer [R] with values in [0, N), or None for ``arange(R)``."""
    if not (torch.is_tensor(queries) and torch.is_tensor(candidates)) or queries.dim() != 2 or candidates.dim() != 2:
        raise ValueError("Retrieval metrics expect 2D feature tensors.")
    if queries.shape[1] != candidates.shape[1]:
        raise ValueError("Retrieval feature tensors must have a consistent feature dimension.")
    if not queries.is_cuda or not candidates.is_cuda:
        raise _no_cpu_path("label_ranks: queries and candidates")
    precision = _resolve_precision(precision, queries.dtype)
    R, N = queries.shape[0], candidates.shape[0]
    if R == 0:
        return torch.empty(0, dtype=torch.int64, device=queries.device)
    if N == 0 or queries.shape[1] == 0:
        raise ValueError("label_ranks: needs at least one candidate and one feature column")
    if labels is None:
        if R > N:
            raise ValueError(f"label_ranks: paired labels arange({R}) leave [0, {N})")
    else:
        labels = _checked_labels(labels, R, N, queries.device)
    rank = ops.label_ranks(_operand(queries, "query", precision), _operand(candidates, "candidate", precision), labels)
    return rank.long()


def _feature_shape(features):
    """(rows, columns) of a tensor or a list of per-batch tensors, with the reference's checks (metrics.py:30-47)"""
    if torch.is_tensor(features):
        if features.ndim != 2:
            raise ValueError("Retrieval metrics expect 2D feature tensors.")
        return tuple(features.shape)
    rows, dim = 0, None
    for f in features:
        if f.ndim != 2:
            raise ValueError("Retrieval metrics expect 2D feature tensors.")
        if dim is None:
            dim = f.shape[1]
        elif f.shape[1] != dim:
            raise ValueError("Retrieval feature tensors must have a consistent feature dimension.")
        rows += f.shape[0]
    return (rows, 0 if dim is None else dim)


def _gather_features(features, device):
    """one device tensor from a tensor or a list of per-batch tensors (concatenated on the device)"""
    parts = [features] if torch.is_tensor(features) else [f for f in features if f.shape[0] > 0]
    parts = [p.to(device=device, non_blocking=True) for p in parts]
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)


def paired_retrieval_ranks(image_features, text_features, precision="fp32", device=None):
    """(image_to_text, text_to_image) ranks, int64 [N] on the device, of N paired features (metrics.py:95-169: item i of one side is labelled item i of the
    other).  Each argument is a tensor or a list of per-batch tensors; CPU inputs are moved to ``device``."""
    image_shape, text_shape = _feature_shape(image_features), _feature_shape(text_features)
    if image_shape != text_shape:
        raise ValueError("Paired retrieval metrics require image and text features with matching shape.")
    first = image_features if torch.is_tensor(image_features) else next((f for f in image_features if f.shape[0] > 0), None)
    if device is None:
        if first is not None and first.is_cuda:
            device = first.device
        elif image_shape[0] > 0:
            raise _no_cpu_path("paired_retrieval_ranks: the features (or `device`)")
    else:
        device = torch.device(device)
        if device.type != "cuda":
            raise _no_cpu_path("paired_retrieval_ranks: `device`")
    if image_shape[0] == 0:
        empty = torch.empty(0, dtype=torch.int64, device=device)
        return empty, empty
    image = _gather_features(image_features, device)
    text = _gather_features(text_features, device)
    precision = _resolve_precision(precision, first.dtype)
    # two products, one per direction: each has its own operand roles ([hi | lo | hi] for whoever asks), and sharing one would halve nothing but the
    # MFMA work of a metric that runs once per validation
    return label_ranks(image, text, None, precision), label_ranks(text, image, None, precision)


def _add_rank_metrics(metrics, name, ranks):
    """metrics.py:172-176 on a device rank vector: numpy's mean, floor(median) + 1 (an even count averages the two middle values) and R@k"""
    n = ranks.numel()
    if n == 0:
        for key in ("mean_rank", "median_rank", "R@1", "R@5", "R@10"):
            metrics[f"{name}_{key}"] = float("nan")
        return
    ordered = torch.sort(ranks).values
    middle = int(ordered[n // 2]) if n % 2 else (int(ordered[n // 2 - 1]) + int(ordered[n // 2])) // 2
    metrics[f"{name}_mean_rank"] = int(ranks.sum()) / n + 1
    metrics[f"{name}_median_rank"] = float(middle + 1)
    for k in (1, 5, 10):
        metrics[f"{name}_R@{k}"] = int((ranks < k).sum()) / n


def get_clip_metrics(
        image_features,
        text_features,
        logit_scale,
        image_key="image",
        text_key="text",
        retrieval_chunk_size=DEFAULT_RETRIEVAL_CHUNK_SIZE,
        retrieval_device=None,
        retrieval_dtype=torch.float32,
):
    """The reference's ``get_clip_metrics`` (metrics.py:179-202): mean_rank, median_rank, R@1, R@5 and R@10 in both directions, ten python floats.

    ``logit_scale`` and ``retrieval_chunk_size`` are accepted for the signature and NOT used: a positive scale changes no rank, and nothing is chunked --
    the scores live in MFMA accumulators only.  ``retrieval_dtype`` takes the reference's spellings (see the module docstring)."""
    i2t, t2i = paired_retrieval_ranks(image_features, text_features, precision=retrieval_dtype, device=retrieval_device)
    metrics = {}
    _add_rank_metrics(metrics, f"{image_key}_to_{text_key}", i2t)
    _add_rank_metrics(metrics, f"{text_key}_to_{image_key}", t2i)
    return metrics


_classifier_operand = []  # at most one entry: (classifier, its version, precision, candidate operand), see zero_shot_accuracy


def _classifier_candidates(classifier, precision):
    """the [C, K] candidate operand of a [E, C] classifier, prepared once per classifier: ``run_zero_shot_classifier`` calls with the same tensor for
    every batch, and transposing + splitting it costs as much as a small batch's ranks.  The entry holds the classifier itself (so its memory cannot be
    handed to another tensor while the entry lives) and its version counter (an in-place update prepares it again); one entry is kept."""
    for held, version, prec, operand in _classifier_operand:
        same = held is classifier or (held.data_ptr() == classifier.data_ptr() and held.shape == classifier.shape and held.stride() == classifier.stride()
                                      and held.dtype == classifier.dtype)
        if same and version == classifier._version and prec == precision:
            return operand
    operand = _operand(classifier.t(), "candidate", precision)
    _classifier_operand[:] = [(classifier, classifier._version, precision, operand)]
    return operand


def zero_shot_accuracy(image_features, classifier, target, topk=(1, 5), precision="fp32"):
    """How many rows have their target class among the k best of ``image_features @ classifier``, for each k of ``topk``: the reference's
    ``accuracy(100. * image_features @ classifier, target, topk)`` (zero_shot.py:15-18, 119-122).  ``classifier`` is [E, C] as ``build_zero_shot_classifier``
    returns it; its operand is prepared on the first call and reused while the same tensor comes back.  A row is correct at k when the rank of its target
    class is below k.  Like the reference's ``.item()`` per k, a call reads its results on the host (one more read checks the targets' range)."""
    if not torch.is_tensor(classifier) or classifier.dim() != 2:
        raise ValueError("zero_shot_accuracy: classifier must be a 2D [E, C] tensor")
    if not torch.is_tensor(image_features) or image_features.dim() != 2 or image_features.shape[1] != classifier.shape[0]:
        raise ValueError("zero_shot_accuracy: image_features must be [B, E] for a [E, C] classifier")
    if not image_features.is_cuda or not classifier.is_cuda:
        raise _no_cpu_path("zero_shot_accuracy: image_features and classifier")
    precision = _resolve_precision(precision, image_features.dtype)
    B, C = image_features.shape[0], classifier.shape[1]
    if B == 0:
        return [0.0 for _ in topk]
    labels = _checked_labels(target, B, C, image_features.device)
    ranks = ops.label_ranks(_operand(image_features, "query", precision), _classifier_candidates(classifier, precision), labels)
    below = torch.stack([(ranks < k).sum() for k in topk]).tolist()  # one host read for every k
    return [float(v) for v in below]
