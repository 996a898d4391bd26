"""The retrieval rank rule restated in elementary torch (int64 / float64 on the CPU), and the input recipes of the retrieval-metric tests.

rank[r] = #{ j : s[r, j] > t[r]  or  (s[r, j] == t[r] and j < labels[r]) },  t[r] = s[r, labels[r]]

Written from the definition, one comparison per (query, candidate); nothing here is chunked and nothing is taken from the reference's code.
"""
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "retrieval_ranks.npz")
GOLDEN_N, GOLDEN_E, GOLDEN_SEED = 300, 32, 20240
METRIC_KEYS = ("mean_rank", "median_rank", "R@1", "R@5", "R@10")


def rule_ranks(scores, labels):
    """int64 [R] from a score matrix [R, N] of any exact dtype (int64 dots of integer features, float64 dots of real ones)"""
    labels = labels.long()
    t = scores.gather(1, labels[:, None])
    j = torch.arange(scores.shape[1])[None, :]
    return ((scores > t) | ((scores == t) & (j < labels[:, None]))).sum(dim=1)


def rank_band(scores, labels, delta):
    """(lo, hi) = (#{s > t + delta}, #{s >= t - delta} - 1): the ranks an evaluation whose scores differ from `scores` by at most delta / 2 can give"""
    t = scores.gather(1, labels.long()[:, None])
    return (scores > t + delta).sum(dim=1), (scores >= t - delta).sum(dim=1) - 1


def rule_metrics(i2t, t2i, image_key="image", text_key="text"):
    """the ten values from two rank vectors: mean + 1, floor(median) + 1 with the mean of the two middle values for an even count, fraction below k"""
    out = {}
    for name, ranks in ((f"{image_key}_to_{text_key}", i2t), (f"{text_key}_to_{image_key}", t2i)):
        r = sorted(int(v) for v in ranks)
        n = len(r)
        med = r[n // 2] if n % 2 else (r[n // 2 - 1] + r[n // 2]) / 2
        out[f"{name}_mean_rank"] = sum(r) / n + 1
        out[f"{name}_median_rank"] = math.floor(med) + 1
        for k in (1, 5, 10):
            out[f"{name}_R@{k}"] = sum(v < k for v in r) / n
    return out


def int_scores(q, c):
    return q.long() @ c.long().t()


def _integers(shape, gen):
    return torch.randint(-3, 4, shape, generator=gen, dtype=torch.int64)


def plant(q, c, labels):
    """hard rows, where the shapes have room for them: every candidate's last feature is -3 and query 2 is 3 * e_last (ALL its scores are -9: a padding
    column's 0 would beat the target), queries 0 and R - 1 are zero (all scores tie at 0), and the labelled candidate of the middle
    query is copied to one row below and one row above the label (exact ties on both sides of it)"""
    R, N = q.shape[0], c.shape[0]
    if R < 4 or N < 8:
        return q, c
    c[:, -1] = -3
    q[0] = 0
    q[R - 1] = 0
    q[2] = 0
    q[2, -1] = 3
    mid = R // 2
    lab = int(labels[mid])
    below, above = lab // 2, (lab + N) // 2
    if below < lab:
        c[below] = c[lab]
    if lab < above < N:
        c[above] = c[lab]
    return q, c


def exact_case(R, N, E, seed):
    """integer features in [-3, 3] (exact in bf16; every fp32 sum exact; lo parts zero): q [R, E], c [N, E], labels [R] (paired when R == N) -- int64"""
    gen = torch.Generator().manual_seed(seed)
    q, c = _integers((R, E), gen), _integers((N, E), gen)
    labels = torch.arange(R) if R == N else torch.randint(0, N, (R,), generator=gen)
    q, c = plant(q, c, labels)
    return q, c, labels


def golden_features(seed=GOLDEN_SEED, n=GOLDEN_N, e=GOLDEN_E):
    """(image, text) int64 [n, e] of the fixture recipe: text = image + noise (so that some pairs do rank first), the planted rows of ``plant``, plus
    duplicated captions and duplicated images"""
    gen = torch.Generator().manual_seed(seed)
    image = _integers((n, e), gen)
    text = (image + torch.randint(-3, 4, (n, e), generator=gen)).clamp(-3, 3)
    image, text = plant(image, text, torch.arange(n))
    if n >= 64:
        text[n - 7] = text[11]   # two captions of one wording, far apart
        text[12] = text[11]      # and next to each other
        image[n - 20] = image[40]
        image[5] = 0             # an all-zero image row
    return image, text


def load_golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def real_pair(E, n=777):
    """unit vectors x, y fp32 [n, E] with y correlated to x (a trained model's paired features in miniature): the recipe of the band tests"""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        x = torch.nn.functional.normalize(torch.randn(n, E), dim=-1)
        y = torch.nn.functional.normalize(0.35 * x + torch.nn.functional.normalize(torch.randn(n, E), dim=-1), dim=-1)
    return x, y


def padded(E):
    return (E + 31) // 32 * 32


def delta_fp32(E):
    """3 * 2^-18: the dropped lo.lo term and the residuals x - hi - lo of unit vectors; 3 Ep 2^-24: worst-case fp32 accumulation of 3 Ep terms"""
    return 3 * 2.0 ** -18 + 3 * padded(E) * 2.0 ** -24


def delta_bf16(E):
    """products of bf16 values are exact in fp32: only the accumulation of Ep terms rounds"""
    return padded(E) * 2.0 ** -24
