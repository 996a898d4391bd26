"""Generates ``tests/golden/retrieval_ranks.npz``: the REFERENCE's retrieval ranks and metrics (open_clip_train/metrics.py ``_paired_retrieval_ranks`` and
``get_clip_metrics``) on the integer recipe of tests/retrieval_util.py.  TEST INFRASTRUCTURE ONLY; run where the reference can be imported (oracle/ref_shim.py):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_retrieval_golden.py

Recipe: ``golden_features()`` -- N = 300 paired rows of E = 32 integer features in [-3, 3] with duplicated rows, all-zero rows and a query whose scores are all
negative; fp32 on the CPU, where every dot product of such features is exact, so the ranks do not depend on chunking: chunk sizes 64 and 0 (= unchunked) are
both run and must agree.  The fixture holds data only: the features as int8, both rank vectors as int64, the ten metric values as float64.
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.ref_shim import import_reference  # noqa: E402
from tests.retrieval_util import GOLDEN, METRIC_KEYS, golden_features  # noqa: E402


def main():
    import_reference()
    from open_clip_train import metrics as ref

    image, text = golden_features()
    fi, ft = image.float(), text.float()
    runs = [ref._paired_retrieval_ranks(fi, ft, 100.0, chunk, device=None, retrieval_dtype=torch.float32) for chunk in (64, 0)]
    assert all(np.array_equal(a, b) for a, b in zip(runs[0], runs[1])), "chunked and unchunked reference ranks differ"
    # the list-of-batches form of the same features (metrics.py:65-92) must give the same ranks
    batches = lambda f: [f[i:i + 37] for i in range(0, f.shape[0], 37)]  # noqa: E731
    listed = ref._paired_retrieval_ranks(batches(fi), batches(ft), 100.0, 64, device=None, retrieval_dtype=torch.float32)
    assert all(np.array_equal(a, b) for a, b in zip(runs[0], listed))
    metrics = ref.get_clip_metrics(fi, ft, 100.0, retrieval_chunk_size=64)
    assert metrics == ref.get_clip_metrics(fi, ft, 100.0, retrieval_chunk_size=0)
    out = {"image": image.numpy().astype(np.int8), "text": text.numpy().astype(np.int8),
           "image_to_text": runs[0][0].astype(np.int64), "text_to_image": runs[0][1].astype(np.int64)}
    for side in ("image_to_text", "text_to_image"):
        for key in METRIC_KEYS:
            out[f"metric/{side}_{key}"] = np.float64(metrics[f"{side}_{key}"])
    np.savez_compressed(GOLDEN, **out)
    print(os.path.basename(GOLDEN), "bytes", os.path.getsize(GOLDEN), {k: float(v) for k, v in metrics.items()})


if __name__ == "__main__":
    main()
