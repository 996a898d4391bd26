"""Records tests/golden/variants_parent.npz: one SHA-256 per array that ``tests.variants_parent_util.run_all`` leaves behind (LayerNorm forward and
backward over every dispatch edge, the deterministic wgrad) plus the device's CU count.

    OCN_LIB_PATH=<library of the commit to record> python tools/variants_parent_golden.py [--out tests/golden/variants_parent.npz] [--check]

The committed file was written ONCE, on the MI355X, with the library of the commit before the wgrad's 32x32x16 main loop and LayerNorm's
cache-policy variants were removed (same ABI number: loaded through ``OCN_LIB_PATH``); tests/test_variants_parent_gpu.py holds every later tree to
those bytes.  Run it again only with a tree whose results are known to be right, and say so in the commit.  ``--check`` writes nothing and
compares with the digests of ``--out``.  Needs the GPU: there is no CPU fallback."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import variants_parent_util as U  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=U.GOLDEN)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X (no CPU fallback)"
    from open_clip_amd import _lib
    dev = torch.device("cuda:0")
    arrays = U.run_all(dev)
    digests = {k: U.digest(v) for k, v in arrays.items()}
    digests[U.CU_KEY] = np.asarray(U.cu_count(dev), dtype=np.int32)
    if a.check:
        want = np.load(a.out)
        bad = sorted(set(want.files) ^ set(digests)) + [k for k in digests if k in want.files and not np.array_equal(want[k], digests[k])]
        print(f"{len(digests) - 1} arrays, {len(bad)} differ from {a.out}: {bad}")
        sys.exit(1 if bad else 0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **digests)
    print(f"wrote {a.out}: {len(arrays)} arrays, {sum(v.nbytes for v in arrays.values())} bytes behind them, {int(digests[U.CU_KEY])} CUs, "
          f"library {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
