"""Records tests/golden/optim_parent.npz: one SHA-256 per array that ``tests.optim_util.golden_cases()`` leave behind (parameters, optimizer state,
operand copies, gradient norms, EMA buffers) after three steps of NativeAdamW / NativeNAdamW / NativeMuon or three updates of the model EMA.

    python tools/optim_golden.py [--out tests/golden/optim_parent.npz] [--full all_bytes.npz] [--check]

The committed file was written ONCE, on the MI355X, with the package of the commit before the optimizers and the EMA moved onto one table layer
(open_clip_amd/tables.py) and the shared kernel helpers (csrc/ocn_common.h, csrc/optim.hip); tests/test_optim_parent_gpu.py holds every later tree to those bytes.  Run it again
only with a tree whose results are known to be right (a change of an update rule itself), and say so in the commit.  ``--full`` also writes the
arrays themselves (3 MB, not for git) so that two trees can be compared element by element; ``--check`` writes no digests and compares with
those of ``--out``.  Needs the GPU: there is no CPU fallback."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import optim_util as U  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=U.GOLDEN)
    ap.add_argument("--full", default=None)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X (no CPU fallback)"
    from open_clip_amd import _lib
    arrays = U.run_all(torch.device("cuda:0"))
    digests = {k: U.digest(v) for k, v in arrays.items()}
    if a.full:
        os.makedirs(os.path.dirname(os.path.abspath(a.full)), exist_ok=True)
        np.savez(a.full, **arrays)
    if a.check:
        want = np.load(a.out)
        bad = sorted(set(want.files) ^ set(digests)) + [k for k in digests if k in want.files and not np.array_equal(want[k], digests[k])]
        print(f"{len(digests)} arrays, {len(bad)} differ from {a.out}: {bad}")
        sys.exit(1 if bad else 0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **digests)
    print(f"wrote {a.out}: {len(digests)} arrays of {len(U.golden_cases())} cases, {sum(v.nbytes for v in arrays.values())} bytes behind them, "
          f"library {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
