"""Records tests/golden/resample_parent.npz: the uint8 outputs of ocn_resized_crop_u8 and ocn_resample_u8 on ``tests.resample_util.golden_cases()``.

    OCN_LIB_PATH=<a build of the library> python tools/resample_golden.py [--out tests/golden/resample_parent.npz]

The committed file was written ONCE, with the library of the commit before csrc/resized_crop.hip and csrc/resample.hip became one tile routine;
tests/test_resample_gpu.py holds every later library to those bytes.  Run it again only with a library whose outputs are known to be right (a
change of the filter itself), and say so in the commit.  Needs the GPU: there is no CPU fallback."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import resample_util as U  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=U.GOLDEN)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X (no CPU fallback)"
    from open_clip_amd import _lib
    dev = torch.device("cuda:0")
    outs = {case["name"]: U.run_golden_case(case, dev) for case in U.golden_cases()}
    assert all(v.dtype == np.uint8 for v in outs.values())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **outs)
    print(f"wrote {a.out}: {len(outs)} cases, {sum(v.size for v in outs.values())} bytes of output, library {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
