"""MI355X: LayerNorm forward and backward and the deterministic wgrad leave the bytes of the commit that still had the variants only a developer
knob reached (the wgrad's 32x32x16 main loop, LayerNorm's default-cache-policy and forced one-row kernels).  Every case of
``tests.variants_parent_util`` runs; every array it leaves is compared, through its SHA-256, with tests/golden/variants_parent.npz, which
tools/variants_parent_golden.py recorded with that commit's library.  The deterministic forms cut their work by the device's CU count: the
fixture holds the count it was recorded on, and another count fails here before anything is compared.  A key missing on either side fails."""
import numpy as np
import pytest
import torch

from tests import variants_parent_util as U

pytestmark = pytest.mark.gpu


def test_every_array_equals_the_parent_commits():
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    golden = np.load(U.GOLDEN)
    assert U.cu_count(dev) == int(golden[U.CU_KEY]), f"the fixture was recorded on {int(golden[U.CU_KEY])} CUs, this device has {U.cu_count(dev)}"
    assert len(U.fwd_cases()) == 72 and len(U.bwd_cases()) == 168
    got = {k: U.digest(v) for k, v in U.run_all(dev).items()}
    want = [k for k in golden.files if k != U.CU_KEY]
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
    differ = [k for k in sorted(got) if not np.array_equal(got[k], golden[k])]
    assert not differ, f"{len(differ)} of {len(got)} arrays differ from the parent commit's bytes: {differ}"
