"""MI355X: the optimizers and the model EMA leave the bytes of the commit before they moved onto one table layer and one chunk walk.  Every case of
``tests.optim_util.golden_cases()`` runs; every array it leaves is compared, through its SHA-256 (tests/optim_util.py says why a digest), with
tests/golden/optim_parent.npz, which tools/optim_golden.py recorded on that commit.  A key missing on either side fails."""
import numpy as np
import pytest
import torch

from tests import optim_util as U

pytestmark = pytest.mark.gpu


def test_every_array_equals_the_parent_commits():
    assert torch.cuda.is_available(), "needs the MI355X"
    golden = np.load(U.GOLDEN)
    cases = U.golden_cases()
    assert len(cases) == 7
    got = {}
    for case in cases:
        arrays = U.run_golden_case(case, torch.device("cuda:0"))
        assert arrays, case["name"]
        got.update({f"{case['name']}/{k}": U.digest(v) for k, v in arrays.items()})
    assert sorted(got) == sorted(golden.files), sorted(set(got) ^ set(golden.files))
    differ = [k for k in sorted(got) if not np.array_equal(got[k], golden[k])]
    assert not differ, f"{len(differ)} of {len(got)} arrays differ from the parent commit's bytes: {differ}"
