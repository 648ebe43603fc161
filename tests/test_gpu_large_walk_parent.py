"""GPU: the two large-array Blast links and the 4 x 4 pilot link reproduce, bit for bit and in BOTH arithmetics, what the commit
before their shared code (csrc/mimo_large_link.hpp, csrc/pilot_block.hpp) computed: tests/golden/large_walk_parent.npz, recorded
from a build of that commit by scripts/make_golden_large_walk.py on the inputs of tests/large_walk_cases.py.

The complex64 tests of these links allow 3 symbol errors of difference per realization against the NumPy restatement and would
not notice a reordered product; this comparison does: every counter block and every per-realization count array with
numpy.array_equal, |H^ - H|^2 and |H|^2 by their bit patterns."""
import numpy as np
import pytest

from conftest import load_golden
from large_walk_cases import collect

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def got(engine):
    return collect(engine)


def test_every_recorded_array_is_reproduced(got):
    want = load_golden("large_walk_parent")
    keys = sorted(set(want.files) - {"parent_commit", "counter_keys"})
    assert keys == sorted(got) and len(keys) > 300
    wrong = []
    for k in keys:
        a, b = got[k], want[k]
        same = a.shape == b.shape and a.dtype == b.dtype and (np.array_equal(a.view(np.uint64), b.view(np.uint64))
                                                              if a.dtype == np.float64 else np.array_equal(a, b))
        if not same:
            wrong.append(k)
            print(k, "differs from parent", str(want["parent_commit"])[:7], "in", int(np.sum(a != b)) if a.shape == b.shape else "shape")
    assert not wrong, wrong
