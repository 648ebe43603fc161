#!/usr/bin/env python3
"""Writes tests/golden/large_walk_parent.npz: what the PARENT commit's kernels compute for the two large-array Blast links and the
4 x 4 pilot link on the inputs of tests/large_walk_cases.py -- counter blocks, per-realization symbol and bit error counts in both
arithmetics, |H^ - H|^2 and |H|^2 as raw float64 -- for tests/test_gpu_large_walk_parent.py, which holds the kernels of the tree to
it bit for bit.

Recorded from a build of the parent commit, on the GPU: build that commit's pyphysim_amd/csrc into a library elsewhere, then

    MCLE_LIBRARY=/path/to/parent/libmcle.so python scripts/make_golden_large_walk.py <parent commit hash> [output.npz]

The hash is stored in the fixture (key parent_commit).  Run without MCLE_LIBRARY it records the tree's own library, which is what a
later refactor of these kernels does with ITS parent."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from pyphysim_amd import _lib  # noqa: E402
from pyphysim_amd.engine import Engine  # noqa: E402

import large_walk_cases  # noqa: E402

if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "tests", "golden", "large_walk_parent.npz")
    eng = Engine(0, "f64")
    fixture = large_walk_cases.collect(eng)
    eng.close()
    fixture["parent_commit"] = np.array(sys.argv[1])
    fixture["counter_keys"] = np.array(large_walk_cases.COUNTER_KEYS)
    np.savez_compressed(out, **fixture)
    print("wrote %s from %s: %d arrays, %d bytes" % (out, os.path.relpath(_lib.LIB_PATH, REPO), len(fixture), os.path.getsize(out)))
