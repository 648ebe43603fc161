#!/usr/bin/env python3
"""Writes tests/golden/g7_ia_envelope.npz: the 50-digit results of the general-geometry IA solver over the case table of
tests/ia_general_oracle.py, for tests/test_ia_general_envelope_cpu.py and tests/test_gpu_ia_general_envelope.py.

Per case and realization (leading axis of every array), rounded to f64:
  PF [K, nt, nt] = F_k F_k^H and PU [K, nr, nr] = U_k^H U_k (Hermitian, packed into one real matrix each: herm_pack),
  sinr [K, max(nr, nt)] per stream (zero padded), capacity, Ns_final [K], iterations, every_capacity (brute force),
  cost [6]: the leakage after 0, 1, 2, 3, 5, 8 iterations (alt-min and min-leakage; NaN past the last iteration run),
  e_np [4]: the error of the f64 NumPy oracle (oracle.ia.general_solve) against the mp result -- capacity, sinr, PF, PU,
  kappa [4]: sensitivity / 1e-14 of the same four, margins [5]: stop, select, cond, phase, stop0.
Slack cases keep kappa, margins and cost only.  Channels and starts are seeds (ia_general_oracle.draw), not matrices.

Pure Python at 50 digits: minutes on a few cores.  usage: python scripts/make_golden_ia_envelope.py [jobs]
"""
import multiprocessing
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import ia_general_oracle as iao  # noqa: E402


def _one(name):
    return name, iao.case_fields(iao.CASE_BY_NAME[name])


def build_fixture(jobs):
    # longest first, so that the pool drains evenly
    names = sorted(iao.CASE_BY_NAME, key=lambda n: -(iao.CASE_BY_NAME[n]["max_iterations"] * iao.CASE_BY_NAME[n]["K"]
                                                       * max(iao.CASE_BY_NAME[n]["nr"], iao.CASE_BY_NAME[n]["nt"]) ** 2))
    with multiprocessing.Pool(jobs) as pool:
        done = {}
        for name, fields in pool.imap_unordered(_one, names):
            done[name] = fields
            print("%3d/%d %s" % (len(done), len(names), name), flush=True)
    return iao.pack_fixture({c["name"]: done[c["name"]] for c in iao.CASES})


if __name__ == "__main__":
    fixture = build_fixture(int(sys.argv[1]) if len(sys.argv) > 1 else min(8, os.cpu_count() or 1))
    np.savez_compressed(iao.GOLDEN, **fixture)
    print("wrote %s: %d values, %d bytes" % (iao.GOLDEN, fixture["data"].size, os.path.getsize(iao.GOLDEN)))
