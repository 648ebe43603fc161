#!/usr/bin/env python3
"""Writes tests/golden/g10_ia3_envelope.npz: the 50-digit results of the 3-user 2x2 IA solvers (closed form, alt-min,
min-leakage, max-SINR, MMSE; every start) over the case table of tests/ia3_oracle.py, for tests/test_ia3_oracle_cpu.py and
tests/test_gpu_ia3_envelope.py.

Per case and realization (leading axis of every array), rounded to f64:
  PF [3, 2, 2] = F_k F_k^H and PU [3, 2, 2] = U_k^H U_k (Hermitian, packed into one real matrix each: herm_pack), F [3, 2, 2]
  (re, im), sinr [3, 2] (zero padded), capacity, iterations, skipped (1: no solution exists -- every result NaN),
  margins [9]: stop, tie, gap, load, mu0, feasible, phase, stop0, cond,
  kappa [4]: sensitivity / 1e-14 of capacity, sinr, PF, PU;  e_np [4]: the error of oracle/ia.py at f64 against the mp result
  (inf where it raises),
  closed form only: cand_PF, cand_PU, cand_F, cand_sinr, cand_capacity, cand_kappa of BOTH candidates and the choice.
Channels and starts are seeds (ia3_oracle.draw), not matrices.

After writing, the strict-share condition of tests/test_ia3_oracle_cpu.py is evaluated and the cases that fail it are
listed: give them another seed in ia3_oracle.RESEEDED and run again.

Pure Python at 50 digits: minutes on a few cores.  usage: python scripts/make_golden_ia3.py [jobs]
"""
import multiprocessing
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import ia3_oracle as o  # noqa: E402


def _one(name):
    return name, o.case_fields(o.CASE_BY_NAME[name])


def build_fixture(jobs):
    names = sorted(o.CASE_BY_NAME, key=lambda n: -(o.CASE_BY_NAME[n]["max_iterations"] * (4 if "mmse" in n else 1)))
    with multiprocessing.Pool(jobs) as pool:
        done = {}
        for name, fields in pool.imap_unordered(_one, names):
            done[name] = fields
            print("%3d/%d %s" % (len(done), len(names), name), flush=True)
    return {c["name"]: done[c["name"]] for c in o.CASES}


def strict_share_failures(results):
    bad = []
    for c in o.CASES:
        if c["name"] in o.NOT_STRICT_BY_CLASS:
            continue
        n = int(o.strict_realizations(c, results[c["name"]]).sum())
        if n < (3 if c["cls"] == "rayleigh" else 2):
            bad.append((c["name"], n))
    return bad


if __name__ == "__main__":
    results = build_fixture(int(sys.argv[1]) if len(sys.argv) > 1 else min(8, os.cpu_count() or 1))
    fixture = o.pack_fixture(results)
    np.savez_compressed(o.GOLDEN, **fixture)
    print("wrote %s: %d values, %d bytes" % (o.GOLDEN, fixture["data"].size, os.path.getsize(o.GOLDEN)))
    for name, n in strict_share_failures(results):
        f = results[name]
        print("NOT STRICT ENOUGH %s: %d of 3; kappa %s margins %s" % (name, n, f["kappa"].max(axis=0), f["margins"].min(axis=0)))
