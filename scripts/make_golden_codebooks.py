#!/usr/bin/env python3
"""Writes tests/golden/g4_codebooks.npz: nine of the reference's stored codebook-search results with the reference's own
pair distances on them, and the reference's subspace metrics and projections on a handful of drawn inputs, for
tests/test_codebooks_cpu.py and tests/test_gpu_codebooks.py.

Drives the reference (darcamo/pyphysim v0.7.2: subspace/metrics.py, subspace/projections.py; the stored results of
apps/codebooks/codebook_results/) with the stub modules of oracle/ref_shim on sys.path and PYPHYSIM_REFERENCE naming its
checkout, and holds none of it.  Arrays only.

usage: PYPHYSIM_REFERENCE=/path/to/pyphysim python scripts/make_golden_codebooks.py
"""
import itertools
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "g4_codebooks.npz")

# (Nt, Ns, K) of the stored results copied
STORED = [(2, 1, 8), (2, 1, 128), (3, 1, 3), (3, 1, 16), (3, 2, 16), (3, 2, 64), (4, 1, 8), (4, 1, 32), (4, 2, 16)]
# drawn pairs: name -> (Nt, Ns, real-valued)
DRAWN = {"c3x1": (3, 1, False), "c4x2": (4, 2, False), "c5x3": (5, 3, False), "c8x4": (8, 4, False), "r4x2": (4, 2, True)}


def build_fixture(ref):
    sys.path.insert(0, os.path.join(REPO, "oracle", "ref_shim"))
    sys.path.insert(0, ref)
    np.int = int
    from pyphysim.subspace.metrics import (calc_chordal_distance, calc_chordal_distance_2,
                                           calc_chordal_distance_from_principal_angles, calc_principal_angles)
    from pyphysim.subspace.projections import Projection

    out = {"stored_shapes": np.array(STORED, dtype=np.int32)}
    for Nt, Ns, K in STORED:
        src = np.load(os.path.join(ref, "apps", "codebooks", "codebook_results",
                                   "codebook_%d_precoders_in_G(%d,%d).npz" % (K, Nt, Ns)))
        key = "g%d_%d_k%d" % (Nt, Ns, K)
        C = np.asarray(src["best_codebook"])
        assert C.shape == (K, Nt, Ns), (key, C.shape)
        out[key + "_codebook"] = C
        out[key + "_best_dist"] = np.float64(src["best_dist"])
        out[key + "_best_principal_angles"] = np.asarray(src["best_principal_angles"], dtype=np.float64)
        d, d2 = [], []
        for a, b in itertools.combinations(range(K), 2):
            pa = calc_principal_angles(C[a], C[b])
            d.append(calc_chordal_distance_from_principal_angles(pa))
            d2.append(float(np.sum(np.sin(pa) ** 2)))
        out[key + "_pair_dist"] = np.array(d)                 # the reference's distances, itertools.combinations order
        out[key + "_pair_d2"] = np.array(d2)                  # sum sin^2 of the reference's principal angles

    rng = np.random.RandomState(20261018)
    for name, (Nt, Ns, real) in DRAWN.items():
        def draw(*shape):
            return rng.randn(*shape) if real else rng.randn(*shape) + 1j * rng.randn(*shape)
        A, B = draw(Nt, Ns), draw(Nt, Ns)
        v, M = draw(Nt), draw(Nt, 3)
        pa = calc_principal_angles(A, B)
        P = Projection(A)
        key = "drawn_" + name
        out.update({key + "_A": A, key + "_B": B, key + "_v": v, key + "_M": M, key + "_angles": pa,
                    key + "_dist_from_angles": np.float64(calc_chordal_distance_from_principal_angles(pa)),
                    key + "_dist": np.float64(calc_chordal_distance(A, B)),
                    key + "_dist2": np.float64(calc_chordal_distance_2(A, B)),
                    key + "_Q": P.Q, key + "_oQ": P.oQ,
                    key + "_calcQ": Projection.calcProjectionMatrix(A),
                    key + "_calcoQ": Projection.calcOrthogonalProjectionMatrix(A),
                    key + "_project_v": P.project(v), key + "_oproject_v": P.oProject(v), key + "_reflect_v": P.reflect(v),
                    key + "_project_M": P.project(M), key + "_oproject_M": P.oProject(M), key + "_reflect_M": P.reflect(M)})
    out["drawn_names"] = np.array(sorted(DRAWN))
    return out


if __name__ == "__main__":
    ref = os.environ.get("PYPHYSIM_REFERENCE")
    if not ref:
        sys.exit("set PYPHYSIM_REFERENCE to the reference's checkout")
    fixture = build_fixture(ref)
    np.savez_compressed(OUT, **fixture)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(fixture), os.path.getsize(OUT)))
