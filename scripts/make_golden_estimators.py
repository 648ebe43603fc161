#!/usr/bin/env python3
"""Writes tests/golden/g3_estimators.npz: the reference's own LS / MMSE block-pilot estimator outputs and closed-form MSEs
for the cases of tests/test_estimators_cpu.py and tests/test_gpu_estimators.py.

Drives the reference (darcamo/pyphysim v0.7.2, channel_estimation/estimators.py) the way scripts/make_golden_chanest.py
does -- the stub modules of oracle/ref_shim on sys.path, PYPHYSIM_REFERENCE naming its checkout -- and holds none of it.
Inputs come from a seeded RandomState; the received arrays are drawn on a grid of 1 / 64 so that the compressed file stays
below the largest fixture of tests/golden/ (the expected outputs are the reference's full-precision numbers).  Arrays only.

usage: PYPHYSIM_REFERENCE=/path/to/pyphysim python scripts/make_golden_estimators.py
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("PYPHYSIM_REFERENCE", "/root/reference")
OUT = os.path.join(REPO, "tests", "golden", "g3_estimators.npz")

# LS cases: name -> (nr, nt, P, batch, pilots per realization); batch = 0: a 2-D Y
LS_CASES = {
    "nr3_2d": (3, 1, 10, 0, False),
    "nr5_shared": (5, 2, 10, 2, False),
    "nr5_per": (5, 2, 10, 2, True),
    "nr17_b37": (17, 3, 7, 37, False),            # odd P, batch not a multiple of 16
    "nr67_per": (67, 3, 33, 5, True),
    "p_eq_nt": (4, 8, 8, 3, False),               # P = nt: a square, worse-conditioned s
    "nr128": (128, 1, 130, 2, False),             # nr at the limit, P beyond one wavefront
}
# MMSE cases: name -> (nr, P, batch, pilots per realization, rho); C[i][k] = 0.49 rho^|i-k| e^{0.3j (i-k)}
MMSE_CASES = {
    "nr3_2d": (3, 100, 0, False, 0.0),            # the reference's own test
    "nr3_b2": (3, 100, 2, False, 0.0),
    "nr3_per": (3, 100, 2, True, 0.0),
    "nr16_b37": (16, 7, 37, False, 0.9),
    "nr67": (67, 33, 5, False, 0.7),
    "nr128": (128, 12, 18, False, 0.9),
}
# closed-form MSEs: (Nr, noise_power, alpha, pilot_power, num_pilots, rho)
THEORY_CASES = [(3, 0.5, 0.7, 1.5, 10, 0.0), (16, 0.5, 0.7, 1.5, 8, 0.9), (64, 0.1, 1.0, 1.0, 10, 0.7), (3, 0.01, 0.7, 1.0, 100, 0.0)]


def covariance(nr, rho, scale=0.49):
    d = np.arange(nr)[:, None] - np.arange(nr)[None, :]
    return scale * (float(rho) ** np.abs(d) if rho else (d == 0).astype(float)) * np.exp(0.3j * d)


def build_fixture():
    sys.path.insert(0, os.path.join(REPO, "oracle", "ref_shim"))
    sys.path.insert(0, REF)
    np.int = int
    from pyphysim.channel_estimation.estimators import (compute_ls_estimation, compute_mmse_estimation,
                                                        compute_theoretical_ls_MSE, compute_theoretical_mmse_MSE)

    rng = np.random.RandomState(20261018)
    out = {}

    def grid(*shape):
        return (np.round(64 * rng.randn(*shape)) + 1j * np.round(64 * rng.randn(*shape))) / 64.0

    def pilots(*shape):
        return np.sqrt(1.5) * np.exp(2j * np.pi * rng.rand(*shape))

    for name, (nr, nt, P, batch, per) in LS_CASES.items():
        Y = grid(*((batch, nr, P) if batch else (nr, P)))
        s = pilots(*((batch, nt, P) if per else (nt, P)))
        out["ls_%s_Y" % name], out["ls_%s_s" % name] = Y, s
        out["ls_%s_out" % name] = compute_ls_estimation(Y, s)
    for name, (nr, P, batch, per, rho) in MMSE_CASES.items():
        Y = grid(*((batch, nr, P) if batch else (nr, P)))
        s = pilots(*((batch, 1, P) if per else (1, P)))
        C = covariance(nr, rho)
        out["mmse_%s_Y" % name], out["mmse_%s_s" % name], out["mmse_%s_C" % name] = Y, s, C
        out["mmse_%s_noise_power" % name] = np.float64(0.5)
        out["mmse_%s_out" % name] = compute_mmse_estimation(Y, s, 0.5, C)
    out["theory_args"] = np.array(THEORY_CASES, dtype=np.float64)
    out["theory_ls"] = np.array([compute_theoretical_ls_MSE(int(nr), npw, a, pp, int(P))
                                 for nr, npw, a, pp, P, rho in THEORY_CASES])
    out["theory_mmse"] = np.array([compute_theoretical_mmse_MSE(int(nr), npw, a, pp, int(P), covariance(int(nr), rho, 1.0))
                                   for nr, npw, a, pp, P, rho in THEORY_CASES])
    return out


if __name__ == "__main__":
    fixture = build_fixture()
    np.savez_compressed(OUT, **fixture)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(fixture), os.path.getsize(OUT)))
