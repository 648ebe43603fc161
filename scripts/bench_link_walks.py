#!/usr/bin/env python3
"""Milliseconds per call of every record-walking link kernel (csrc/link_walk.hpp) at the project's own shape for each, for the
A/B of two builds of the library: run once per build with MCLE_LIBRARY pointing at it, alternating.

    k_mimo_flat_link   2^18 realizations, NSymbs 200, 16-QAM, 15 dB; blast 4 x 4, alamouti 2 x 2, svd 4 x 4; slicer and
                       min-distance; both arithmetics (scripts/bench_mimo_schemes.py)
    k_mimo_pilot_link  4 x 4, P = 16, 2^20 realizations, slicer (scripts/bench_pilot_link.py)
    k_mimo_large_link  8 x 8, 2^20 realizations, slicer (scripts/bench_mimo_large.py)
    k_mimo_large_pilot_link  8 x 8 with P = 16 in both arithmetics and 8 x 16 with P = 64 in complex128 (dominated by the set-up
                       kernel), LS estimate from drawn pilots, 2^20 realizations, slicer (scripts/bench_large_pilot.py)
    k_comp_link        variant None, 3 cells of 2 x 2, one interferer antenna, NSymbs 500, 4-PSK (scripts/bench_comp.py)
    k_iagl_link        K = 3, 5 x 3, Ns = 2, max-SINR with max_iterations = 1 (the fewest the entry point accepts), 2^16 realizations
    k_ia_link          bench.py's c5: 262 144 realizations of 200 columns, 16-QAM, 20 dB, slicer, walk_legacy = 1
    k_bd_link          bench.py's f6: 131 072 realizations, 3 users of 2 x 2, 500 columns, 4-PSK, 15 dB, walk_legacy = 1

A call is timed by the wall clock and ends in a device synchronise; one warm-up call, then the median of REPS calls.  Prints ONE
JSON line: {"library": ..., "ms": {name: median ms per call}}.

usage: MCLE_LIBRARY=/path/to/libmcle.so python scripts/bench_link_walks.py [scale]    (scale divides the realization counts)
       python scripts/bench_link_walks.py --table profiles/r26/link_walk_ab.log          (no GPU: the A/B table of a log whose lines
                                                                                          are "parent {json}" / "result {json}")
The bar of the table: the result's median over the rounds is at most the parent's median plus the parent's own spread (max - min)."""
import json
import os
import sys
import time

import numpy as np


def table(path):
    runs = {"parent": {}, "result": {}}
    for line in open(path):
        who, _, doc = line.partition(" ")
        if who in runs and doc.startswith("{"):
            for name, v in json.loads(doc)["ms"].items():
                runs[who].setdefault(name, []).append(v)
    print("| link | parent ms (median, min - max) | result ms (median, min - max) | change | bar |\n|---|---|---|---|---|")
    failed = []
    for name, p in runs["parent"].items():
        r = sorted(runs["result"][name])
        p = sorted(p)
        pm, rm = p[len(p) // 2], r[len(r) // 2]
        ok = rm <= pm + (p[-1] - p[0])
        if not ok:
            failed.append(name)
        print("| %s | %.3f (%.3f - %.3f) | %.3f (%.3f - %.3f) | %+.2f %% | %s |" % (name, pm, p[0], p[-1], rm, r[0], r[-1],
                                                                                100.0 * (rm - pm) / pm, "pass" if ok else "FAIL"))
    print("failed:", failed)


if len(sys.argv) > 2 and sys.argv[1] == "--table":
    table(sys.argv[2])
    sys.exit(0)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pyphysim_amd import _lib  # noqa: E402
from pyphysim_amd.engine import Engine  # noqa: E402
from pyphysim_amd.modulators import constellation  # noqa: E402

REPS = 5
scale = int(sys.argv[1]) if len(sys.argv) > 1 else 1
eng = Engine(0, "f32")
ms = {}


def measure(name, call):
    call(1 << 30)
    eng.sync()
    ts = []
    for rep in range(REPS):
        t0 = time.perf_counter()
        call(rep << 24)
        eng.sync()
        ts.append(time.perf_counter() - t0)
    ms[name] = round(1e3 * sorted(ts)[REPS // 2], 4)


NV15 = 10 ** -1.5
DEMOD = (("slicer", _lib.DEMOD_QAM_SLICER), ("mindist", _lib.DEMOD_MINDIST))
eng.set_constellation(constellation("qam", 16), _lib.CONST_QAM)
n = max((1 << 18) // scale, 64)
for dtype in ("f32", "f64"):
    for scheme, nt, nr in (("blast", 4, 4), ("alamouti", 2, 2), ("svd", 4, 4)):
        for dname, method in DEMOD:
            cnt = eng.new_counters()
            measure("flat %s %dx%d %s %s" % (scheme, nr, nt, dname, dtype),
                    lambda first: eng.run_mimo_flat(scheme, nt, nr, 200, NV15, 1, first, n, method=method, dtype=dtype, counters=cnt))
n = max((1 << 20) // scale, 64)
for dtype in ("f32", "f64"):
    measure("pilot 4x4 P16 %s" % dtype,
            lambda first: eng.run_mimo_pilot_link(4, 4, 16, 200, NV15, 1, first, n, method=_lib.DEMOD_QAM_SLICER, dtype=dtype))
    measure("large 8x8 %s" % dtype,
            lambda first: eng.run_mimo_large(8, 8, 200, NV15, 1, first, n, method=_lib.DEMOD_QAM_SLICER, dtype=dtype))
    measure("large pilot 8x8 P16 %s" % dtype,
            lambda first: eng.run_mimo_large_pilot_link(8, 8, 16, 200, NV15, 1, first, n, method=_lib.DEMOD_QAM_SLICER, dtype=dtype))
measure("large pilot 8x16 P64 f64",          # the set-up kernel's share is largest here: 64 pilots through 16 receive rows
        lambda first: eng.run_mimo_large_pilot_link(8, 16, 64, 200, NV15, 1, first, n, method=_lib.DEMOD_QAM_SLICER, dtype="f64"))
n = max((1 << 16) // scale, 64)
for dtype in ("f32", "f64"):
    measure("iagl K3 5x3 Ns2 it1 %s" % dtype,
            lambda first: eng.run_ia_general(3, 5, 3, 2, 200, NV15, 1, first, n, solver="max_sinr", max_iterations=1, dtype=dtype))
with eng.options(walk_legacy=1):
    n = max(262144 // scale, 64)
    for dtype in ("f32", "f64"):
        cnt = eng.new_counters()
        measure("ia c5 %s" % dtype,
                lambda first: eng.run_ia(200, 0.01, 1, first, n, method=_lib.DEMOD_QAM_SLICER, dtype=dtype, counters=cnt))
    eng.set_constellation(constellation("psk", 4), _lib.CONST_GENERIC)
    n = max(131072 // scale, 64)
    for dtype in ("f32", "f64"):
        cnt = eng.new_counters()
        measure("bd f6 %s" % dtype,
                lambda first: eng.run_bd(3, 2, 500, 1.0, NV15, 1, first, n, method=_lib.DEMOD_MINDIST, dtype=dtype, counters=cnt))
# the application's CoMP shape (scripts/bench_comp.py)
K, R, E, PLB = 3, 2, 1, 10 ** -12.81
noise_var = 10.0 ** (-116.4 / 10.0) / 1000.0
iPu, pe = 10.0 ** 0.5 * noise_var / PLB, 10.0 ** 1.0 / 1000.0
pl, ple = PLB * (2.0 * np.ones((K, K)) + 6.0 * np.eye(K)), 1.5 * PLB * np.ones((K, E))
n = max((1 << 20) // scale, 64)
for dtype in ("f32", "f64"):
    measure("comp None 3x(2x2) %s" % dtype,
            lambda first: eng.run_comp(K, R, E, 500, iPu, noise_var, pe, 1, first, n, variant="None", packet_length=60, pathloss=pl,
                                       pathloss_ext=ple, dtype=dtype))
print(json.dumps({"library": os.path.relpath(_lib.LIB_PATH, REPO), "ms": ms}))
