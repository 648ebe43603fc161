#!/usr/bin/env python3
"""Rates of the fused limited-feedback IA pipeline (mcle_run_ia_quantized) at the application's shape -- K = 3, 2 x 2, NSymbs 50,
BPSK, 15 dB: realizations/s with codebooks of 16 / 512 / 4096 words, both metrics, both arithmetics, the closed-form and the
max-SINR (120 iterations) solver.  Next to each figure, from the same session: mcle_run_ia with the same solver (perfect CSI).

A call is timed by the wall clock over `reps` calls after one warm-up call; every call ends in the blocking read-back of its
counter block and of the per-realization capacity / distance arrays (as Engine.run_ia_quantized returns them).  Writes
profiles/r19/quant_ia.json; its "kernel_resources" block is the new kernels' entries of profiles/r19/kernel_resources.json
(`python scripts/kernel_resources.py r19 k_quantize` on the build host first).  The split of the three launches comes from a
separate run under `rocprofv3 --kernel-trace --stats` (usage below, `split`): profiles/r19/quant_ia_kernel_stats.csv.

usage: python scripts/bench_quant_ia.py [scale [out.json]]      (scale divides the realization count; default 1)
       rocprofv3 --kernel-trace --stats -d DIR -o quant_ia -- python scripts/bench_quant_ia.py split"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pyphysim_amd import modulators, quantization  # noqa: E402
from pyphysim_amd.engine import Engine  # noqa: E402

NS, SNR_DB, MAX_IT = 50, 15.0, 120
noise_var = 10.0 ** (-SNR_DB / 10.0)
eng = Engine(0, "f64")
modulators.BPSK(engine=eng)._bind()
books = {C: quantization.gen_codebook(C, 4, seed=19, engine=eng) for C in (16, 512, 4096)}

if len(sys.argv) > 1 and sys.argv[1] == "split":
    # one call per form under the profiler: the app's size, both arithmetics, both solvers
    for dtype in ("f32", "f64"):
        for solver in ("closed_form", "max_sinr"):
            eng.run_ia_quantized(NS, noise_var, 1, 0, 1 << 18, books[512], dtype=dtype, solver=solver, max_iterations=MAX_IT)
    eng.close()
    sys.exit(0)

scale = int(sys.argv[1]) if len(sys.argv) > 1 else 1
count = max((1 << 20) // scale, 64)
out = {"device": eng.device_name, "realizations_per_call": count,
       "shape": dict(K=3, Nr=2, Nt=2, NSymbs=NS, modulator="BPSK", SNR_dB=SNR_DB, max_iterations=MAX_IT),
       "run_ia_quantized": [], "run_ia": []}


def wall(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


for dtype in ("f32", "f64"):
    for solver, reps in (("closed_form", 10), ("max_sinr", 3)):
        dt = wall(lambda: eng.run_ia(NS, noise_var, 1, 0, count, dtype=dtype, solver=solver, max_iterations=MAX_IT), reps)
        base = count / dt
        out["run_ia"].append(dict(solver=solver, dtype=dtype, calls_timed=reps, realizations_per_s=base, ms_per_call_wall=dt * 1e3))
        for C in (16, 512, 4096):
            d_cb = eng.to_device(books[C], np.complex64 if dtype == "f32" else np.complex128)
            for metric in ("euclidean", "chordal"):
                dt = wall(lambda: eng.run_ia_quantized(NS, noise_var, 1, 0, count, d_cb, metric=metric, dtype=dtype, solver=solver,
                                                       max_iterations=MAX_IT), reps)
                out["run_ia_quantized"].append(dict(solver=solver, dtype=dtype, codebook_size=C, metric=metric, calls_timed=reps,
                                                    realizations_per_s=count / dt, ms_per_call_wall=dt * 1e3,
                                                    run_ia_realizations_per_s=base))

res_path = os.path.join(REPO, "profiles", "r19", "kernel_resources.json")
if os.path.exists(res_path):
    kr = json.load(open(res_path))["kernels"]
    out["kernel_resources"] = {k: v for k, v in kr.items() if k.startswith("k_quantize")}
else:
    out["kernel_resources"] = "not recorded: run scripts/kernel_resources.py r19 k_quantize on the build host first"
dest = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "r19", "quant_ia.json")
os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
json.dump(out, open(dest, "w"), indent=1)
for row in out["run_ia"] + out["run_ia_quantized"]:
    print(row)
eng.close()
