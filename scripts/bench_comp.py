#!/usr/bin/env python3
"""Rates of the fused CoMP pipeline with an external interferer (mcle_run_comp) at the application's shape -- K = 3 cells,
2 x 2 antennas, one interferer antenna, NSymbs = 500, 4-PSK, SNR 5 dB at the cell border, Pe 10 dBm: realizations/s of every
variant in complex64 and complex128.  Next to them, from the same session: mcle_run_bd(waterfilling = 0) at the same K, r,
NSymbs (the nearest existing kernel) and the NumPy oracle of tests/comp_oracle.py on the CPU (solve + link, variant None and
'effec_throughput').

A call is timed by the wall clock over `reps` calls after one warm-up call; every call ends in the blocking read-back of
its counter block (the per-realization arrays are not requested).  Writes profiles/r18/comp.json; its "kernel_resources"
block is the new kernels' entries of profiles/r18/kernel_resources.json (`python scripts/kernel_resources.py r18 k_comp_`
on the build host first).

usage: python scripts/bench_comp.py [scale [out.json]]      (scale divides the realization count; default 1)"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from pyphysim_amd import modulators  # noqa: E402
from pyphysim_amd.engine import Engine  # noqa: E402

K, R, E, NS, PACKET = 3, 2, 1, 500, 60
PLB = 10 ** -12.81
VARIANTS = ("None", "naive", "fixed", "capacity", "effec_throughput", "Whitening")
scale = int(sys.argv[1]) if len(sys.argv) > 1 else 1
count = max((1 << 20) // scale, 64)
reps = 10
noise_var = 10.0 ** (-116.4 / 10.0) / 1000.0
iPu, pe = 10.0 ** 0.5 * noise_var / PLB, 10.0 ** 1.0 / 1000.0
pl, ple = PLB * (2.0 * np.ones((K, K)) + 6.0 * np.eye(K)), 1.5 * PLB * np.ones((K, E))

eng = Engine(0, "f64")
modulators.PSK(4, engine=eng)._bind()
out = {"device": eng.device_name, "calls_timed": reps, "realizations_per_call": count,
       "shape": dict(K=K, r=R, n_ext=E, NSymbs=NS, modulator="PSK-4", SNR_dB=5.0, Pe_dBm=10.0), "run_comp": [], "run_bd": []}


def wall(fn):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


for dtype in ("f32", "f64"):
    for v in VARIANTS:
        dt = wall(lambda: eng.run_comp(K, R, E, NS, iPu, noise_var, pe, 1, 0, count, variant=v, packet_length=PACKET,
                                       pathloss=pl, pathloss_ext=ple, dtype=dtype))
        out["run_comp"].append(dict(variant=v, dtype=dtype, realizations_per_s=count / dt, ms_per_call_wall=dt * 1e3,
                                    kernel=eng.last_kernel()))
    dt = wall(lambda: eng.run_bd(K, R, NS, iPu, noise_var, 1, 0, count, pathloss=pl, waterfilling=False, dtype=dtype))
    out["run_bd"].append(dict(dtype=dtype, realizations_per_s=count / dt, ms_per_call_wall=dt * 1e3))

# the NumPy oracle on the CPU (one core): solve + link per realization
import comp_oracle as co  # noqa: E402
table = co.table_for("psk", 4)
out["cpu_oracle"] = []
for v in ("None", "effec_throughput"):
    n = 200
    t0 = time.perf_counter()
    for i in range(n):
        H = co.draw_big_H(1, i, K, R, E, pl, ple)
        MsPk, W, Ns = co.solve(H, K, R, iPu, noise_var, pe, v, 1, "psk", 4, PACKET)
        data, ext, noise = co.draw_link_inputs(1, i, K, R, E, Ns, NS, 4, noise_var, pe)
        co.link(H, MsPk, W, data, ext, noise, table)
    out["cpu_oracle"].append(dict(variant=v, realizations=n, realizations_per_s=n / (time.perf_counter() - t0)))

res_path = os.path.join(REPO, "profiles", "r18", "kernel_resources.json")
if os.path.exists(res_path):
    kr = json.load(open(res_path))["kernels"]
    out["kernel_resources"] = {k: v for k, v in kr.items() if ", 2" in k}
else:
    out["kernel_resources"] = "not recorded: run scripts/kernel_resources.py r18 k_comp_ on the build host first"
dest = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "r18", "comp.json")
os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
json.dump(out, open(dest, "w"), indent=1)
for row in out["run_comp"] + out["run_bd"] + out["cpu_oracle"]:
    print(row)
