#!/usr/bin/env python3
"""First rates of the fused general-geometry IA link (mcle_run_ia_general), complex64 and complex128, 16-QAM at 15 dB, NSymbs 200:
    K = 3, 5 x 3, Ns = 2, max-SINR, 60 iterations (apps/ia/IA_Results_NrxNt(Ns).py)
    K = 3, 3 x 3, Ns = 3, max-SINR under the greedy stream selection, 60 iterations (apps/ia/simulate_greedy_ia.py)
Next to each, from the same session: mcle_ia_solve_general alone on the same number of DEVICE-RESIDENT channels and starts (the
pipeline's own, copied out of a first call), outputs left on the device.  The difference is what the link adds to the solve --
draw, record, walk and the read-back of the per-realization arrays -- and the only figure that says whether the walk matters.

A call is timed by the wall clock over `reps` calls after one warm-up call.  The pipeline's calls end in the blocking read-back
of the counters and the per-realization capacity / iteration / stream-count arrays (as Engine.run_ia_general returns them); the
solver's calls end in mcle_ctx_sync.  Writes profiles/r21/ia_general_link.json; its "kernel_resources" block is the walk kernels'
entries of profiles/r21/kernel_resources.json (`python scripts/kernel_resources.py r21 k_iagl` on the build host first).

usage: python scripts/bench_ia_general_link.py [scale [out.json]]      (scale divides the realization count; default 1)"""
import json
import os
import sys
import time
from ctypes import byref

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pyphysim_amd import _lib, modulators  # noqa: E402
from pyphysim_amd.engine import Engine  # noqa: E402

NS, SNR_DB, MAX_IT = 200, 15.0, 60
noise_var = 10.0 ** (-SNR_DB / 10.0)
CASES = [dict(name="K3 5x3 Ns2 max_sinr", K=3, nr=5, nt=3, Ns=2, select=None),
         dict(name="K3 3x3 Ns3 max_sinr greedy", K=3, nr=3, nt=3, Ns=3, select="greedy")]

eng = Engine(0, "f64")
modulators.QAM(16, engine=eng)._bind()
scale = int(sys.argv[1]) if len(sys.argv) > 1 else 1
count = max((1 << 16) // scale, 64)
out = {"device": eng.device_name, "realizations_per_call": count,
       "shape": dict(NSymbs=NS, modulator="16-QAM", SNR_dB=SNR_DB, max_iterations=MAX_IT, relative_factor=1e-6), "rows": []}


def wall(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


for c in CASES:
    K, nr, nt = c["K"], c["nr"], c["nt"]
    D = 4 if max(nr, nt) <= 4 else 6
    link = lambda dtype: eng.run_ia_general(K, nr, nt, c["Ns"], NS, noise_var, 1, 0, count, solver="max_sinr", select=c["select"],
                                            max_iterations=MAX_IT, dtype=dtype)
    # the solver alone, on the pipeline's own channels and starts, everything device-resident
    _, a = eng.run_ia_general(K, nr, nt, c["Ns"], 2, noise_var, 1, 0, count, solver="max_sinr", select=c["select"],
                              max_iterations=MAX_IT, per_realization=True, outputs=("big_H", "F_init"))
    pad = np.zeros((count, 4, D, D), dtype=np.complex128)
    pad[:, :K] = a["F_init"]
    d_H, d_F0 = eng.to_device(a["big_H"]), eng.to_device(pad)
    F, U = eng.empty((count, 4, D, D), np.complex128), eng.empty((count, 4, D, D), np.complex128)
    sinr, cap = eng.empty((count, 4, D), np.float64), eng.empty(count, np.float64)
    its, ns, sk = eng.empty(count, np.uint32), eng.empty((count, 4), np.int32), eng.empty(count, np.uint32)
    cfg = _lib.IaGeneralCfg()
    cfg.K, cfg.nr, cfg.nt = K, nr, nt
    for k in range(4):
        cfg.ns[k] = c["Ns"] if k < K else 0
    cfg.solver, cfg.initialize_with, cfg.max_iterations = _lib.IA_SOLVERS["max_sinr"], 0, MAX_IT
    cfg.stream_selection = _lib.IA_STREAM_SELECTION[c["select"]]
    cfg.noise_var, cfg.relative_factor = noise_var, 1e-6

    def solve():
        _lib.check(eng.lib.mcle_ia_solve_general(eng.ctx, byref(cfg), d_H.ptr, d_F0.ptr, F.ptr, U.ptr, sinr.ptr, cap.ptr, its.ptr,
                                                 ns.ptr, sk.ptr, None, count))
        eng.sync()

    t_solve = wall(solve, 3)
    for dtype in ("f32", "f64"):
        t_link = wall(lambda: link(dtype), 3)
        kernel = eng.last_kernel()
        out["rows"].append(dict(case=c["name"], dtype=dtype, kernel=kernel, calls_timed=3, link_realizations_per_s=count / t_link,
                                link_ms_per_call_wall=t_link * 1e3, solve_alone_realizations_per_s=count / t_solve,
                                solve_alone_ms_per_call_wall=t_solve * 1e3, link_minus_solve_ms=(t_link - t_solve) * 1e3,
                                mean_iterations=float(a["iterations"].mean()), mean_streams_kept=float(a["ns"].sum(axis=1).mean())))

res_path = os.path.join(REPO, "profiles", "r21", "kernel_resources.json")
if os.path.exists(res_path):
    kr = json.load(open(res_path))["kernels"]
    out["kernel_resources"] = {k: v for k, v in kr.items() if k.startswith("k_iagl")}
else:
    out["kernel_resources"] = "not recorded: run scripts/kernel_resources.py r21 k_iagl on the build host first"
dest = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "r21", "ia_general_link.json")
os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
json.dump(out, open(dest, "w"), indent=1)
for row in out["rows"]:
    print(row)
eng.close()
