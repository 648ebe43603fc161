#!/usr/bin/env python3
"""Rates of the channel-estimation kernels at the common shape (Ne = 150, size_multiplier 2, 15 taps kept, 4 receive
antennas, 3 users), both arithmetics: rows/s of mcle_cazac_estimate on device-resident rows, realizations/s of
mcle_run_chanest, and next to them the NumPy restatement's rate on this host's CPU.  Kernel time comes from the
context's event timer around `reps` back-to-back launches after one warm-up launch.
Writes profiles/r09/chanest.json.  Its "kernel_resources" block is the two kernels' entries of
profiles/r09/kernel_resources.json, which `python scripts/kernel_resources.py r09` writes from the built objects (run it
first, on the build host; that file is a by-product and is not kept in the repository).  Without it the block says so.

usage: python scripts/bench_chanest.py [rows] [realizations]"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import chanest_oracle as co  # noqa: E402
from pyphysim_amd import reference_signals as rs  # noqa: E402
from pyphysim_amd.engine import Engine  # noqa: E402

NE, M, K, NR, SHIFTS = 150, 2, 15, 4, (0, 3, 6)
rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 18
reals = int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 16
reps = 5
root = rs.RootSequence(root_index=25, size=NE)
seqs = np.stack([rs.SrsUeSequence(root, s).seq_array() for s in SHIFTS])
power, delay = list(10.0 ** (np.array([0.0, -3.0, -6.0, -9.0]) / 10.0)), [0, 1, 2, 4]
eng = Engine(0, "f64")
rng = np.random.RandomState(1)
out = {"shape": dict(Ne=NE, size_multiplier=M, num_taps_to_keep=K, n_rx=NR, n_users=len(SHIFTS), rows=rows, realizations=reals,
                     launches_timed=reps), "device": eng.device_name}
for dtype, cplx in (("f64", np.complex128), ("f32", np.complex64)):
    rx = eng.to_device((rng.randn(rows, NE) + 1j * rng.randn(rows, NE)).astype(cplx))
    ref = eng.to_device(seqs[0].astype(cplx))
    eng.cazac_estimate(ref, rx, K, size_multiplier=M, dtype=dtype)
    eng.sync()
    eng.timer_start()
    for _ in range(reps):
        eng.cazac_estimate(ref, rx, K, size_multiplier=M, dtype=dtype)
    ms = eng.timer_stop_ms() / reps
    out["cazac_estimate_" + dtype] = dict(rows_per_s=rows / (ms * 1e-3), ms_per_launch=ms, kernel=eng.last_kernel())
    del rx
    eng.run_chanest(seqs, NR, K, M, 0.1, power, delay, 1, 0, reals, dtype=dtype)
    t0 = time.perf_counter()
    for _ in range(reps):
        eng.run_chanest(seqs, NR, K, M, 0.1, power, delay, 1, 0, reals, dtype=dtype)
    dt = (time.perf_counter() - t0) / reps          # wall clock: includes the read-back of the two [count, users] arrays
    out["run_chanest_" + dtype] = dict(realizations_per_s=reals / dt, ms_per_launch_wall=dt * 1e3, kernel=eng.last_kernel())
cfg = dict(ref_seqs=seqs, n_rx=NR, size_multiplier=M, num_taps_to_keep=K, noise_var=0.1, tap_power=power, tap_delay=delay)
t0 = time.perf_counter()
for r in range(200):
    co.chanest_realization(1, r, cfg)
dt = time.perf_counter() - t0
y = rng.randn(4000, NE) + 1j * rng.randn(4000, NE)
t1 = time.perf_counter()
co.estimate(seqs[0], y, K, M)
out["numpy_restatement_cpu"] = dict(realizations_per_s=200 / dt, rows_per_s=4000 / (time.perf_counter() - t1))
res = os.path.join(REPO, "profiles", "r09", "kernel_resources.json")
out["kernel_resources"] = "not recorded: run scripts/kernel_resources.py r09 before this script"
if os.path.exists(res):
    out["kernel_resources"] = {k: v for k, v in json.load(open(res))["kernels"].items() if "cazac" in k or "chanest" in k}
os.makedirs(os.path.join(REPO, "profiles", "r09"), exist_ok=True)
dst = os.environ.get("CHANEST_BENCH_OUT", os.path.join(REPO, "profiles", "r09", "chanest.json"))
json.dump(out, open(dst, "w"), indent=1)
print(json.dumps({k: v for k, v in out.items() if k != "kernel_resources"}, indent=1))
