#!/usr/bin/env python3
"""Rates of the estimation-error pipeline with interference cancellation at the common shape (Ne = 150, size_multiplier 2,
15 taps kept, 4 receive antennas, 3 users with gains 1, 0.2, 0.03), both arithmetics: realizations/s of mcle_run_chanest_ic
in modes 0 / 1 / 2 next to mcle_run_chanest in the same session, and each mode's ratio to the plain pipeline.  Wall clock
around `reps` calls after one warm-up call, the read-back of the [count, users] arrays included (as scripts/bench_chanest.py
times run_chanest); the rounds alternate over the four variants so that clock drift hits them alike.
Writes profiles/r11/chanest_ic.json (CHANEST_IC_BENCH_OUT names another place).

usage: python scripts/bench_chanest_ic.py [realizations]"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pyphysim_amd import reference_signals as rs  # noqa: E402
from pyphysim_amd.engine import Engine  # noqa: E402

NE, M, K, NR, SHIFTS, GAINS = 150, 2, 15, 4, (0, 3, 6), (1.0, 0.2, 0.03)
reals = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 16
reps = 5
root = rs.RootSequence(root_index=25, size=NE)
seqs = np.stack([rs.SrsUeSequence(root, s).seq_array() for s in SHIFTS])
power, delay = list(10.0 ** (np.array([0.0, -3.0, -6.0, -9.0]) / 10.0)), [0, 1, 2, 4]
eng = Engine(0, "f64")
out = {"shape": dict(Ne=NE, size_multiplier=M, num_taps_to_keep=K, n_rx=NR, n_users=len(SHIFTS), link_gain=list(GAINS),
                     realizations=reals, calls_timed=reps), "device": eng.device_name}
args = (seqs, NR, K, M, 0.1, power, delay, 1, 0, reals)
for dtype in ("f64", "f32"):
    variants = {"run_chanest": lambda: eng.run_chanest(*args, dtype=dtype)}
    for mode in (0, 1, 2):
        variants["run_chanest_ic_mode%d" % mode] = (lambda mode=mode: eng.run_chanest_ic(*args, mode, direct_user=0,
                                                                                         link_gain=GAINS, dtype=dtype))
    spent, tags = {k: 0.0 for k in variants}, {}
    for k, call in variants.items():
        call()
        tags[k] = eng.last_kernel()
    for _ in range(reps):
        for k, call in variants.items():
            t0 = time.perf_counter()
            call()
            spent[k] += time.perf_counter() - t0
    for k in variants:
        dt = spent[k] / reps
        out["%s_%s" % (k, dtype)] = dict(realizations_per_s=reals / dt, ms_per_call_wall=dt * 1e3, kernel=tags[k],
                                         time_relative_to_run_chanest=spent[k] / spent["run_chanest"])
dst = os.environ.get("CHANEST_IC_BENCH_OUT", os.path.join(REPO, "profiles", "r11", "chanest_ic.json"))
os.makedirs(os.path.dirname(dst), exist_ok=True)
json.dump(out, open(dst, "w"), indent=1)
print(json.dumps(out, indent=1))
