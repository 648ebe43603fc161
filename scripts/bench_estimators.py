#!/usr/bin/env python3
"""Rates of the LS / MMSE block-pilot estimator kernels, both arithmetics: realizations/s and noise samples/s of
mcle_run_pilot_mse at (Nr, P) = (3, 10), (64, 16), (128, 16) with Nt = 1, LS only and LS + MMSE (coloured channel); GB/s
(Y read + estimates written) of mcle_ls_estimate and mcle_mmse_estimate on device-resident arrays at the same shapes; and,
from the same session, mcle_run_chanest's noise samples/s at its common shape as the nearest existing kernel.
The pipelines are timed by the wall clock over `reps` calls after one warm-up call (the read-back of the per-realization
arrays included, as scripts/bench_chanest.py does); the operators by the context's event timer around `reps` launches.
Writes profiles/r13/estimators.json.  Its "kernel_resources" block is the new kernels' entries of
profiles/r13/kernel_resources.json, which `python scripts/kernel_resources.py r13` writes from the built objects (run it
first, on the build host; that file is a by-product and is not kept in the repository).  Without it the block says so.

usage: python scripts/bench_estimators.py [scale]      (scale divides the realization counts; default 1)"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pyphysim_amd import reference_signals as rs  # noqa: E402
from pyphysim_amd.engine import Engine  # noqa: E402

SHAPES = ((3, 10, 1 << 20), (64, 16, 1 << 16), (128, 16, 1 << 15))          # Nr, P, realizations per call
scale = int(sys.argv[1]) if len(sys.argv) > 1 else 1
reps = 5
eng = Engine(0, "f64")
rng = np.random.RandomState(1)
out = {"device": eng.device_name, "calls_timed": reps, "pilot_mse": [], "operators": []}


def covariance(nr, rho=0.9):
    d = np.arange(nr)[:, None] - np.arange(nr)[None, :]
    return rho ** np.abs(d) * np.exp(0.3j * d)


def wall(fn):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


for nr, P, count in SHAPES:
    count = max(count // scale, 16)
    C = covariance(nr)
    L = np.linalg.cholesky(C)
    for dtype, cplx in (("f64", np.complex128), ("f32", np.complex64)):
        for mode, kw in (("ls", {}), ("ls+mmse", dict(chan_factor=L, cov=0.49 * C))):
            dt = wall(lambda: eng.run_pilot_mse(nr, 1, P, 0.5, 1, 0, count, pilot_power=1.5, alpha=0.7, dtype=dtype, **kw))
            out["pilot_mse"].append(dict(Nr=nr, P=P, dtype=dtype, estimators=mode, realizations=count,
                                         realizations_per_s=count / dt, noise_samples_per_s=count * nr * P / dt,
                                         ms_per_call_wall=dt * 1e3, kernel=eng.last_kernel()))
        batch = max(count // 4, 16)
        Y = eng.to_device((rng.randn(batch, nr, P) + 1j * rng.randn(batch, nr, P)).astype(cplx))
        s = eng.to_device((np.sqrt(1.5) * np.exp(2j * np.pi * rng.rand(1, P))).astype(cplx))
        nbytes = (batch * nr * P + batch * nr) * np.dtype(cplx).itemsize
        for name, fn in (("ls_estimate", lambda: eng.ls_estimate(Y, s, dtype=dtype)),
                         ("mmse_estimate", lambda: eng.mmse_estimate(Y, s, 0.5, 0.49 * C, dtype=dtype))):
            fn()
            eng.sync()
            eng.timer_start()
            for _ in range(reps):
                fn()
            ms = eng.timer_stop_ms() / reps
            out["operators"].append(dict(op=name, Nr=nr, P=P, dtype=dtype, batch=batch, GB_per_s=nbytes / (ms * 1e-3) / 1e9,
                                         ms_per_launch=ms, kernel=eng.last_kernel()))
        del Y

# the nearest existing kernel, same session: mcle_run_chanest at its common shape
NE, M, K, NR, SHIFTS = 150, 2, 15, 4, (0, 3, 6)
root = rs.RootSequence(root_index=25, size=NE)
seqs = np.stack([rs.SrsUeSequence(root, sh).seq_array() for sh in SHIFTS])
power, delay = list(10.0 ** (np.array([0.0, -3.0, -6.0, -9.0]) / 10.0)), [0, 1, 2, 4]
reals = max((1 << 16) // scale, 16)
out["run_chanest"] = []
for dtype in ("f64", "f32"):
    dt = wall(lambda: eng.run_chanest(seqs, NR, K, M, 0.1, power, delay, 1, 0, reals, dtype=dtype))
    out["run_chanest"].append(dict(dtype=dtype, Ne=NE, n_rx=NR, realizations=reals, realizations_per_s=reals / dt,
                                   noise_samples_per_s=reals * NR * NE / dt, ms_per_call_wall=dt * 1e3,
                                   kernel=eng.last_kernel()))
res = os.path.join(REPO, "profiles", "r13", "kernel_resources.json")
out["kernel_resources"] = "not recorded: run scripts/kernel_resources.py r13 before this script"
if os.path.exists(res):
    out["kernel_resources"] = {k: v for k, v in json.load(open(res))["kernels"].items()
                               if k.startswith(("k_ls_estimate", "k_mmse_estimate", "k_pilot_mse"))}
os.makedirs(os.path.join(REPO, "profiles", "r13"), exist_ok=True)
dst = os.environ.get("ESTIMATORS_BENCH_OUT", os.path.join(REPO, "profiles", "r13", "estimators.json"))
json.dump(out, open(dst, "w"), indent=1)
print(json.dumps({k: v for k, v in out.items() if k != "kernel_resources"}, indent=1))
