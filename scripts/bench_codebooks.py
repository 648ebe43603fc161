#!/usr/bin/env python3
"""Rates of the fused Grassmannian codebook search (mcle_run_codebook_search, csrc/kernels_codebook.hip), both arithmetics:
candidates/s and pairs/s for G(2,1) K = 64, G(3,1) K = 64 and G(4,2) K = 16, complex codebooks, timed by the wall clock over
`reps` calls after one warm-up call (the result's trip to the host included; no per-candidate array is asked for).  Next to
them the CPU rate of the NumPy restatement of the same search (tests/codebook_oracle.py) measured in the same run on a few
candidates, and the rate of the chordal-distance operator on device-resident codebooks by the context's event timer.
Writes profiles/r14/codebooks.json.  Its "kernel_resources" block is the new kernels' entries of
profiles/r14/kernel_resources.json, which `python scripts/kernel_resources.py r14` writes from the built objects (run it
first, on the build host; that file lists every kernel of the library, is a by-product and is not kept in the repository).
Without it the block says so.

usage: python scripts/bench_codebooks.py [scale]      (scale divides the candidate counts; default 1)"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import codebook_oracle as co  # noqa: E402
from pyphysim_amd.engine import Engine  # noqa: E402

SHAPES = ((2, 1, 64, 1 << 21), (3, 1, 64, 1 << 21), (4, 2, 16, 1 << 22))          # Nt, Ns, K, candidates per call
SEED = 20261018
scale = int(sys.argv[1]) if len(sys.argv) > 1 else 1
reps, cpu_candidates = 5, 64
eng = Engine(0, "f64")
out = {"device": eng.device_name, "calls_timed": reps, "codebook_type": "complex", "search": [], "operator": [], "numpy_restatement": []}


def wall(fn):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


for Nt, Ns, K, count in SHAPES:
    count = max(count // scale, 64)
    pairs = K * (K - 1) // 2
    t0 = time.perf_counter()
    want = co.search(SEED, 0, cpu_candidates, K, Nt, Ns, "complex")
    cpu = (time.perf_counter() - t0) / cpu_candidates
    out["numpy_restatement"].append(dict(Nt=Nt, Ns=Ns, K=K, candidates=cpu_candidates, candidates_per_s=1.0 / cpu,
                                         pairs_per_s=pairs / cpu))
    for dtype in ("f64", "f32"):
        res = eng.run_codebook_search(K, Nt, Ns, SEED, 0, cpu_candidates, dtype=dtype)
        assert res["best_index"] == want["best_index"], (res, want["best_index"])
        dt = wall(lambda: eng.run_codebook_search(K, Nt, Ns, SEED, 0, count, dtype=dtype))
        out["search"].append(dict(Nt=Nt, Ns=Ns, K=K, dtype=dtype, candidates=count, candidates_per_s=count / dt,
                                  pairs_per_s=count * pairs / dt, ms_per_call_wall=dt * 1e3, kernel=eng.last_kernel(),
                                  speedup_over_numpy_restatement=count / dt * cpu))
        batch = max(count // 8, 64)
        C = eng.codebook_generate(K, Nt, Ns, SEED, 0, batch, dtype=dtype, device=True)
        eng.chordal_min_dist(C, dtype=dtype)
        eng.sync()
        eng.timer_start()
        for _ in range(reps):
            md2, pair = eng.empty(batch, "float64"), eng.empty((batch, 2), "int32")
            eng._raise_value(eng.lib.mcle_chordal_min_dist(eng.ctx, eng._dt(dtype), C.ptr, batch, K, Nt, Ns, md2.ptr, pair.ptr, None))
        ms = eng.timer_stop_ms() / reps
        out["operator"].append(dict(Nt=Nt, Ns=Ns, K=K, dtype=dtype, codebooks=batch, codebooks_per_s=batch / (ms * 1e-3),
                                    pairs_per_s=batch * pairs / (ms * 1e-3), ms_per_launch=ms, kernel=eng.last_kernel()))
        del C
res = os.path.join(REPO, "profiles", "r14", "kernel_resources.json")
out["kernel_resources"] = "not recorded: run scripts/kernel_resources.py r14 before this script"
if os.path.exists(res):
    out["kernel_resources"] = {k: v for k, v in json.load(open(res))["kernels"].items() if k.startswith("k_codebook")}
os.makedirs(os.path.join(REPO, "profiles", "r14"), exist_ok=True)
dst = os.environ.get("CODEBOOKS_BENCH_OUT", os.path.join(REPO, "profiles", "r14", "codebooks.json"))
json.dump(out, open(dst, "w"), indent=1)
print(json.dumps({k: v for k, v in out.items() if k != "kernel_resources"}, indent=1))
