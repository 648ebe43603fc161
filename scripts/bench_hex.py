#!/usr/bin/env python3
"""First measurement of the hexagonal-cell system-level kernels (csrc/pipeline_hex.hip) on one MI355X: drops/s of
Engine.run_hex_drops at 3 x 1, 7 x 10 and 19 x 13 users (cells x users per cell: one, two and four users per lane), both
arithmetics, with and without wrap around where the cluster has it (19 cells), five timed calls after a warm-up; and the time
of CompSimulator's batch with user_positioning_method='Random' against the same batch with a fixed path-loss matrix, the two
alternating in one process, as a ratio.

Where the time goes: the kernel alone is timed between two GPU events (outputs allocated once, nothing read back) in three
forms -- users drawn and only the per-drop outputs written; the same users injected (no placement: the difference is the
Philox draws and the rejection loop); users drawn and the records written too (the difference is the records' stores, K + n_ext
doubles per user at a stride of one row per lane).  The registers of the kernels stand next to the result in
kernel_resources.json (scripts/kernel_resources.py).

Each GPU step runs in a child process under its own time limit.  Writes profiles/r29/hex.json (or argv[2]).

usage: python scripts/bench_hex.py [scale [out.json]]      (scale divides the drop counts; default 1)"""
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = [(3, 1, 1 << 16), (7, 10, 1 << 16), (19, 13, 1 << 14)]           # (cells, users per cell, drops per call)
REPS = 5
CFG = dict(cell_radius=1.0, tx_power=0.2, noise_power=3.0e-14, ext_power=2.0e-9, hist_bins=60, hist_lo_dB=-10.0, hist_step_dB=1.0)
STEP_LIMIT_S = 240


def wall(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def kernel_ms(eng, dtype, cfg, count, KU, cols, d_pos=None, records=False, pos_out=None):
    """GPU time of ONE launch between two events on the context's stream (mean of REPS after a warm-up)."""
    from pyphysim_amd import _lib
    hist, flags = eng.zeros(cfg.hist_bins + 2, np.uint64), eng.empty(count, np.int32)
    per_drop = [eng.empty(count, np.float64) for _ in range(2)]
    rec = eng.empty((count, KU, cols), np.float64) if records else None
    args = (eng.ctx, _lib.dtype_code(dtype), _lib.byref(cfg), 1, 0, count, d_pos.ptr if d_pos is not None else None, flags.ptr,
            rec.ptr if records else None, pos_out.ptr if pos_out is not None else None, None, None, hist.ptr, per_drop[0].ptr,
            per_drop[1].ptr)
    total = 0.0
    for i in range(REPS + 1):
        eng.timer_start()
        rc = eng.lib.mcle_run_hex_drops(*args)
        ms = eng.timer_stop_ms()
        assert rc == 0, eng.lib.mcle_last_error()
        total += ms if i else 0.0
    return total / REPS


def step_drops(K, U, dtype, wrap, count):
    from pyphysim_amd.engine import Engine
    eng = Engine(0, dtype)
    kw = dict(num_cells=K, users_per_cell=U, wrap_around=wrap, n_ext=1, **CFG)
    dt = wall(lambda: eng.run_hex_drops(seed=1, first=0, count=count, dtype=dtype, **kw), REPS)
    cfg = eng._hex_cfg(**kw)
    pos = eng.empty((count, K * U, 2), np.float64)
    kernel_ms(eng, dtype, cfg, count, K * U, K + 1, pos_out=pos)          # (not a measurement: fills `pos` for the injected form)
    ms_drawn = kernel_ms(eng, dtype, cfg, count, K * U, K + 1)
    ms_injected = kernel_ms(eng, dtype, cfg, count, K * U, K + 1, d_pos=pos)
    ms_records = kernel_ms(eng, dtype, cfg, count, K * U, K + 1, records=True)
    row = dict(cells=K, users_per_cell=U, users=K * U, dtype=dtype, wrap_around=bool(wrap), drops_per_call=count,
               calls_timed=REPS, drops_per_s=count / dt, users_per_s=count * K * U / dt, ms_per_call_wall=dt * 1e3,
               kernel=eng.last_kernel(),
               kernel_events=dict(ms_drawn=ms_drawn, ms_injected=ms_injected, ms_drawn_with_records=ms_records,
                                  drops_per_s_drawn=count / (ms_drawn * 1e-3), share_placement=1.0 - ms_injected / ms_drawn,
                                  records_over_drawn=ms_records / ms_drawn))
    eng.close()
    return row


def step_comp(batch):
    """One batch of CompSimulator (K = 3, 2 x 2, 500 symbols, all six variants) with 'Random' users against a fixed matrix:
    A B A B ... in one process, the ratio of the medians."""
    from pyphysim_amd.engine import Engine
    from pyphysim_amd.simulators import CompSimulator
    eng = Engine(0, "f64")
    kw = dict(SNR=[10.0], Pe_dBm=[-60.0], K=3, Nr=2, ext_int_rank=1, NSymbs=500, rep_max=batch, batch_size=batch, engine=eng)
    rand = CompSimulator(user_positioning_method="Random", **kw)
    pl, ple = CompSimulator.far_away_pathloss(1.0, 1)
    fixed = CompSimulator(pathloss=pl, pathloss_ext=ple, **kw)
    params = rand.params.get_unpacked_params_list()[0]
    times = {"random": [], "fixed": []}
    for i in range(REPS + 1):
        for name, sim in (("random", rand), ("fixed", fixed)):
            t0 = time.perf_counter()
            sim._run_batch(params, 0, batch)
            eng.sync()
            if i:
                times[name].append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    for _ in range(REPS):
        rand.drop_records(eng, params, 0, batch)
    eng.sync()
    drops_s = (time.perf_counter() - t0) / REPS
    med = {k: float(np.median(v)) for k, v in times.items()}
    eng.close()
    return dict(batch=batch, variants=6, n_symbols=500, ms_random=med["random"] * 1e3, ms_fixed=med["fixed"] * 1e3,
                ratio_random_over_fixed=med["random"] / med["fixed"], ms_drop_call_alone=drops_s * 1e3, alternations=REPS)


def child(spec):
    """one step in a fresh process under its own time limit -> its JSON result (or the failure, and nothing more is started)"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", json.dumps(spec)], capture_output=True, text=True,
                       timeout=STEP_LIMIT_S)
    if r.returncode != 0:
        raise SystemExit("step %s failed (%d): %s" % (spec, r.returncode, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        spec = json.loads(sys.argv[2])
        res = (step_comp(spec["batch"]) if spec["step"] == "comp"
               else step_drops(spec["K"], spec["U"], spec["dtype"], spec["wrap"], spec["count"]))
        print(json.dumps(res))
        sys.exit(0)
    scale = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    out = {"config": dict(CFG, model="general 3.76 / 128.1 (PathLoss3GPP1, km)", n_ext=1, min_dist_ratio=0.0), "drops": []}
    for K, U, count in SHAPES:
        for dtype in ("f32", "f64"):
            for wrap in ((False, True) if K == 19 else (False,)):
                out["drops"].append(child(dict(step="drops", K=K, U=U, dtype=dtype, wrap=wrap, count=max(count // scale, 64))))
                print(out["drops"][-1])
    out["comp_simulator_batch"] = child(dict(step="comp", batch=max(4096 // scale, 64)))
    print(out["comp_simulator_batch"])
    dest = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "r29", "hex.json")
    os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
    json.dump(out, open(dest, "w"), indent=1)
    print("wrote", dest)
