#!/usr/bin/env python3
"""First measurement of the indoor system-level kernels (csrc/pipeline_indoor.hip) at the application's shape -- 12 x 12 rooms
of 10 m, 100 users, METIS PS7, best-channel association, the unused APs off: drops/s of Engine.run_indoor_drops at 2^16 drops
per call with ap_decimation 1 (144 APs) and 4 (36 APs), both arithmetics, five timed calls after a warm-up; the heat-map
operator in points/s on the application's 32 400 points; and the NumPy restatement (tests/metis_oracle.py) on the same host.

Next to every drops/s stands a ceiling from the pair count and the issue cost of a transcendental instruction (8 cycles per
wave instruction of one wave's stream on a SIMD, MI355X: 256 CUs x 4 SIMDs at 2.4 GHz): pass 1 issues one log2 per (user
slot, AP), pass 2 one log2 and one exp2 per (user slot, transmitting AP); a lane holds ceil(U / 64) rounded up to 1, 2 or 4
slots.  f64 has no transcendental instruction (the device libm's polynomials), so the ceiling is stated for f32 only.
Where the time goes: the kernel alone is timed between two GPU events (no allocation, no read-back) on drawn users, on
injected users spread over the floor, and on injected users that all sit in ONE room, so that one AP transmits and pass 2
shrinks to 1 / A of its work -- what remains is pass 1 and the per-drop epilogue (and all 100 users' LDS atomics on one address).
The registers of the kernels stand next to the result in kernel_resources.json (scripts/kernel_resources.py).

Each GPU step runs in a child process under its own time limit.  Writes profiles/<next unused rNN>/metis.json (or argv[2]).

usage: python scripts/bench_metis.py [scale [out.json]]      (scale divides the drop count; default 1)"""
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

N, L, U, REPS = 12, 10.0, 100, 5
TX, NOISE = 0.1, 2.0e-14
CLOCK_HZ, SIMDS, TRANS_CYCLES = 2.4e9, 256 * 4, 8
STEP_LIMIT_S = 240


def wall(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def kernel_ms(eng, dtype, kw, count, d_pos=None):
    """GPU time of ONE launch between two events on the context's stream (mean of REPS after a warm-up): the outputs are
    allocated once and nothing is read back, so what is timed is the launch and the kernel, not the call's fixed host cost."""
    from pyphysim_amd import _lib
    cfg = eng._indoor_cfg(model="metis_ps7", assoc="best_channel", active=1, wall_loss_dB=5.0, pl_n=3.76, pl_C=128.1,
                          dist_scale=1e-3, fc_MHz=900.0, **{k: v for k, v in kw.items() if k != "dtype"})
    hist, load = eng.zeros(2, np.uint64), eng.zeros(U + 1, np.uint64)
    per_drop = [eng.empty(count, np.float64) for _ in range(3)] + [eng.empty(count, np.int32)]
    args = (eng.ctx, _lib.dtype_code(dtype), _lib.byref(cfg), 1, 0, count, d_pos.ptr if d_pos is not None else None, hist.ptr,
            load.ptr, per_drop[0].ptr, per_drop[1].ptr, per_drop[2].ptr, per_drop[3].ptr, None, None, None)
    total = 0.0
    for i in range(REPS + 1):
        eng.timer_start()
        rc = eng.lib.mcle_run_indoor_drops(*args)
        ms = eng.timer_stop_ms()
        assert rc == 0, eng.lib.mcle_last_error()
        total += ms if i else 0.0
    return total / REPS


def step_drops(dec, dtype, count):
    from pyphysim_amd.engine import Engine
    eng = Engine(0, dtype)
    kw = dict(rooms_per_side=N, side_length=L, ap_decimation=dec, n_users=U, tx_power=TX, noise_power=NOISE, dtype=dtype)
    out = {}
    dt = wall(lambda: out.update(eng.run_indoor_drops(seed=1, first=0, count=count, **kw)), REPS)
    A = {1: 144, 4: 36}[dec]
    active = float(out["active_aps"].mean())
    slots = 2                                                   # 100 users: two per lane
    ms_kernel = kernel_ms(eng, dtype, kw, count)
    row = dict(ap_decimation=dec, dtype=dtype, drops_per_call=count, calls_timed=REPS, drops_per_s=count / dt,
               ms_per_call_wall=dt * 1e3, ms_kernel_events=ms_kernel, kernel_drops_per_s=count / (ms_kernel * 1e-3),
               kernel=eng.last_kernel(), mean_active_aps=active, pairs_per_drop=dict(pass1=A * U, pass2=active * U))
    if dtype == "f32":
        cycles = (A * slots + 2 * active * slots) * TRANS_CYCLES
        row["ceiling_drops_per_s"] = SIMDS * CLOCK_HZ / cycles
        row["kernel_share_of_ceiling"] = row["kernel_drops_per_s"] / row["ceiling_drops_per_s"]
    # every user of a drop in ONE room: one AP transmits, pass 2 walks one AP.  Same drop count, device-resident positions, GPU
    # events.  The probe also skips the Philox draw (injected positions) and sends all 100 users' LDS atomics to one counter
    # and one mask bit, which the drawn users spread over many: it is an estimate of "everything but pass 2", biased both ways.
    rs = np.random.RandomState(7)
    pos = np.empty((count, U, 2))
    pos[..., 0] = -55.0 + 10.0 * (rs.rand(count, U) - 0.5) * 0.9 + (10.0 if dec == 4 else 0.0)
    pos[..., 1] = 55.0 + 10.0 * (rs.rand(count, U) - 0.5) * 0.9 - (10.0 if dec == 4 else 0.0)
    d_pos = eng.to_device(pos)
    ms_one = kernel_ms(eng, dtype, kw, count, d_pos)
    spread = np.empty((count, U, 2))                            # injected positions spread over the floor: the draw's cost
    spread[...] = N * L * (rs.rand(count, U, 2) - 0.5)
    ms_spread = kernel_ms(eng, dtype, kw, count, eng.to_device(spread))
    row["one_room_probe"] = dict(drops=count, ms_one_ap_events=ms_one, ms_injected_spread_events=ms_spread,
                                 ms_drawn_users_events=ms_kernel, share_outside_pass2=ms_one / ms_spread)
    eng.close()
    return row


def step_heatmap(dtype):
    import metis_oracle as mo
    from pyphysim_amd.engine import Engine
    eng = Engine(0, dtype)
    pts = mo.heat_points(L, N)
    rows = []
    for model in mo.HEAT_MODELS:
        cfg = mo.base_cfg(N, 1, L, tx=TX, noise=NOISE, assoc=0, **model)
        kw = mo.engine_kwargs(cfg)
        dt = wall(lambda: eng.indoor_sinr(pts, dtype=dtype, **kw), REPS)
        rows.append(dict(dtype=dtype, model=cfg["model"], pl_n=cfg["pl_n"], points=int(pts.size), points_per_s=pts.size / dt,
                         ms_per_call_wall=dt * 1e3, kernel=eng.last_kernel()))
    eng.close()
    return rows


def step_numpy():
    import metis_oracle as mo
    cfg = mo.base_cfg(N, 1, L, tx=TX, noise=NOISE, assoc=1, active=1)
    pos = mo.philox_positions(1, 0, 20, U, N, L)
    t0 = time.perf_counter()
    for p in pos:
        mo.drop(cfg, p)
    per_drop = (time.perf_counter() - t0) / len(pos)
    pts = mo.heat_points(L, N)
    heat = mo.base_cfg(N, 1, L, tx=TX, noise=NOISE, assoc=0)
    t0 = time.perf_counter()
    mo.heat_map(heat, pts)
    t_heat = time.perf_counter() - t0
    return dict(drops_per_s=1.0 / per_drop, ms_per_drop=per_drop * 1e3, heat_map_points_per_s=pts.size / t_heat,
                heat_map_s=t_heat)


def child(spec):
    """one step in a fresh process under its own time limit -> its JSON result (or the failure, and nothing more is started)"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", json.dumps(spec)], capture_output=True, text=True,
                       timeout=STEP_LIMIT_S)
    if r.returncode != 0:
        raise SystemExit("step %s failed (%d): %s" % (spec, r.returncode, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def next_round():
    """profiles/rNN of the first round that holds no measurement yet (a kernel_resources.json alone does not count)"""
    taken = [int(os.path.basename(p)[1:]) for p in glob.glob(os.path.join(REPO, "profiles", "r[0-9][0-9]"))
             if set(os.listdir(p)) - {"kernel_resources.json"}]
    return "r%02d" % (max(taken + [0]) + 1)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        spec = json.loads(sys.argv[2])
        res = {"drops": lambda: step_drops(spec["dec"], spec["dtype"], spec["count"]),
               "heat": lambda: step_heatmap(spec["dtype"]), "numpy": step_numpy}[spec["step"]]()
        print(json.dumps(res))
        sys.exit(0)
    scale = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    count = max((1 << 16) // scale, 64)
    out = {"shape": dict(rooms_per_side=N, side_length=L, users=U, model="metis_ps7", assoc="best_channel", active=1),
           "ceiling": dict(clock_hz=CLOCK_HZ, simds=SIMDS, cycles_per_transcendental_wave_instruction=TRANS_CYCLES),
           "drops": [], "heat_map": []}
    for dec in (1, 4):
        for dtype in ("f32", "f64"):
            out["drops"].append(child(dict(step="drops", dec=dec, dtype=dtype, count=count)))
            print(out["drops"][-1])
    for dtype in ("f32", "f64"):
        out["heat_map"] += child(dict(step="heat", dtype=dtype))
    out["numpy_restatement_same_host"] = child(dict(step="numpy"))
    print(out["heat_map"], out["numpy_restatement_same_host"])
    dest = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", next_round(), "metis.json")
    os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
    json.dump(out, open(dest, "w"), indent=1)
    print("wrote", dest)
