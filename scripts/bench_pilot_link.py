#!/usr/bin/env python3
"""Realizations/s of the flat Blast link with pilot-estimated CSI (Engine.run_mimo_pilot_link: both filters on one walk) next to
the perfect-CSI pipeline it extends (Engine.run_mimo_flat('blast')): 4 x 4, 16-QAM, NSymbs = 200 symbols per layer, SNR 15 dB,
slicer demodulation, LS estimator with P = 4, 16, 64 drawn pilots, both arithmetics.  2^20 realizations per call, every call
ended by a device synchronise, one warm-up call of each, then five repetitions alternating the two in the same process; the
figure to look at is the ratio of the two times.  Writes profiles/r23/pilot_link.json and prints it."""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pyphysim_amd import _lib  # noqa: E402
from pyphysim_amd.engine import Engine  # noqa: E402
from pyphysim_amd.modulators import constellation  # noqa: E402

N, NT, NR, NSYMBS, NOISE_VAR, REPS = 1 << 20, 4, 4, 200, 10 ** -1.5, 5


def timed(eng, call):
    eng.sync()
    t0 = time.perf_counter()
    res = call()
    eng.sync()
    return time.perf_counter() - t0, res


def main():
    eng = Engine(0, "f32")
    eng.set_constellation(constellation("qam", 16), _lib.CONST_QAM)
    out = {"_shape": "%dx%d 16-QAM NSymbs %d noise_var %.6g slicer, %d realizations per call, median of %d alternating repetitions"
                     % (NR, NT, NSYMBS, NOISE_VAR, N, REPS)}
    for dtype in ("f32", "f64"):
        for P in (4, 16, 64):
            pilot = lambda first: eng.run_mimo_pilot_link(NT, NR, P, NSYMBS, NOISE_VAR, 1, first, N, method=_lib.DEMOD_QAM_SLICER,
                                                          dtype=dtype)
            flat = lambda first: eng.run_mimo_flat("blast", NT, NR, NSYMBS, NOISE_VAR, 1, first, N, method=_lib.DEMOD_QAM_SLICER,
                                                   dtype=dtype)
            timed(eng, lambda: pilot(1 << 30))
            timed(eng, lambda: flat(1 << 30))
            tp, tf = [], []
            for rep in range(REPS):
                s, (c_est, c_perf) = timed(eng, lambda: pilot(rep * N))
                tp.append(s)
                s, c_flat = timed(eng, lambda: flat(rep * N))
                tf.append(s)
            tp.sort()
            tf.sort()
            units = float(c_est["n_realizations"] * NSYMBS * NT)
            out["%s_P%d" % (dtype, P)] = dict(
                pilot_link_realizations_per_s=N / tp[REPS // 2], mimo_flat_realizations_per_s=N / tf[REPS // 2],
                time_ratio=tp[REPS // 2] / tf[REPS // 2], pilot_link_ms=[round(1e3 * t, 3) for t in tp],
                mimo_flat_ms=[round(1e3 * t, 3) for t in tf], ser_estimated_csi=c_est["sym_errors"] / units,
                ser_perfect_csi=c_perf["sym_errors"] / units, ser_mimo_flat=c_flat["sym_errors"] / units, kernel=eng.last_kernel())
    dst = os.path.join(REPO, "profiles", "r23")
    os.makedirs(dst, exist_ok=True)
    with open(os.path.join(dst, "pilot_link.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
