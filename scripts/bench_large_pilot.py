#!/usr/bin/env python3
"""First measurements of the large-array pilot link (Engine.run_mimo_large_pilot_link: the walk of run_mimo_large through the
filter of the pilot estimate and that of the channel at once) next to ONE call of Engine.run_mimo_large on the same shape, which
this link leaves untouched and which is therefore the yardstick: 16-QAM, NSymbs = 200 symbols per transmit antenna, SNR 15 dB, LS
estimate from drawn pilots, slicer demodulation, zero forcing; shapes Nt x Nr = 4 x 16, 8 x 8, 8 x 16; P = 8, 16, 64 pilots; both
arithmetics.  2^20 realizations per call, every call ended by a device synchronise, one warm-up call of each, then five repetitions
alternating the two in the same process.  The figure of interest is ratio = median time of the pilot link / median time of
run_mimo_large: two separate launches of the large link would cost 2.0 plus the set-up.  No acceptance threshold.
Writes profiles/r27/large_pilot.json (or the path given as the first argument) and prints it."""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pyphysim_amd import _lib  # noqa: E402
from pyphysim_amd.engine import Engine  # noqa: E402
from pyphysim_amd.modulators import constellation  # noqa: E402

N, NSYMBS, SNR_DB, REPS = 1 << 20, 200, 15.0, 5
NOISE_VAR = 10.0 ** (-SNR_DB / 10.0)
SHAPES = ((4, 16), (8, 8), (8, 16))                  # (nt, nr)
PILOTS = (8, 16, 64)


def timed(eng, call):
    eng.sync()
    t0 = time.perf_counter()
    res = call()
    eng.sync()
    return time.perf_counter() - t0, res


def main():
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "r27", "large_pilot.json")
    eng = Engine(0, "f32")
    eng.set_constellation(constellation("qam", 16), _lib.CONST_QAM)
    out = {"_shape": "16-QAM NSymbs %d noise_var %.6g (15 dB) LS estimate from P drawn pilots of power 1, slicer, zero forcing, %d "
                     "realizations per call, median of %d repetitions alternating with run_mimo_large on the same shape in the "
                     "same process; ratio = pilot link / run_mimo_large" % (NSYMBS, NOISE_VAR, N, REPS)}
    for dtype in ("f32", "f64"):
        for nt, nr in SHAPES:
            large = lambda first: eng.run_mimo_large(nt, nr, NSYMBS, NOISE_VAR, 1, first, N, method=_lib.DEMOD_QAM_SLICER,
                                                     dtype=dtype)
            timed(eng, lambda: large(1 << 30))
            for P in PILOTS:
                pilot = lambda first: eng.run_mimo_large_pilot_link(nt, nr, P, NSYMBS, NOISE_VAR, 1, first, N,
                                                                    method=_lib.DEMOD_QAM_SLICER, dtype=dtype)
                timed(eng, lambda: pilot(1 << 30))
                kernel = eng.last_kernel()
                tp, tl = [], []
                for rep in range(REPS):
                    s, (c_est, c_perf) = timed(eng, lambda: pilot(rep * N))
                    tp.append(s)
                    s, c_large = timed(eng, lambda: large(rep * N))
                    tl.append(s)
                same = all(c_perf[k] == c_large[k] for k in ("n_realizations", "n_skipped", "sym_errors", "bit_errors"))
                tp.sort()
                tl.sort()
                mp, ml = tp[REPS // 2], tl[REPS // 2]
                nsym = float(c_est["n_realizations"] * NSYMBS * nt)
                out["%s_%dx%d_p%d" % (dtype, nt, nr, P)] = dict(
                    ratio=mp / ml, pilot_realizations_per_s=N / mp, pilot_ns_per_realization=1e9 * mp / N,
                    large_realizations_per_s=N / ml, large_ns_per_realization=1e9 * ml / N,
                    pilot_ms=[round(1e3 * t, 3) for t in tp], large_ms=[round(1e3 * t, 3) for t in tl],
                    ser_estimated_csi=c_est["sym_errors"] / nsym, ser_perfect_csi=c_perf["sym_errors"] / nsym,
                    perfect_block_equals_run_mimo_large=bool(same), n_skipped=c_est["n_skipped"], kernel=kernel)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
