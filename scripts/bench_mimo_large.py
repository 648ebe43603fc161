#!/usr/bin/env python3
"""First measurements of the large-array Blast link (Engine.run_mimo_large: est = A x + G n on the matrix cores) next to the 4 x 4
flat kernel (Engine.run_mimo_flat('blast', 4, 4)): 16-QAM, NSymbs = 200 symbols per transmit antenna, SNR 15 dB, slicer
demodulation, zero forcing, shapes Nt x Nr = 4 x 4, 8 x 8, 4 x 16, 8 x 16, both arithmetics.  2^20 realizations per call, every call
ended by a device synchronise, one warm-up call of each, then five repetitions alternating the two in the same process.  Quoted
as realizations/s, time per realization and time per complex multiply-accumulate of Nt (Nt + Nr) NSymbs.  The NumPy oracle's rate
on this host's CPU for 8 x 8 (oracle.chains.chain_mimo_scheme, one process) goes in the same file.  No acceptance threshold.
Writes profiles/r24/mimo_large.json (or the path given as the first argument) and prints it."""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import chains  # noqa: E402
from pyphysim_amd import _lib  # noqa: E402
from pyphysim_amd.engine import Engine  # noqa: E402
from pyphysim_amd.modulators import constellation  # noqa: E402

N, NSYMBS, SNR_DB, REPS = 1 << 20, 200, 15.0, 5
NOISE_VAR = 10.0 ** (-SNR_DB / 10.0)
SHAPES = ((4, 4), (8, 8), (4, 16), (8, 16))          # (nt, nr)


def timed(eng, call):
    eng.sync()
    t0 = time.perf_counter()
    res = call()
    eng.sync()
    return time.perf_counter() - t0, res


def main():
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "r24", "mimo_large.json")
    eng = Engine(0, "f32")
    eng.set_constellation(constellation("qam", 16), _lib.CONST_QAM)
    out = {"_shape": "16-QAM NSymbs %d noise_var %.6g (15 dB) slicer zero forcing, %d realizations per call, median of %d "
                     "repetitions alternating with run_mimo_flat('blast', 4, 4) in the same process; macs = Nt (Nt + Nr) NSymbs "
                     "complex multiply-accumulates per realization" % (NSYMBS, NOISE_VAR, N, REPS)}
    flat_macs = 4 * (4 + 4) * NSYMBS
    for dtype in ("f32", "f64"):
        flat = lambda first: eng.run_mimo_flat("blast", 4, 4, NSYMBS, NOISE_VAR, 1, first, N, method=_lib.DEMOD_QAM_SLICER,
                                               dtype=dtype)
        timed(eng, lambda: flat(1 << 30))
        for nt, nr in SHAPES:
            large = lambda first: eng.run_mimo_large(nt, nr, NSYMBS, NOISE_VAR, 1, first, N, method=_lib.DEMOD_QAM_SLICER,
                                                     dtype=dtype)
            timed(eng, lambda: large(1 << 30))
            kernel = eng.last_kernel()
            tl, tf = [], []
            for rep in range(REPS):
                s, c_large = timed(eng, lambda: large(rep * N))
                tl.append(s)
                s, c_flat = timed(eng, lambda: flat(rep * N))
                tf.append(s)
            tl.sort()
            tf.sort()
            ml, mf = tl[REPS // 2], tf[REPS // 2]
            macs = nt * (nt + nr) * NSYMBS
            out["%s_%dx%d" % (dtype, nt, nr)] = dict(
                large_realizations_per_s=N / ml, large_ns_per_realization=1e9 * ml / N, large_ps_per_mac=1e12 * ml / N / macs,
                flat4x4_realizations_per_s=N / mf, flat4x4_ns_per_realization=1e9 * mf / N,
                flat4x4_ps_per_mac=1e12 * mf / N / flat_macs, macs_per_realization=macs,
                large_ms=[round(1e3 * t, 3) for t in tl], flat4x4_ms=[round(1e3 * t, 3) for t in tf],
                ser_large=c_large["sym_errors"] / float(c_large["n_realizations"] * NSYMBS * nt),
                ser_flat4x4=c_flat["sym_errors"] / float(c_flat["n_realizations"] * NSYMBS * 4),
                n_skipped=c_large["n_skipped"], kernel=kernel)
    eng.close()
    n_cpu = 200
    t0 = time.perf_counter()
    for r in range(n_cpu):
        chains.chain_mimo_scheme(chains.PhiloxRng(1, r), scheme="blast", mod="qam", M=16, nt=8, nr=8, NSymbs=NSYMBS, snr_db=SNR_DB)
    dt = time.perf_counter() - t0
    out["numpy_oracle_8x8"] = dict(realizations=n_cpu, realizations_per_s=n_cpu / dt, note="one process on this host's CPU")
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
