"""The large-array Blast link with pilot-estimated next to perfect channel state (csrc/pipeline_mimo_large_pilot.hip:
mcle_run_mimo_large_pilot): the cases shared by test_large_pilot_cpu.py (CPU: the conditions on the inputs) and
test_gpu_large_pilot.py (GPU: the kernels).  TEST INFRASTRUCTURE.

Every case is the size-generic NumPy restatement tests/pilot_link_oracle.py (make_case / realization) with 16-QAM over
realizations FIRST .. FIRST + COUNT - 1 = 3 .. 72 of pilot_link_oracle.SEED, computed once and shared read-only.  The GPU tests run
these inputs and no larger ones.

Edges: P = 1 = nt; odd P (a half-used last PILOT block); P = 255; nt not a multiple of 4 (padded symbol pairs); nr not a multiple of
4; column counts 33, 34, 51, 130 (around the 32-column pass; an odd count makes NOISE pairs straddle blocks); 70 realizations = more
than one 16-realization chunk per wavefront and not a multiple of the set-up kernel's 4."""
import functools

import numpy as np

import estimators_oracle as eo
import pilot_link_oracle as po

FIRST, COUNT, SEED = po.FIRST, po.COUNT, po.SEED

_C16, _C7 = eo.toeplitz_cov(16, 0.9), eo.toeplitz_cov(7, 0.9)
# name: (nt, nr, P, n_symbols, SNR dB, pilot power, MMSE filter, pilots)
CASES = {
    "1x16-p1": po.make_case(1, 16, 1, 130, -4.0, 1.0, False, "random"),
    "4x16-p4-dft": po.make_case(4, 16, 4, 33, 4.0, 1.0, True, "dft"),
    "5x6-p5-dft": po.make_case(5, 6, 5, 51, 20.0, 1.0, False, "dft"),
    "7x9-p12": po.make_case(7, 9, 12, 34, 18.0, 2.0, False, "random"),
    "8x8-p16": po.make_case(8, 8, 16, 130, 14.0, 1.0, True, "random"),
    "8x8-p8-dft-zf": po.make_case(8, 8, 8, 51, 30.0, 1.0, False, "dft"),
    "8x16-p9": po.make_case(8, 16, 9, 130, 8.0, 1.0, False, "random"),
    "6x16-p255": po.make_case(6, 16, 255, 51, 6.0, 1.0, True, "random"),
    "mmse-est-1x16": po.make_case(1, 16, 5, 51, 0.0, 1.0, False, "random", estimator="mmse", L=np.linalg.cholesky(_C16),
                                  cov=0.49 * _C16, alpha=0.7),
    "ls-L-5x7": po.make_case(5, 7, 9, 51, 16.0, 1.0, False, "random", L=np.linalg.cholesky(_C7), alpha=0.7),
}
NAMES = sorted(CASES)
PLAIN = [n for n in NAMES if CASES[n]["L"] is None]       # L = I, alpha = 1: block 1 is the large link / the Blast chain


@functools.lru_cache(maxsize=None)
def reference(name):
    """pilot_link_oracle.run of a named case (se / be [2, COUNT], err, pow, gap, route, gram_cond, n_symbols, n_bits) plus what the
    CPU conditions need per realization: H, Hest [COUNT, nr, nt], est [COUNT, 2, nt n_symbols], idx [COUNT, nt n_symbols]."""
    cfg = CASES[name]
    outs = [po.realization(cfg, r) for r in range(FIRST, FIRST + COUNT)]
    res = dict(se=np.stack([o["se"] for o in outs], axis=1), be=np.stack([o["be"] for o in outs], axis=1),
               err=np.array([o["err"] for o in outs]), pow=np.array([o["pow"] for o in outs]),
               gap=np.array([o["gap"] for o in outs]), gram_cond=np.array([o["gram_cond"] for o in outs]),
               route=np.array([float(np.max(np.abs(o["est_lstsq"] - o["est"][0]))) for o in outs]),
               H=np.stack([o["H"] for o in outs]), Hest=np.stack([o["Hest"] for o in outs]),
               est=np.stack([o["est"] for o in outs]), idx=np.stack([o["idx"] for o in outs]),
               n_symbols=cfg["nt"] * cfg["n_symbols"], n_bits=cfg["nt"] * cfg["n_symbols"] * 4)
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res
