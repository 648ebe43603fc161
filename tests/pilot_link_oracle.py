"""NumPy restatement of the flat Blast link with pilot-estimated and with perfect channel state (mcle_run_mimo_pilot_link).
TEST INFRASTRUCTURE.

Written from the model and the draw ledger of include/mcle.h / DESIGN section 4; shares no code with the product.  Per realization
r of `seed` (mcle-philox-v1, oracle/philox.py):

    W[r][a]              CN sample r nt + a of stream 2;  H = alpha L W
    pilot phase (a, p)   uniform a P + p of stream 3;  s = sqrt(pilot_power) e^{2 pi j u}      (random pilots only)
    pilot noise (r, p)   CN sample 2 ceil(P / 2) r + p of stream 4;  Y_p = H s + sqrt(noise_var) N_p
    data symbol          n = t nt + a of stream 0;  X = reshape(sym, (nt, -1), 'F') / sqrt(nt)
    data noise (r, t)    CN sample r n_symbols + t of stream 1;  Y = H X + sqrt(noise_var) N

    LS:    H^ = Y_p s^H (s s^H)^-1
    MMSE:  h^ = B (Y_p s^H) P / |s|^2,  B = (noise_var I + P C)^-1 C                            (nt = 1)

and est = G Y with the Blast filter G of H^ (block 0, estimated CSI) and of H (block 1, perfect CSI).
"""
import functools

import numpy as np

from oracle import mimo as omimo
from oracle import modem as omodem
from oracle import philox

import estimators_oracle as eo
import helpers

STREAM_PILOT = 4
SEED = 20261020
FIRST, COUNT = helpers.FLAT_FIRST, helpers.FLAT_COUNT
M = 16


def dft_pilots(nt, P, power):
    """The first nt rows of the P-point DFT matrix times sqrt(power), as PilotEstimationSimulator fills a fixed block"""
    return np.sqrt(power) * np.exp(-2j * np.pi * np.outer(np.arange(nt), np.arange(P)) / P)


def make_case(nt, nr, P, n_symbols, snr_db, pilot_power=1.0, mmse=False, pilots="random", estimator="ls", L=None, cov=None,
              alpha=1.0, seed=SEED, noise_var=None):
    return dict(nt=nt, nr=nr, P=P, n_symbols=n_symbols, snr_db=snr_db, pilot_power=float(pilot_power), mmse=bool(mmse),
                pilots=None if pilots == "random" else dft_pilots(nt, P, pilot_power), estimator=estimator, L=L, cov=cov,
                alpha=float(alpha), seed=seed,
                noise_var=1.0 / float(omodem.dB2Linear(snr_db)) if noise_var is None else float(noise_var))


# (nt, nr, P, n_symbols, SNR dB, pilot_power, mmse, pilots): the smallest shape; P = nt; odd P (a half-used last PILOT block); the
# largest P in reach of an odd count; one, two and many columns per lane; 70 realizations = more than one 64-realization chunk
PARITY_CASES = {
    "1x1-p1": make_case(1, 1, 1, 6, 16.0, 1.0, False, "random"),
    "1x4-p3": make_case(1, 4, 3, 51, 16.0, 1.5, True, "random"),
    "2x2-p2-dft": make_case(2, 2, 2, 130, 16.0, 1.0, False, "dft"),
    "2x3-p5": make_case(2, 3, 5, 51, 16.0, 2.0, True, "random"),
    "3x3-p3-dft": make_case(3, 3, 3, 2, 16.0, 1.0, False, "dft"),
    "3x4-p7": make_case(3, 4, 7, 51, 10.0, 1.0, True, "random"),
    "4x4-p4-dft": make_case(4, 4, 4, 130, 16.0, 1.0, True, "dft"),
    "4x4-p9": make_case(4, 4, 9, 51, 16.0, 4.0, False, "random"),
    "4x4-p16": make_case(4, 4, 16, 130, 10.0, 1.0, True, "random"),
    "2x4-p255": make_case(2, 4, 255, 51, 16.0, 1.0, True, "random"),
}
_C4, _C3 = eo.toeplitz_cov(4, 0.9), eo.toeplitz_cov(3, 0.9)
EXTRA_CASES = {
    "mmse-est-1x4": make_case(1, 4, 5, 51, 16.0, 1.0, False, "random", estimator="mmse", L=np.linalg.cholesky(_C4),
                              cov=0.49 * _C4, alpha=0.7),
    "ls-L-2x3": make_case(2, 3, 5, 51, 16.0, 1.0, False, "random", L=np.linalg.cholesky(_C3), alpha=0.7),
}
ALL_CASES = dict(PARITY_CASES, **EXTRA_CASES)


def table():
    return omodem.qam_constellation(M)


def _gap(tab, est):
    """distance to the second-nearest constellation point minus the distance to the nearest, smallest over `est`"""
    d = np.sort(np.abs(est.reshape(-1, 1) - tab.reshape(1, -1)), axis=1)
    return float(np.min(d[:, 1] - d[:, 0]))


def realization(cfg, r, seed=None):
    """One realization: dict of H, Hest, Hest_lstsq (the estimate by numpy.linalg.lstsq on s^T), the estimates est [2, nt n]
    (row 0 estimated CSI, row 1 perfect), est_lstsq (row 0 by the second route), se / be [2], err, pow, gap."""
    seed = cfg["seed"] if seed is None else seed
    nt, nr, P, ns, nv = cfg["nt"], cfg["nr"], cfg["P"], cfg["n_symbols"], cfg["noise_var"]
    tab = table()
    W = philox.cnormal(seed, r, nr * nt, philox.STREAM_CHAN).reshape(nr, nt)
    L = np.eye(nr) if cfg["L"] is None else np.asarray(cfg["L"], dtype=np.complex128)
    H = cfg["alpha"] * (L @ W)
    if cfg["pilots"] is None:
        u = philox.uniforms(seed, r, nt * P, stream=philox.STREAM_PHASE).reshape(nt, P)
        s = np.sqrt(cfg["pilot_power"]) * np.exp(2j * np.pi * u)
    else:
        s = np.asarray(cfg["pilots"], dtype=np.complex128).reshape(nt, P)
    half = (P + 1) // 2
    Yp = H @ s
    if nv != 0:
        Yp = Yp + np.sqrt(nv) * philox.cnormal(seed, r, 2 * half * nr, STREAM_PILOT).reshape(nr, 2 * half)[:, :P]
    sh = s.conj().T
    ls = (Yp @ sh) @ np.linalg.inv(s @ sh)
    ls2 = np.linalg.lstsq(s.T, Yp.T, rcond=None)[0].T
    if cfg["estimator"] == "mmse":
        B = np.linalg.solve(nv * np.eye(nr) + P * np.asarray(cfg["cov"], dtype=np.complex128), cfg["cov"])
        Hest = B @ (Yp @ sh) * (P / np.real(s @ sh))
        Hest2 = P * (B @ ls2)
    else:
        Hest, Hest2 = ls, ls2
    idx = philox.symbols(seed, r, ns * nt, M)
    X = omimo.blast_encode(omodem.modulate(tab, idx), nt)
    Y = H @ X
    if nv != 0:
        Y = Y + np.sqrt(nv) * philox.cnormal(seed, r, nr * ns, philox.STREAM_NOISE).reshape(nr, ns)
    fnv = nv if cfg["mmse"] else 0.0
    est = np.stack([omimo.blast_decode(Y, Hest, fnv), omimo.blast_decode(Y, H, fnv)])
    dec = omodem.demodulate(tab, est)
    return dict(H=H, Hest=Hest, Hest_lstsq=Hest2, est=est, est_lstsq=omimo.blast_decode(Y, Hest2, fnv), idx=idx, dec=dec,
                se=np.array([omodem.count_symbol_errors(idx, dec[b]) for b in range(2)]),
                be=np.array([int(omodem.count_bit_errors(idx, dec[b])) for b in range(2)]),
                err=float(np.sum(np.abs(Hest - H) ** 2)), pow=float(np.sum(np.abs(H) ** 2)), gap=_gap(tab, est),
                gram_cond=float(np.linalg.cond(s @ sh)))


def run(cfg, first, count, seed=None):
    """Realizations first .. first + count - 1: se / be [2, count], err, pow, gap, route (the largest move of an estimate by
    the second route), gram_cond [count], and the per-realization symbol / bit counts n_symbols, n_bits."""
    outs = [realization(cfg, r, seed) for r in range(int(first), int(first) + int(count))]
    res = dict(se=np.stack([o["se"] for o in outs], axis=1), be=np.stack([o["be"] for o in outs], axis=1),
               err=np.array([o["err"] for o in outs]), pow=np.array([o["pow"] for o in outs]),
               gap=np.array([o["gap"] for o in outs]), gram_cond=np.array([o["gram_cond"] for o in outs]),
               route=np.array([float(np.max(np.abs(o["est_lstsq"] - o["est"][0]))) for o in outs]),
               n_symbols=cfg["nt"] * cfg["n_symbols"], n_bits=cfg["nt"] * cfg["n_symbols"] * 4)
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement of a named case over realizations FIRST .. FIRST + COUNT - 1, computed once and shared (read-only)."""
    return run(ALL_CASES[name], FIRST, COUNT)


def err_rounding_bound(cfg, ref):
    """What f64 rounding can move err = |H^ - H|_F^2 by, relative, largest over the realizations of `ref`: the entries of H^ carry
    about sqrt(nt P) cond(s s^H) eps |H| of rounding (nt P accumulated terms, then the Gram solve), and the difference H^ - H is
    smaller than H by sqrt(err / pow), so err moves by 2 sqrt(nt P) cond eps / sqrt(err / pow).  The element-wise bar of
    1e-11 on err is a fair demand where this stays below it."""
    eps = np.finfo(np.float64).eps
    return float(np.max(2.0 * np.sqrt(cfg["nt"] * cfg["P"]) * ref["gram_cond"] * eps / np.sqrt(ref["err"] / ref["pow"])))
