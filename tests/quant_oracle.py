"""NumPy restatement (test infrastructure) of the codebook channel quantizer and of the limited-feedback IA link -- written from
include/mcle.h (mcle_quantize_links, mcle_run_ia_quantized) and the reference's apps/ia/simple_maxsinr_quantized.py:40-154,
170-273, on top of oracle/philox.py, oracle/ia.py and oracle/modem.py.  It shares no code with the product.

    link (k1, k2) of big_H [K Nr, K Nt]: the block big_H[k1 Nr:(k1+1) Nr, k2 Nt:(k2+1) Nt].reshape(-1)
    euclidean (calc_dist):        || v / ||v|| - c ||^2
    chordal (calc_angle_dist):    1 - |v^H c|^2 / (||v||^2 ||c||^2)
    index = argmin (lowest index on a tie); a block of zeros -> 0
    pipeline: big_H from stream 2 (as mcle_run_ia), quantized link by link, the solver on the quantized blocks (iterative solvers:
    the start from stream 3), data / noise as mcle_run_ia draws them, transmitted through the drawn big_H; SINR and capacity by
    calc_SINR on the drawn big_H.
"""
import math

import numpy as np

from oracle import ia as oia
from oracle import modem as omodem
from oracle import philox
from oracle.chains import STREAM_INIT, PhiloxRng, constellation

METRICS = ("euclidean", "chordal")


def links_of(big_H, K, nr, nt):
    """big_H [batch, K nr, K nt] -> v [batch, K, K, nr nt]"""
    H = np.asarray(big_H)
    b = H.shape[0]
    return H.reshape(b, K, nr, K, nt).transpose(0, 1, 3, 2, 4).reshape(b, K, K, nr * nt)


def distances(v, codebook, metric, dtype=np.complex128):
    """v [..., dim], codebook [C, dim] -> d [..., C] in the real type of `dtype`, the reference's formulas as written."""
    v = np.asarray(v).astype(dtype)
    c = np.asarray(codebook).astype(dtype)
    rt = np.float32 if np.dtype(dtype) == np.complex64 else np.float64
    with np.errstate(invalid="ignore", divide="ignore"):
        nv = np.sqrt(np.sum(np.abs(v) ** 2, axis=-1, dtype=rt))[..., None]
        if metric == "euclidean":
            vh = (v / nv).astype(dtype)
            diff = vh[..., None, :] - c
            return np.sum(np.abs(diff) ** 2, axis=-1, dtype=rt)
        nc = np.sqrt(np.sum(np.abs(c) ** 2, axis=-1, dtype=rt))
        ip = np.einsum("...d,cd->...c", v.conj(), c).astype(dtype)
        cos_sq = (np.abs(ip) / (nv * nc)).astype(rt) ** 2
        return (rt(1) - cos_sq).astype(rt)


def quantize(big_H, codebook, K, nr, nt, metric="euclidean", dtype=np.complex128):
    """-> dict(index [b, K, K], big_Hq [b, K nr, K nt], dist [b, K, K] (chosen), gap [b, K, K]: second smallest - smallest
    distance of the link, inf with one codeword)."""
    H = np.asarray(big_H)
    if H.ndim == 2:
        H = H[None]
    cb = np.asarray(codebook)
    b = H.shape[0]
    d = distances(links_of(H, K, nr, nt), cb, metric, dtype).astype(np.float64)
    zero = np.isnan(d).all(axis=-1)
    d_safe = np.where(np.isnan(d), np.inf, d)
    index = np.argmin(d_safe, axis=-1)
    index[zero] = 0
    if cb.shape[0] > 1:
        part = np.partition(d_safe, 1, axis=-1)
        with np.errstate(invalid="ignore"):
            gap = part[..., 1] - part[..., 0]
    else:
        gap = np.full(index.shape, np.inf)
    dist = np.take_along_axis(d, index[..., None], axis=-1)[..., 0]
    Hq = cb[index].reshape(b, K, K, nr, nt).transpose(0, 1, 3, 2, 4).reshape(b, K * nr, K * nt)
    return dict(index=index, big_Hq=Hq, dist=dist, gap=gap)


def restatement_error(fixture, metric, dtype):
    """Worst |restatement - reference| over the fixture's full calc_dist / calc_angle_dist rows, in `dtype`."""
    worst = 0.0
    for ci in range(3):
        pre = "cb%d_" % ci
        C, nr, nt, K = (int(x) for x in fixture[pre + "cfg"])
        v = links_of(fixture[pre + "H"], K, nr, nt).reshape(-1, K * K, nr * nt)
        rows = fixture[pre + ("rows_dist" if metric == "euclidean" else "rows_angle")]
        for (b, l), want in zip(fixture[pre + "rows_link"], rows):
            got = distances(v[b, l], fixture[pre + "codebook"], metric, dtype).astype(np.float64)
            worst = max(worst, float(np.max(np.abs(got - want))))
    return worst


def distance_tolerance(fixture, metric, dtype):
    """The project's convention: 8 x the restatement's own worst error against the reference in the same arithmetic."""
    return 8.0 * restatement_error(fixture, metric, dtype)


def draw_big_H(seed, realization):
    return philox.cnormal(seed, realization, 36, philox.STREAM_CHAN).reshape(6, 6)


def true_sinr(big_H, F, U, noise_var):
    return np.concatenate([np.asarray(s, dtype=float) for s in oia.calc_SINR(oia.split_blocks(big_H, 3, 2, 2), F, U, noise_var)])


def solve_quantized(Hq, solver, noise_var, F_init=None, max_iterations=120, relative_factor=1e-6):
    """-> (F, U = full_W_H, runned, ok) of `solver` on the quantized channel Hq [6, 6]."""
    Hb = oia.split_blocks(np.asarray(Hq), 3, 2, 2)
    try:
        with np.errstate(all="ignore"):
            if solver == "closed_form":
                sol = oia.closed_form_solve(Hb, 1, noise_var)
                if sol is None:
                    return None, None, 0, False
                F, U, runned = sol[0], sol[1], 0
            else:
                F, U, _, _, runned = oia.iterative_solve(solver, Hb, F_init, noise_var, max_iterations, relative_factor)
    except np.linalg.LinAlgError:
        return None, None, 0, False
    ok = all(np.all(np.isfinite(f)) for f in F) and all(np.all(np.isfinite(u)) for u in U)
    return F, U, runned, ok


def link_run(big_H, F, U, idx, noise, noise_var, table):
    """Precode, MultiUserChannelMatrix.corrupt_data on the TRUE channel, filter, demodulate (app :234-254)."""
    sym = omodem.modulate(table, idx)
    X = np.vstack([F[k] @ sym[k:k + 1] for k in range(3)])
    Y = oia.mu_corrupt(big_H, X, noise, noise_var)
    est = np.vstack([U[k] @ Y[2 * k:2 * k + 2] for k in range(3)])
    dec = omodem.demodulate(table, est)
    return dict(received=Y, est=est, decisions=dec, symbol_errors=int(omodem.count_symbol_errors(idx, dec)),
                bit_errors=int(omodem.count_bit_errors(idx, dec)))


def chain(seed, realization, codebook, metric="euclidean", solver="closed_form", mod="bpsk", M=2, NSymbs=50, snr_db=15.0,
          max_iterations=120, relative_factor=1e-6, dtype=np.complex128):
    """One realization of mcle_run_ia_quantized."""
    rng = PhiloxRng(seed, realization)
    table = constellation(mod, M)
    noise_var = 1.0 / float(omodem.dB2Linear(snr_db))
    big_H = rng.cn(philox.STREAM_CHAN, 6, 6)
    q = quantize(big_H.astype(dtype), np.asarray(codebook).astype(dtype), 3, 2, 2, metric, dtype)
    F_init = None
    if solver != "closed_form":
        F_init = []
        for k in range(3):
            f = rng.cn(STREAM_INIT, 2, 1)
            F_init.append(f / np.linalg.norm(f, "fro"))
    F, U, runned, ok = solve_quantized(q["big_Hq"][0].astype(np.complex128), solver, noise_var, F_init, max_iterations, relative_factor)
    idx = rng.symbols(3 * NSymbs, M).reshape(3, NSymbs)
    noise = rng.cn(philox.STREAM_NOISE, 6, NSymbs)
    out = dict(big_H=big_H, index=q["index"][0], gap=q["gap"][0], dist=q["dist"][0], big_Hq=q["big_Hq"][0], ok=ok, idx=idx,
               noise=noise, noise_var=noise_var, runned_iterations=runned, num_symbols=idx.size,
               num_bits=idx.size * omodem.level2bits(M))
    if ok:
        out.update(link_run(big_H, F, U, idx, noise, noise_var, table))
        out["sinr"] = true_sinr(big_H, F, U, noise_var)
        out["sum_capacity"] = float(np.sum(np.log2(1.0 + out["sinr"])))
        out["F"], out["U"] = F, U
    return out


# ---- the cases tests/test_gpu_quantize.py runs and tests/test_quant_cpu.py checks the gap rule's precondition on ----
# (C, Nr, Nt, K, batch)
OPERATOR_CASES = [(1, 2, 2, 3, 5), (2, 1, 1, 2, 3), (15, 2, 2, 3, 7), (16, 2, 2, 3, 7), (17, 2, 2, 3, 7), (33, 2, 3, 4, 4),
                  (17, 3, 3, 2, 9), (64, 6, 6, 2, 5), (512, 2, 2, 3, 33), (4096, 6, 6, 1, 2)]
GAP_CAP = 0.01          # share of a case's links the gap rule may leave out


def randn_c(rs, *shape):
    return (rs.randn(*shape) + 1j * rs.randn(*shape)) / math.sqrt(2.0)


def random_codebook(rs, C, dim):
    """unit-norm rows h / ||h||, h ~ CN(0, I)"""
    h = randn_c(rs, C, dim)
    return h / np.linalg.norm(h, axis=1, keepdims=True)


def operator_inputs(case, dtype=np.complex128):
    """The case's (big_H [batch, K Nr, K Nt], codebook [C, Nr Nt]) rounded to `dtype`: a fixed seed per case."""
    C, nr, nt, K, batch = case
    rs = np.random.RandomState(7100 + 13 * C + 5 * nr + 3 * nt + K)
    cb = random_codebook(rs, C, nr * nt)
    H = randn_c(rs, batch, K * nr, K * nt)
    return H.astype(dtype), cb.astype(dtype)


def pipeline_codebook(C=512, seed=99, dtype=np.complex128):
    return random_codebook(np.random.RandomState(seed), C, 4).astype(dtype)


# the drawn channels of tests/test_gpu_ia_quantized.py
PIPE_SEED, PIPE_FIRST, PIPE_COUNT = 20261019, 5, 128
