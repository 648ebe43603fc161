"""NumPy restatement (test infrastructure) of the CoMP link with an external interferer and of the results the
application forms from it -- written from include/mcle.h (mcle_run_comp: the draw ledger) and the reference's
apps/comp_BD/simulate_comp.py:311-621, on top of oracle/philox.py, oracle/bd.py and oracle/multiuser.py.  It shares no
code with the product.

    big_H        draw_big_H: stream 2, user block entry (i, c) at i n + c, interferer entry (i, e) at n^2 + i n_ext + e,
                 block (rx k, tx l) times sqrt(pathloss[k, l]), interferer column e of user k times sqrt(pathloss_ext[k, e])
    data         stream 0, active streams q = 0, 1, .. in user order, symbol j of stream q at q n_symbols + j
    noise        stream 1, receive antenna i, symbol j at i n_symbols + j, times sqrt(noise_var)
    interferer   stream 3, CN(0, 1) sample e n_symbols + j, times sqrt(pe)
"""
import math

import numpy as np

from oracle import bd as obd
from oracle import modem as omodem
from oracle import multiuser as omu
from oracle import philox

VARIANTS = ("None", "naive", "fixed", "capacity", "effec_throughput", "Whitening")


def table_for(mod, M):
    if mod == "qam":
        return omodem.qam_constellation(M)
    if mod == "bpsk":
        return omodem.bpsk_constellation()
    if mod == "qpsk":
        return omodem.psk_constellation(4, math.pi / 4.0)
    return omodem.psk_constellation(M)


def draw_big_H(seed, realization, K, r, n_ext, pathloss=None, pathloss_ext=None):
    n = K * r
    Hu = philox.cnormal(seed, realization, n * n, philox.STREAM_CHAN).reshape(n, n)
    He = philox.cnormal(seed, realization, n * n_ext, philox.STREAM_CHAN, offset=n * n).reshape(n, n_ext)
    if pathloss is not None:
        Hu = Hu * np.sqrt(np.kron(np.asarray(pathloss, dtype=float), np.ones((r, r))))
        if n_ext:
            He = He * np.sqrt(np.repeat(np.asarray(pathloss_ext, dtype=float).reshape(K, n_ext), r, axis=0))
    return np.hstack([Hu, He])


def draw_link_inputs(seed, realization, K, r, n_ext, Ns, n_symbols, M, noise_var, pe):
    """-> (data [sum Ns, n_symbols] int, interferer data [n_ext, n_symbols], noise [K r, n_symbols])."""
    q = int(np.sum(Ns))
    data = philox.symbols(seed, realization, q * n_symbols, M).reshape(q, n_symbols)
    ext = math.sqrt(pe) * philox.cnormal(seed, realization, n_ext * n_symbols, philox.STREAM_PHASE).reshape(n_ext, n_symbols)
    noise = math.sqrt(noise_var) * philox.cnormal(seed, realization, K * r * n_symbols,
                                                  philox.STREAM_NOISE).reshape(K * r, n_symbols)
    return data, ext, noise


def link(big_H, MsPk, W, data, ext, noise, table, slicer_M=None):
    """__simulate_for_one_metric (:528-556): precode, corrupt_concatenated_data, filter, demodulate.
    MsPk[k] [K r, Ns_k], W[k] [Ns_k, r].  -> dict(received [K r, n], est [sum Ns, n], decisions, sym_err [sum Ns],
    bit_err [sum Ns]) per active stream."""
    symbols = table[data]
    precoded = np.hstack(MsPk) @ symbols
    received = big_H @ np.vstack([precoded, ext]) + noise
    r = received.shape[0] // len(W)
    est = np.vstack([W[k] @ received[k * r:(k + 1) * r] for k in range(len(W))])
    dec = omodem.qam_slicer(slicer_M, est) if slicer_M else omodem.demodulate(table, est)
    return dict(received=received, est=est, decisions=dec, sym_err=np.sum(dec != data, 1),
                bit_err=omodem.count_bit_errors(dec, data, 1))


def to_slots(per_stream, Ns, r):
    """Per-active-stream values -> [K r] by stream slot k r + j, 0 on an inactive stream."""
    out = np.zeros(len(Ns) * r, dtype=np.asarray(per_stream).dtype)
    q = 0
    for k, ns in enumerate(Ns):
        out[k * r:k * r + ns] = per_stream[q:q + ns]
        q += ns
    return out


def stream_results(sym_err, bit_err, n_symbols, Kb, packet_length):
    """The application's per-realization figures from the per-active-stream counts (:556-590): returns dict of
    (value, total) pairs for ber / ser / per / spec_effic."""
    sym_err, bit_err = np.asarray(sym_err, dtype=float), np.asarray(bit_err, dtype=float)
    num_symbols = np.ones(sym_err.size) * n_symbols
    num_bits = num_symbols * Kb
    ber = bit_err / num_bits
    per = 1.0 - ((1.0 - ber) ** packet_length)
    num_packages = num_bits / packet_length
    return dict(ber=(float(np.sum(bit_err)), float(np.sum(num_bits))), ser=(float(np.sum(sym_err)), float(np.sum(num_symbols))),
                per=(float(np.sum(per * num_packages)), float(np.sum(num_packages))),
                spec_effic=(float(np.sum((1.0 - per) * Kb)), 1.0))


def jp_sinr(big_H, K, r, MsPk, W, noise_var, pe=1.0):
    """MultiUserChannelMatrixExtInt.calc_JP_SINR(MsPk, W^H) -> list over users of per-stream linear SINRs."""
    U = [w.conj().T for w in W]
    return omu.calc_sinr(big_H, [r] * K, [r] * K, MsPk, U, noise_var=noise_var, pe=pe, joint=True)


# ---- the modulators' closed forms (fundamental.py calcTheoreticalBER / PER / SpectralEfficiency) on LINEAR SINRs ----------
_erfc = np.vectorize(math.erfc, otypes=[float])


def qfunc(x):
    return 0.5 * _erfc(np.asarray(x, dtype=float) / math.sqrt(2.0))


def theoretical_ber(mod, M, sinr):
    sinr = np.asarray(sinr, dtype=float)
    Kb = omodem.level2bits(M)
    if mod == "bpsk":
        return qfunc(np.sqrt(2.0 * sinr))
    if mod == "qam":
        psc = 2.0 * (1.0 - 1.0 / math.sqrt(M)) * qfunc(np.sqrt(sinr * 3.0 / (M - 1.0)))
        return (2.0 * psc) / Kb
    return 1.0 / Kb * (2.0 * qfunc(np.sqrt(2.0 * sinr) * math.sin(math.pi / M)))


def throughput_value(mod, M, packet_length, sinrs):
    """'effective_throughput' value of a candidate: sum_i Kb (1 - PER_i), PER = 1 - (1 - BER)^L."""
    Kb = omodem.level2bits(M)
    per = 1.0 - ((1.0 - theoretical_ber(mod, M, sinrs)) ** packet_length)
    return float(np.sum(Kb * (1.0 - per)))


def capacity_value(sinrs):
    return float(np.sum(np.log2(1.0 + np.asarray(sinrs, dtype=float))))


def candidate_values(cand_sinr, variant, mod, M, packet_length):
    """cand_sinr [K, r, r] (row ns-1 = the SINRs with ns streams, zero padded) -> values [K, r]."""
    K, r, _ = cand_sinr.shape
    f = capacity_value if variant == "capacity" else (lambda s: throughput_value(mod, M, packet_length, s))
    return np.array([[f(cand_sinr[k, ns - 1, :ns]) for ns in range(1, r + 1)] for k in range(K)])


def near_tie(values):
    """The gap rule: True when some user's two best candidate values differ by at most 1e-9 |best| + 1e-12."""
    values = np.asarray(values, dtype=float)
    if values.shape[1] < 2:
        return False
    top = np.sort(values, axis=1)[:, ::-1]
    return bool(np.any(top[:, 0] - top[:, 1] <= 1e-9 * np.abs(top[:, 0]) + 1e-12))


def candidate_sinrs(big_H, K, r, iPu, noise_var, pe, Ms_bad=None):
    """EnhancedBD's candidates: [K, r, r], row ns-1 = the post-filter SINRs with ns streams (zero padded)."""
    n_tx = K * r
    Re = obd.cov_extint_plus_noise(big_H, K, r, n_tx, pe, noise_var)
    Msb = Ms_bad if Ms_bad is not None else obd.bd_no_power_scaling(big_H[:, :n_tx], K)[0]
    cand = np.zeros((K, r, r))
    for k in range(K):
        Msk = Msb[:, k * r:(k + 1) * r]
        Heq = big_H[k * r:(k + 1) * r, :n_tx] @ Msk
        for ns in range(1, r + 1):
            Pk = obd.stream_reduction_matrix(Re[k], ns) if ns < r else np.eye(r)
            Hred = Heq @ (Pk / (np.linalg.norm(Msk @ Pk, "fro") / math.sqrt(iPu)))
            cand[k, ns - 1, :ns] = obd.ebd_linear_sinrs(Hred, obd.ebd_receive_filter(Hred, Pk), Re[k])
    return cand


def solve(big_H, K, r, iPu, noise_var, pe, variant, num_streams=1, mod="psk", M=4, packet_length=60, Ms_bad=None):
    """The variant's (MsPk, W, Ns) from oracle/bd.py (LAPACK phases unless Ms_bad is given)."""
    if variant == "Whitening":
        out = obd.whitening_bd(big_H, K, r, r, iPu, noise_var, pe)
    elif variant == "None":
        out = obd.enhanced_bd(big_H, K, r, r, iPu, noise_var, pe, None)
    elif variant in ("naive", "fixed"):
        out = obd.enhanced_bd(big_H, K, r, r, iPu, noise_var, pe, variant, num_streams, Ms_bad=Ms_bad)
    elif variant == "capacity":
        out = obd.enhanced_bd(big_H, K, r, r, iPu, noise_var, pe, "capacity", Ms_bad=Ms_bad)
    else:
        out = obd.enhanced_bd(big_H, K, r, r, iPu, noise_var, pe, "effective_throughput",
                              metric_func=lambda s: throughput_value(mod, M, packet_length, s), Ms_bad=Ms_bad)
    MsPk, W, Ns = out
    return list(MsPk), list(W), [int(v) for v in Ns]
