#!/usr/bin/env python3
"""Writes tests/golden/g5_comp.npz: the reference's own CoMP-with-external-interference results for
tests/test_comp_cpu.py and tests/test_gpu_comp.py.

Drives the reference (darcamo/pyphysim v0.7.2) the way scripts/make_golden_estimators.py does -- the stub modules of
oracle/ref_shim on sys.path, PYPHYSIM_REFERENCE naming its checkout -- and holds none of it: the steps below are the calls
apps/comp_BD/simulate_comp.py makes on the library's objects (cell.Grid, PathLoss3GPP1, MultiUserChannelMatrixExtInt,
EnhancedBD / WhiteningBD, the modulators), made from here.  Arrays only.

Contents:
  pathloss [3, 3], pathlossInt [3, 1], path_loss_border: the 'Symmetric Far Away' scenario (three cells of radius 1 km, one
      user per cell at 70 % of the way to the border, angles 210 / -30 / 90 degrees), 3GPP scenario-1 path loss;
  single realizations r<i>_<variant>_*: at (SNR 5 dB, Pe 10 dBm), four channels x six variants: big_H, the interferer's
      data, the noise, the symbol indices, MsPk / W / Ns, the received and decoded arrays, per-stream counts, calc_JP_SINR;
  ref_p<point>_<figure>_<variant>_{sum,sq}: a seeded run of `ref_realizations` realizations at (5 dB, 10 dBm) and
      (15 dB, -10 dBm): sum and sum of squares of the per-realization ser, ber, per, spec_effic and mean SINR; ns_hist.

usage: PYPHYSIM_REFERENCE=/path/to/pyphysim python scripts/make_golden_comp.py
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("PYPHYSIM_REFERENCE", "/root/reference")
OUT = os.path.join(REPO, "tests", "golden", "g5_comp.npz")

VARIANTS = ("None", "naive", "fixed", "capacity", "effec_throughput", "Whitening")
K, NR, EXT, M, NSYMBS, PACKET, N0_DBM = 3, 2, 1, 4, 500, 60, -116.4
POINTS = [(5.0, 10.0), (15.0, -10.0)]
REF_REALIZATIONS = 2000
SINGLE_NSYMBS = 40


def build_fixture():
    sys.path.insert(0, os.path.join(REPO, "oracle", "ref_shim"))
    sys.path.insert(0, REF)
    np.int = int
    from pyphysim.cell import cell
    from pyphysim.channels import multiuser, pathloss
    from pyphysim.comm.blockdiagonalization import EnhancedBD, WhiteningBD
    from pyphysim.modulators import fundamental
    from pyphysim.util import misc
    from pyphysim.util.conversion import dB2Linear, dBm2Linear

    out = {}
    # ---- the scenario ----
    plo = pathloss.PathLoss3GPP1()
    grid = cell.Grid()
    grid.create_clusters(1, K, 1.0)
    cluster0 = grid.get_cluster_from_index(0)
    cluster0.delete_all_users()
    cluster0.add_border_users(np.arange(1, K + 1), np.array([210, -30, 90]), 0.7)
    pl = plo.calc_path_loss(cluster0.calc_dist_all_users_to_each_cell())
    to_center = np.array([cluster0.calc_dist(u) for u in cluster0.get_all_users()])
    pl_int = plo.calc_path_loss(cluster0.external_radius - to_center).reshape(K, 1)
    border = plo.calc_path_loss(1.0)
    noise_var = dBm2Linear(N0_DBM)
    out.update(pathloss=np.asarray(pl, dtype=float), pathlossInt=np.asarray(pl_int, dtype=float), path_loss_border=np.float64(border),
               noise_var=np.float64(noise_var), cfg=np.array([K, NR, EXT, M, PACKET]), ref_points=np.array(POINTS),
               ref_realizations=np.int64(REF_REALIZATIONS), ref_nsymbs=np.int64(NSYMBS), ref_packet_length=np.int64(PACKET),
               transmit_power=np.array([dB2Linear(s) * noise_var / border for s, _ in POINTS]))

    modulator = fundamental.PSK(M)
    Kb = modulator.K

    def solvers(snr, pe_dbm):
        pt, pe = dB2Linear(snr) * dBm2Linear(N0_DBM) / border, dBm2Linear(pe_dbm)
        extra = {"modulator": modulator, "packet_length": PACKET, "num_streams": 1}
        objs = {}
        for v in VARIANTS:
            if v == "Whitening":
                objs[v] = WhiteningBD(K, pt, noise_var, pe)
            else:
                objs[v] = EnhancedBD(K, pt, noise_var, pe)
                objs[v].set_ext_int_handling_metric("effective_throughput" if v == "effec_throughput" else v, extra)
        return objs, pe

    def one_metric(muc, MsPk, W, Ns, ext_data, nsymbs, data_seed, noise_seed):
        """the steps of BDSimulationRunner.__simulate_for_one_metric"""
        input_data = np.random.RandomState(data_seed).randint(0, M, [int(np.sum(Ns)), nsymbs])
        symbols = modulator.modulate(input_data)
        precoded = np.dot(np.hstack(list(MsPk)), symbols)
        all_data = np.vstack([precoded, ext_data])
        muc.set_noise_seed(noise_seed)
        received = muc.corrupt_concatenated_data(all_data)
        from scipy.linalg import block_diag
        est = np.dot(block_diag(*W), received)
        decoded = modulator.demodulate(est)
        sym_err = np.sum(decoded != input_data, 1)
        bit_err = misc.count_bit_errors(decoded, input_data, 1)
        num_bits = np.ones(int(np.sum(Ns))) * nsymbs * Kb
        ber = bit_err / num_bits
        per = 1.0 - ((1.0 - ber) ** PACKET)
        packages = num_bits / PACKET
        U = np.empty(K, dtype=np.ndarray)
        F = np.empty(K, dtype=np.ndarray)
        for k in range(K):
            U[k], F[k] = W[k].conjugate().T, MsPk[k]
        sinr = muc.calc_JP_SINR(F, U)
        return dict(input_data=input_data, all_data=all_data, received=received, decoded=decoded, sym_err=sym_err, bit_err=bit_err,
                    ser=np.sum(sym_err) / (np.sum(Ns) * nsymbs), ber=np.sum(bit_err) / np.sum(num_bits),
                    per=np.sum(per * packages) / np.sum(packages), spec_effic=np.sum((1.0 - per) * Kb),
                    sinr=np.concatenate([np.asarray(s, dtype=float) for s in sinr]))

    # ---- single realizations ----
    muc = multiuser.MultiUserChannelMatrixExtInt()
    muc.noise_var = noise_var
    muc.set_channel_seed(20261019)
    ext_rs = np.random.RandomState(611)
    objs, pe = solvers(*POINTS[0])
    for i in range(4):
        muc.randomize(NR, NR, K, EXT)
        muc.set_pathloss(pl, pl_int)
        big_H = np.array(muc.big_H)
        ext_data = np.sqrt(pe) * misc.randn_c_RS(ext_rs, EXT, SINGLE_NSYMBS)
        for v in VARIANTS:
            MsPk, W, Ns = objs[v].block_diagonalize_no_waterfilling(muc)
            o = one_metric(muc, MsPk, W, Ns, ext_data, SINGLE_NSYMBS, 2105 + i, 4445 + i)
            tag = "r%d_%s_" % (i, v)
            out[tag + "big_H"], out[tag + "ext_data"] = big_H, ext_data
            out[tag + "noise"] = o["received"] - np.dot(big_H, o["all_data"])
            out[tag + "input_data"], out[tag + "Ns"] = o["input_data"], np.asarray(Ns, dtype=np.int64)
            for k in range(K):
                out[tag + "MsPk%d" % k], out[tag + "W%d" % k] = np.asarray(MsPk[k]), np.asarray(W[k])
            out[tag + "received"], out[tag + "decoded"] = o["received"], o["decoded"]
            out[tag + "sym_err"], out[tag + "bit_err"] = o["sym_err"], o["bit_err"]
            out[tag + "results"] = np.array([o["ser"], o["ber"], o["per"], o["spec_effic"]])
            out[tag + "sinr"] = o["sinr"]
    out["single_point"] = np.array(POINTS[0])
    out["single_pe"] = np.float64(pe)

    # ---- seeded runs ----
    for pi, (snr, pe_dbm) in enumerate(POINTS):
        objs, pe = solvers(snr, pe_dbm)
        muc = multiuser.MultiUserChannelMatrixExtInt()
        muc.noise_var = noise_var
        muc.set_channel_seed(22522 + pi)
        ext_rs = np.random.RandomState(6114 + pi)
        sums = {}
        hist = np.zeros((len(VARIANTS), NR + 1), dtype=np.int64)
        for rep in range(REF_REALIZATIONS):
            muc.randomize(NR, NR, K, EXT)
            muc.set_pathloss(pl, pl_int)
            ext_data = np.sqrt(pe) * misc.randn_c_RS(ext_rs, EXT, NSYMBS)
            for vi, v in enumerate(VARIANTS):
                MsPk, W, Ns = objs[v].block_diagonalize_no_waterfilling(muc)
                o = one_metric(muc, MsPk, W, Ns, ext_data, NSYMBS, 1000003 * (pi + 1) + rep, 7000003 * (pi + 1) + 6 * rep + vi)
                for n in Ns:
                    hist[vi, int(n)] += 1
                for m, val in (("ser", o["ser"]), ("ber", o["ber"]), ("per", o["per"]), ("spec_effic", o["spec_effic"]),
                               ("sinr", float(np.mean(o["sinr"])))):
                    s = sums.setdefault((m, v), [0.0, 0.0])
                    s[0] += val
                    s[1] += val * val
        for (m, v), (s1, s2) in sums.items():
            out["ref_p%d_%s_%s_sum" % (pi, m, v)], out["ref_p%d_%s_%s_sq" % (pi, m, v)] = np.float64(s1), np.float64(s2)
        out["ref_p%d_ns_hist" % pi] = hist
    return out


if __name__ == "__main__":
    fixture = build_fixture()
    np.savez_compressed(OUT, **fixture)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(fixture), os.path.getsize(OUT)))
