#!/usr/bin/env python3
"""Writes tests/golden/g6_quant_ia.npz: the reference's own limited-feedback IA results for tests/test_quant_cpu.py,
tests/test_gpu_quantize.py and tests/test_gpu_ia_quantized.py.

Drives the reference (darcamo/pyphysim v0.7.2) the way scripts/make_golden_comp.py does -- the stub modules of oracle/ref_shim on
sys.path, PYPHYSIM_REFERENCE naming its checkout -- and holds none of it.  The functions of apps/ia/simple_maxsinr_quantized.py
(gen_codebook, calc_dist, calc_angle_dist, my_quant_func) are imported and called; the steps of its __main__ block (which passes
`map` objects and so does not run under Python 3) are the same library calls made from here with lists.  Arrays only.

Contents:
  cb<i>_codebook [C, dim], cb<i>_cfg = (C, Nr, Nt, K): gen_codebook under np.random.seed, (C, dim) = (512, 4), (17, 9), (5, 4);
  cb<i>_H [n, K Nr, K Nt], cb<i>_Hq: channels and my_quant_func's output; cb<i>_index [n, K, K]: the argmin of every link;
  cb<i>_rows_link [n, 2] = (channel, link), cb<i>_rows_dist / cb<i>_rows_angle [n, C]: the full calc_dist / calc_angle_dist
      rows of n links (8 for the 512-word codebook, else 20);
  r<i>_<solver>_*: six single realizations of the whole application at 15 dB, BPSK, NSymbs 50, codebook cb0, solver 'closed_form'
      (ClosedFormIASolver) and 'max_sinr' (MaxSinrIASolver, 120 iterations, start stored): big_H, Hq, F_init, F, U (= full_W_H),
      idx, noise (unit variance), received, est, decoded, symbol_errors, bit_errors, sinr (calc_SINR on the true channel),
      sum_capacity, runned_iterations.

usage: PYPHYSIM_REFERENCE=/path/to/pyphysim python scripts/make_golden_quant_ia.py
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("PYPHYSIM_REFERENCE", "/root/reference")
OUT = os.path.join(REPO, "tests", "golden", "g6_quant_ia.npz")

CODEBOOKS = [(512, 2, 2, 3, 24), (17, 3, 3, 2, 32), (5, 2, 2, 3, 32)]     # (C, Nr, Nt, K, channels)
N_ROWS = {512: 8, 17: 20, 5: 20}
N_SINGLE, SNR_DB, NSYMBS, MAX_IT = 6, 15.0, 50, 120


def build_fixture():
    sys.path.insert(0, os.path.join(REPO, "oracle", "ref_shim"))
    sys.path.insert(0, REF)
    np.int = int
    from apps.ia import simple_maxsinr_quantized as app
    from pyphysim.channels import multiuser
    from pyphysim.ia import algorithms
    from pyphysim.modulators import fundamental
    from pyphysim.util import misc
    from pyphysim.util.conversion import dB2Linear

    out = {}
    books = []
    for ci, (C, nr, nt, K, n) in enumerate(CODEBOOKS):
        np.random.seed(20261019 + ci)
        cb = app.gen_codebook(C, nr * nt)
        books.append(cb)
        H = np.stack([misc.randn_c(K * nr, K * nt) for _ in range(n)])
        Hq = np.stack([app.my_quant_func(h, nr, nt, K, cb) for h in H])
        index = np.empty((n, K, K), dtype=np.int64)
        for b in range(n):
            for k1 in range(K):
                for k2 in range(K):
                    v = H[b, k1 * nr:(k1 + 1) * nr, k2 * nt:(k2 + 1) * nt].reshape(-1)
                    index[b, k1, k2] = np.argmin([app.calc_dist(v, c) for c in cb])
        links = np.array([(i % n, (7 * i) % (K * K)) for i in range(N_ROWS[C])])
        rows_d, rows_a = np.empty((N_ROWS[C], C)), np.empty((N_ROWS[C], C))
        for i, (b, l) in enumerate(links):
            k1, k2 = divmod(int(l), K)
            v = H[b, k1 * nr:(k1 + 1) * nr, k2 * nt:(k2 + 1) * nt].reshape(-1)
            rows_d[i] = [app.calc_dist(v, c) for c in cb]
            rows_a[i] = [app.calc_angle_dist(v, c) for c in cb]
        pre = "cb%d_" % ci
        out[pre + "codebook"], out[pre + "cfg"] = cb, np.array([C, nr, nt, K])
        out[pre + "H"], out[pre + "Hq"], out[pre + "index"] = H, Hq, index
        out[pre + "rows_link"], out[pre + "rows_dist"], out[pre + "rows_angle"] = links, rows_d, rows_a

    # ---- single realizations of the application (its __main__ block, :170-273) ----
    K, nr, nt, Ns, M = 3, 2, 2, 1, 2
    noise_var = 1.0 / dB2Linear(SNR_DB)
    modulator = fundamental.BPSK()
    cb = books[0]
    for solver_name in ("closed_form", "max_sinr"):
        for i in range(N_SINGLE):
            np.random.seed(31000 + i)
            muc, muc_q = multiuser.MultiUserChannelMatrix(), multiuser.MultiUserChannelMatrix()
            muc.noise_var = noise_var
            muc_q.noise_var = noise_var
            muc.set_noise_seed(4100 + i)
            if solver_name == "closed_form":
                solver = algorithms.ClosedFormIASolver(muc_q, use_best_init=True)
            else:
                solver = algorithms.MaxSinrIASolver(muc_q)
                solver._rs = np.random.RandomState(5200 + i)
                solver.max_iterations = MAX_IT
            idx = np.random.randint(0, M, [K * Ns, NSYMBS])
            sym = modulator.modulate(idx)
            tx = np.split(sym, np.cumsum(np.ones(K, dtype=int) * Ns)[:-1])
            big_H = misc.randn_c(K * nr, K * nt)
            Hq = app.my_quant_func(big_H, nr, nt, K, cb)
            muc.init_from_channel_matrix(big_H, nr, nt, K)
            muc_q.init_from_channel_matrix(Hq, nr, nt, K)
            F_init = {"F": [np.zeros((nt, Ns), dtype=complex)] * K}
            if solver_name == "max_sinr":
                orig = solver.randomizeF

                def spy(Ns_, P=None, orig=orig, solver=solver, F_init=F_init):
                    orig(Ns_, P)
                    F_init["F"] = [np.array(f) for f in solver._F]
                solver.randomizeF = spy
            runned = solver.solve(Ns)
            pre = [np.dot(f, x) for f, x in zip(solver.full_F, tx)]
            rx = muc.corrupt_data(pre)
            est = np.vstack([np.dot(u, y) for u, y in zip(solver.full_W_H, rx)])
            dec = modulator.demodulate(est)
            sinr = muc.calc_SINR(solver.F, solver.W)
            tag = "r%d_%s_" % (i, solver_name)
            out[tag + "big_H"], out[tag + "Hq"] = big_H, Hq
            out[tag + "F_init"] = np.stack([np.asarray(f).reshape(-1) for f in F_init["F"]])
            out[tag + "F"] = np.stack([np.asarray(f).reshape(-1) for f in solver.full_F])
            out[tag + "U"] = np.stack([np.asarray(u).reshape(-1) for u in solver.full_W_H])
            out[tag + "idx"], out[tag + "noise"] = idx, muc.last_noise / np.sqrt(noise_var)
            out[tag + "received"], out[tag + "est"], out[tag + "decoded"] = np.vstack(list(rx)), est, dec
            out[tag + "symbol_errors"] = np.int64(np.sum(idx != dec))
            out[tag + "bit_errors"] = np.int64(misc.count_bit_errors(idx, dec))
            out[tag + "sinr"] = np.concatenate([np.asarray(s, dtype=float) for s in sinr])
            out[tag + "sum_capacity"] = np.float64(np.sum(np.log2(1 + np.hstack(sinr))))
            out[tag + "runned_iterations"] = np.int64(0 if runned is None else runned)
    out["single_cfg"] = np.array([N_SINGLE, NSYMBS, MAX_IT])
    out["single_snr_db"], out["noise_var"] = np.float64(SNR_DB), np.float64(noise_var)
    return out


if __name__ == "__main__":
    fixture = build_fixture()
    np.savez_compressed(OUT, **fixture)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(fixture), os.path.getsize(OUT)))
