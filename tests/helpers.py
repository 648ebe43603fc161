"""Shared helpers for the parity tests (test infrastructure)."""
import functools
import json
import os

import numpy as np

SEED = 20260927

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_cases(name):
    """Yield (kwargs, realization dicts) for every stored case of a chain fixture."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    out = []
    for ci in range(int(z["n_cases"])):
        kw = json.loads(str(z["case%d_kwargs" % ci]))
        for k, v in list(kw.items()):
            if isinstance(v, list):
                kw[k] = tuple(v)
        reals = []
        for r in range(int(z["n_real"])):
            pre = "case%d_r%d_" % (ci, r)
            reals.append({k[len(pre):]: z[k] for k in z.files if k.startswith(pre)})
        out.append((kw, reals))
    return out


def relerr(a, b):
    a = np.asarray(a)
    b = np.asarray(b)
    scale = max(1.0, float(np.max(np.abs(b)))) if b.size else 1.0
    return float(np.max(np.abs(a - b))) / scale if a.size else 0.0


def oracle_counts(fn, first, count, **kw):
    from oracle import chains
    se, be = [], []
    for r in range(first, first + count):
        out = fn(chains.PhiloxRng(SEED, r), **kw)
        se.append(out["symbol_errors"])
        be.append(out["bit_errors"])
    return np.array(se), np.array(be), out["num_symbols"], out["num_bits"]


def check(res, se, be, want_se, want_be, nsym, nbits, exact):
    cnt = res
    assert cnt["n_realizations"] == len(want_se) and cnt["n_skipped"] == 0
    assert cnt["n_symbols"] == nsym and cnt["n_bits"] == nbits
    assert cnt["sym_errors"] == int(se.sum()) and cnt["bit_errors"] == int(be.sum())
    assert cnt["sym_errors_sq"] == int((se.astype(np.int64) ** 2).sum())
    assert cnt["bit_errors_sq"] == int((be.astype(np.int64) ** 2).sum())
    if exact:
        assert np.array_equal(se, want_se) and np.array_equal(be, want_be)
    else:
        n = len(want_se)
        assert abs(int(se.sum()) - int(want_se.sum())) / (n * nsym) <= 1e-4
        assert abs(int(be.sum()) - int(want_be.sum())) / (n * nbits) <= 1e-4


# ---- the flat MIMO link against the exact (canonical-phase) oracle: cases shared by test_oracle_mimo_canonical.py (CPU:
# the conditions on the inputs) and test_gpu_mimo_flat_exact.py (GPU: the kernels) -------------------------------------
FLAT_FIRST, FLAT_COUNT = 3, 70      # a wave takes 16 realizations: four full chunks and one of 6, two workgroups
FLAT_COLUMNS = (130, 51, 2)         # even (two columns per lane, a last pass with one busy lane) / odd (one column per lane) / one pair
FLAT_SNR = 16.0
# (scheme, N, mmse) with 16-QAM at FLAT_SNR and canonical=True
SVD_GMD_CASES = [("svd", n, False) for n in (2, 3, 4)] + [("gmd", n, m) for n in (2, 3, 4) for m in (False, True)]
# (scheme, nt, nr) with mmse=True, 16-QAM at MMSE_SNR, where MMSE and zero-forcing decisions differ
MMSE_SNR = 6.0
MMSE_CASES = [("blast", 1, 1), ("blast", 2, 2), ("blast", 2, 3), ("blast", 3, 4), ("blast", 4, 4), ("mrc", 1, 3)]
MMSE_COLUMNS = (130, 51)
# complex64 decision forms x layer count: Blast zero forcing (a phase-free oracle), 1 .. 4 layers
FORM_SHAPES = [(1, 2), (2, 2), (3, 4), (4, 4)]
FORM_COLUMNS = (130, 51)
# (id, mod, M, demodulator, snr_db): an SNR at which every form still makes errors
FORMS = [("qam16-slicer", "qam", 16, "slicer", 16.0), ("qam16-mindist", "qam", 16, "mindist", 16.0),
         ("psk8-mindist", "psk", 8, "mindist", 14.0), ("bpsk", "bpsk", 2, "mindist", 4.0),
         ("qam64-mindist", "qam", 64, "mindist", 22.0)]


def decision_margins(table, est):
    """Distance of every estimate from the border of its decision region (the Voronoi cell of the nearest constellation
    point: min over the other points c of the distance to the bisector of (nearest, c)); for square QAM these are the
    slicer's thresholds too."""
    table = np.asarray(table, dtype=complex)
    est = np.asarray(est, dtype=complex).reshape(-1)
    d2 = np.abs(est[:, None] - table[None, :]) ** 2
    near = np.argmin(d2, axis=1)
    rows = np.arange(est.size)
    sep = np.abs(table[None, :] - table[near][:, None])
    sep[rows, near] = 1.0
    m = (d2 - d2[rows, near][:, None]) / (2.0 * sep)
    m[rows, near] = np.inf
    return np.min(m, axis=1)


@functools.lru_cache(maxsize=None)
def flat_reference(scheme, mod, M, nt, nr, ns, snr, mmse=False, canonical=False):
    """oracle.chains.chain_mimo_scheme over realizations FLAT_FIRST .. FLAT_FIRST + FLAT_COUNT - 1, computed once per case
    and shared (read-only): per-realization counts plus the inputs and estimates the CPU checks need."""
    from oracle import chains
    kw = dict(scheme=scheme, mod=mod, M=M, nt=nt, nr=nr, NSymbs=ns, snr_db=snr, mmse=mmse, canonical=canonical)
    outs = [chains.chain_mimo_scheme(chains.PhiloxRng(SEED, r), **kw) for r in range(FLAT_FIRST, FLAT_FIRST + FLAT_COUNT)]
    ref = dict(se=np.array([o["symbol_errors"] for o in outs]), be=np.array([o["bit_errors"] for o in outs]),
               nsym=outs[0]["num_symbols"], nbits=outs[0]["num_bits"], table=outs[0]["table"], noise_var=outs[0]["noise_var"],
               H=np.stack([o["H"] for o in outs]), idx=np.stack([o["idx"] for o in outs]),
               noise=np.stack([o["noise"] for o in outs]), est=np.stack([o["est"] for o in outs]))
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref
