"""No GPU: the conditions that make "exact" a fair demand of the large-array pilot link (csrc/pipeline_mimo_large_pilot.hip) on the
very inputs tests/test_gpu_large_pilot.py uses (large_pilot_cases.CASES: realizations 3 .. 72 of pilot_link_oracle.SEED, 16-QAM),
asserted on the NumPy restatement alone.  The cap on realizations left out of the exact comparison is ZERO: every realization of
every case has to meet every condition.

Measured on these ten cases (worst figure, its case):
    smallest decision gap of a realization                          5.6e-7    ls-L-5x7         (floor 1e-9)
    move of an estimate by the lstsq route, share of the gap        3.8e-8    8x8-p16          (cap 1e-3)
    closest totals of the two blocks                                7011 / 6986 symbol errors, 6x16-p255
    err_rounding_bound                                              3.9e-12   7x9-p12          (cap 0.5e-11)
    smallest margin / largest difference of the formulations        7e5       ls-L-5x7         (floor 1e3)
    decisions changed by the formulation in NumPy complex64         0 everywhere

The kernels' formulation: normal-equation Cholesky of M^H M + nv I for M = H^ (block 0) and M = H (block 1),
G = sqrt(Nt) (M^H M + nv I)^-1 M^H, A = G H / sqrt(Nt) with the TRUE H in both blocks, est = A x + G n."""
import math

import numpy as np
import pytest

from oracle import chains
from oracle import modem as omodem
from oracle import philox

import pilot_link_oracle as po
from helpers import decision_margins
from large_pilot_cases import CASES, COUNT, FIRST, NAMES, PLAIN, SEED, reference

GAP_FLOOR = 1e-9           # every realization's smallest decision gap
ROUTE_SHARE = 1e-3         # the estimate by a second route moves no est by more than this share of the gap
MARGIN_RATIO = 1e3         # smallest decision margin over the largest difference between the formulations


def _kernel_formulation(M, H, nv, nt):
    """G of the channel knowledge M through the Cholesky factor of the normal equations; A = G H / sqrt(Nt) with the true H"""
    L = np.linalg.cholesky(M.conj().T @ M + nv * np.eye(nt))
    G = math.sqrt(nt) * np.linalg.solve(L.conj().T, np.linalg.solve(L, M.conj().T))
    return G @ H / math.sqrt(nt), G


def _estimates(name):
    """Per realization and block (oracle estimate [nt, ns], the kernel formulation's, A, G, x, scaled noise)."""
    cfg, ref = CASES[name], reference(name)
    nt, nr, ns, nv = cfg["nt"], cfg["nr"], cfg["n_symbols"], cfg["noise_var"]
    fnv = nv if cfg["mmse"] else 0.0
    tab = po.table()
    for i, r in enumerate(range(FIRST, FIRST + COUNT)):
        x = tab[ref["idx"][i]].reshape((nt, ns), order="F")
        n = math.sqrt(nv) * philox.cnormal(cfg["seed"], r, nr * ns, philox.STREAM_NOISE).reshape(nr, ns)
        for b, M in enumerate((ref["Hest"][i], ref["H"][i])):
            A, G = _kernel_formulation(M, ref["H"][i], fnv, nt)
            yield b, ref["est"][i][b].reshape((nt, ns), order="F"), A @ x + G @ n, A, G, x, n


def test_the_case_table():
    assert len(CASES) == 10 and (FIRST, COUNT) == (3, 70) and SEED == po.SEED
    shapes = {n: (c["nt"], c["nr"], c["P"], c["n_symbols"]) for n, c in CASES.items()}
    assert shapes["1x16-p1"] == (1, 16, 1, 130) and shapes["6x16-p255"] == (6, 16, 255, 51) and shapes["8x16-p9"] == (8, 16, 9, 130)
    assert {s[3] for s in shapes.values()} == {33, 34, 51, 130}
    assert sorted(PLAIN) == sorted(set(NAMES) - {"mmse-est-1x16", "ls-L-5x7"})
    for name in ("mmse-est-1x16", "ls-L-5x7"):
        assert CASES[name]["alpha"] == 0.7 and CASES[name]["L"].shape == (CASES[name]["nr"],) * 2
    assert CASES["mmse-est-1x16"]["estimator"] == "mmse" and CASES["mmse-est-1x16"]["cov"].shape == (16, 16)


@pytest.mark.parametrize("name", NAMES)
def test_no_realization_is_near_a_decision_border(name):
    ref = reference(name)
    print(name, "smallest gap %.3g, largest route move as a share of the gap %.3g, largest Gram condition %.3g"
          % (ref["gap"].min(), float(np.max(ref["route"] / ref["gap"])), ref["gram_cond"].max()))
    assert ref["gap"].shape == (COUNT,)
    assert np.all(ref["gap"] >= GAP_FLOOR), int(np.sum(ref["gap"] < GAP_FLOOR))
    assert np.all(ref["route"] <= ROUTE_SHARE * ref["gap"]), int(np.sum(ref["route"] > ROUTE_SHARE * ref["gap"]))


@pytest.mark.parametrize("name", NAMES)
def test_estimated_and_perfect_csi_give_different_counts(name):
    cfg, ref = CASES[name], reference(name)
    assert cfg["noise_var"] > 0
    print(name, "symbol errors estimated %d perfect %d, bit errors %d / %d"
          % (ref["se"][0].sum(), ref["se"][1].sum(), ref["be"][0].sum(), ref["be"][1].sum()))
    assert ref["se"][0].sum() != ref["se"][1].sum() and ref["be"][0].sum() != ref["be"][1].sum()
    assert ref["se"].max() > 0 and np.min(ref["err"] / ref["pow"]) > 0


@pytest.mark.parametrize("name", NAMES)
def test_the_error_bar_is_above_the_rounding_of_the_subtraction(name):
    """|H^ - H|^2 is held at 1e-11 relative on the GPU: what f64 rounding can move it by stays below half of that."""
    cfg, ref = CASES[name], reference(name)
    bound = po.err_rounding_bound(cfg, ref)
    print(name, "smallest err / pow %.3g, modelled rounding of err %.3g" % (np.min(ref["err"] / ref["pow"]), bound))
    assert bound <= 0.5e-11


@pytest.mark.parametrize("name", NAMES)
def test_decision_margins_dwarf_the_difference_of_formulations(name):
    tab = po.table()
    margin, diff = np.inf, 0.0
    for _b, est, mine, *_rest in _estimates(name):
        margin = min(margin, float(decision_margins(tab, est).min()))
        diff = max(diff, float(np.max(np.abs(est - mine))))
    print("%s: smallest margin %.2g, largest estimate difference %.2g, ratio %.2g" % (name, margin, diff, margin / diff))
    assert margin / diff >= MARGIN_RATIO


@pytest.mark.parametrize("name", NAMES)
def test_the_formulation_alone_decides_the_same_in_complex64(name):
    """A and G rounded from complex128, a sequential float accumulate: 0 decisions change in either block, so the GPU test's
    complex64 bound (at most 3 symbol errors of difference in a realization) has the reference alone at 0 inside it."""
    cfg, tab = CASES[name], po.table()
    nt, nr, ns = cfg["nt"], cfg["nr"], cfg["n_symbols"]
    changed = [0, 0]
    for b, est, _mine, A, G, x, n in _estimates(name):
        A32, G32, x32, n32 = (v.astype(np.complex64) for v in (A, G, x, n))
        acc = np.zeros((nt, ns), dtype=np.complex64)
        for c in range(nt):
            acc = acc + A32[:, c:c + 1] * x32[c:c + 1, :]
        for r in range(nr):
            acc = acc + G32[:, r:r + 1] * n32[r:r + 1, :]
        assert acc.dtype == np.complex64
        changed[b] += int(np.count_nonzero(omodem.demodulate(tab, acc) != omodem.demodulate(tab, est)))
    print("%s: complex64 changes %d decisions with estimated CSI, %d with perfect CSI" % ((name,) + tuple(changed)))
    assert changed == [0, 0]


@pytest.mark.parametrize("name", PLAIN)
def test_perfect_csi_half_is_the_blast_chain(name):
    cfg, ref = CASES[name], reference(name)
    assert cfg["L"] is None and cfg["alpha"] == 1.0
    for i, r in enumerate(range(FIRST, FIRST + COUNT)):
        out = chains.chain_mimo_scheme(chains.PhiloxRng(SEED, r), "blast", mod="qam", M=16, nt=cfg["nt"], nr=cfg["nr"],
                                       NSymbs=cfg["n_symbols"], snr_db=cfg["snr_db"], mmse=cfg["mmse"])
        assert out["noise_var"] == cfg["noise_var"]
        assert (out["symbol_errors"], out["bit_errors"]) == (ref["se"][1, i], ref["be"][1, i]), (name, r)
        assert (out["num_symbols"], out["num_bits"]) == (ref["n_symbols"], ref["n_bits"])
