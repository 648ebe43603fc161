"""No GPU: when "exact" is a fair demand of the large-array Blast link (csrc/pipeline_mimo_large.hip), on the very inputs
tests/test_gpu_mimo_large.py uses (mimo_large_cases.CASES: realizations 3 .. 72 of helpers.SEED, 16-QAM, chain_mimo_scheme), and
the kernels' operand maps (csrc/mimo_large_map.hpp) as a stand-alone host program.

Margins.  The kernels do not solve the oracle's way: normal-equation Cholesky of H^H H + nv I, then A = G H / sqrt(Nt), then
est = A x + G n, against pinv / solve and est = G (H X + n).  Per case the smallest decision margin (helpers.decision_margins)
over the largest estimate difference between the oracle and a NumPy statement of that formulation must be >= 1e3.  Measured:

    case                               smallest margin   largest difference   ratio
    8 x 8 ZF, 30 dB, 130 columns       2.0e-05           1.6e-11              1.3e+06   (largest cond(H) 357)
    8 x 8 MMSE, 14 dB, 130 columns     4.6e-06           7.6e-14              6.1e+07
    8 x 16 ZF, 8 dB, 130 columns       1.2e-07           1.3e-14              9.1e+06
    5 x 6 ZF, 20 dB, 51 columns        4.6e-05           2.9e-14              1.6e+09
    6 x 16 MMSE, 6 dB, 51 columns      2.6e-05           2.2e-15              1.2e+10
    1 x 16 ZF, -4 dB, 130 columns      4.7e-05           1.5e-15              3.1e+10
    7 x 9 ZF, 18 dB, 34 columns        5.4e-06           2.2e-14              2.5e+08

Complex64.  The oracle's own link in NumPy complex64 (A and G rounded from complex128, a sequential float accumulate) differs
from its complex128 decisions in 0 symbols in every case: asserted, so the bound of the GPU test (at most 3 symbol errors of
difference in a realization) has the reference alone at 0 inside it."""
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import modem as omodem

from helpers import FLAT_COUNT, decision_margins
from mimo_large_cases import CASE_IDS, CASES, reference

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kernel_formulation(H, nv, nt):
    """G = sqrt(Nt) (H^H H + nv I)^-1 H^H through the Cholesky factor, A = G H / sqrt(Nt)."""
    L = np.linalg.cholesky(H.conj().T @ H + nv * np.eye(nt))
    Z = np.linalg.solve(L, H.conj().T)
    G = math.sqrt(nt) * np.linalg.solve(L.conj().T, Z)
    return G @ H / math.sqrt(nt), G


def _estimates(ref, nt, nr, mmse, ns):
    """Per realization (oracle estimate [nt, ns], the kernel formulation's, A, G, x, scaled noise)."""
    sigma = math.sqrt(ref["noise_var"])
    for b in range(FLAT_COUNT):
        A, G = _kernel_formulation(ref["H"][b], ref["noise_var"] if mmse else 0.0, nt)
        x = ref["table"][ref["idx"][b]].reshape((nt, ns), order="F")
        n = sigma * ref["noise"][b]
        yield ref["est"][b].reshape((nt, ns), order="F"), A @ x + G @ n, A, G, x, n


@pytest.mark.parametrize("nt,nr,mmse,snr,ns", CASES, ids=CASE_IDS)
def test_decision_margins_dwarf_the_difference_of_formulations(nt, nr, mmse, snr, ns):
    ref = reference(nt, nr, mmse, snr, ns)
    assert ref["se"].max() > 0 and ref["H"].shape == (FLAT_COUNT, nr, nt)
    margin, diff, cond = np.inf, 0.0, 0.0
    for b, (est, mine, *_rest) in enumerate(_estimates(ref, nt, nr, mmse, ns)):
        margin = min(margin, float(decision_margins(ref["table"], est).min()))
        diff = max(diff, float(np.max(np.abs(est - mine))))
        cond = max(cond, float(np.linalg.cond(ref["H"][b])))
    print("%d x %d mmse=%d %g dB %d columns: smallest margin %.2g, largest estimate difference %.2g, ratio %.2g, largest "
          "cond(H) %.0f, %d errors in %d symbols" % (nt, nr, mmse, snr, ns, margin, diff, margin / diff, cond, ref["se"].sum(),
                                                     FLAT_COUNT * ref["nsym"]))
    assert margin / diff >= 1e3


@pytest.mark.parametrize("nt,nr,mmse,snr,ns", CASES, ids=CASE_IDS)
def test_the_reference_alone_decides_the_same_in_complex64(nt, nr, mmse, snr, ns):
    ref = reference(nt, nr, mmse, snr, ns)
    table = ref["table"]
    changed = 0
    for est, _mine, A, G, x, n in _estimates(ref, nt, nr, mmse, ns):
        A32, G32, x32, n32 = (v.astype(np.complex64) for v in (A, G, x, n))
        acc = np.zeros((nt, ns), dtype=np.complex64)
        for c in range(nt):
            acc = acc + A32[:, c:c + 1] * x32[c:c + 1, :]
        for r in range(nr):
            acc = acc + G32[:, r:r + 1] * n32[r:r + 1, :]
        assert acc.dtype == np.complex64
        changed += int(np.count_nonzero(omodem.demodulate(table, acc) != omodem.demodulate(table, est)))
    print("%d x %d mmse=%d %g dB %d columns: complex64 changes %d decisions" % (nt, nr, mmse, snr, ns, changed))
    assert changed == 0


@pytest.mark.parametrize("nt,nr,mmse,snr,ns", [c for c in CASES if c[2]], ids=[i for i, c in zip(CASE_IDS, CASES) if c[2]])
def test_mmse_and_zero_forcing_counts_differ(nt, nr, mmse, snr, ns):
    assert not np.array_equal(reference(nt, nr, True, snr, ns)["se"], reference(nt, nr, False, snr, ns)["se"])


# ---- the operand maps --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mimo_large_map") / "mimo_large_map_dump")
    subprocess.run(["c++", "-std=c++17", "-I", "pyphysim_amd/csrc", "scripts/mimo_large_map_dump.cpp", "-o", exe], cwd=REPO,
                   check=True)                          # no host compiler or no header: this fails, it does not skip
    return exe


def _maps(exe, f64, nt, nr):
    out = subprocess.run([exe], input="%d %d %d\n" % (f64, nt, nr), capture_output=True, text=True, check=True).stdout.split("\n")
    steps = int(out[0].split()[1])
    rows = [ln.split() for ln in out[1:] if ln]
    pick = lambda tag: np.array([[int(v) for v in r[1:]] for r in rows if r[0] == tag])
    return steps, pick("L"), pick("R"), pick("D")


@pytest.mark.parametrize("f64", [1, 0], ids=["f64", "f32"])
@pytest.mark.parametrize("nt,nr", [(1, 1), (3, 5), (8, 8), (8, 16)])
def test_operand_maps_compute_the_link(dump, nt, nr, f64):
    """Scatter random A, G into the record by the dumped map, multiply as the real 16 x 4S matrix of the matrix-core
    instruction (lane l supplies L[l & 15][4 s + (l >> 4)] and R[4 s + (l >> 4)][l & 15]) by the real-embedded [x; n], read back
    by the instruction's C/D map (result i of lane l: row (l >> 4) + 4 i in f64, 4 (l >> 4) + i in f32): A x + G n to 1e-12,
    padding exactly zero."""
    steps, Lm, Rm, Dm = _maps(dump, f64, nt, nr)
    assert steps == 2 * (-(-nt // 4) - (-nr // 4)) and steps <= 12
    assert Lm.shape == (64 * steps, 7) and Rm.shape == (4 * steps, 5) and Dm.shape == (256, 5)
    rng = np.random.default_rng(nt * 100 + nr)
    cn = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    A, G, x, n = cn(nt, nt), cn(nt, nr), cn(nt, 16), cn(nr, 16)
    src = {1: A, 2: G}
    left = np.zeros((16, 4 * steps))
    used = set()
    for s, lane, kind, i, col, part, sign in Lm:
        if kind == 0:
            assert (i, col, part, sign) == (0, 0, 0, 0)
            continue
        v = src[kind][i, col]
        left[lane & 15, 4 * s + (lane >> 4)] = sign * (v.imag if part else v.real)
        used.add((kind, i, col))
    assert used == {(1, i, c) for i in range(nt) for c in range(nt)} | {(2, i, c) for i in range(nt) for c in range(nr)}
    right = np.zeros((4 * steps, 16))
    seen = set()
    for s, g, kind, idx, part in Rm:
        if kind == 0:
            continue
        v = (x if kind == 1 else n)[idx]
        right[4 * s + g] = v.imag if part else v.real
        seen.add((kind, idx, part))
        # Re and Im of one complex input sit in consecutive steps of the same lane group
        assert part == s % 2
    assert seen == {(1, a, p) for a in range(nt) for p in (0, 1)} | {(2, r, p) for r in range(nr) for p in (0, 1)}
    D = left @ right
    want = A @ x + G @ n
    got = np.zeros((nt, 16), dtype=complex)
    rows_read = set()
    for lane, i, row, stream, part in Dm:
        assert row == ((lane >> 4) + 4 * i if f64 else 4 * (lane >> 4) + i)
        if stream < 0:
            assert D[row, lane & 15] == 0.0                   # padded rows: exactly zero
            continue
        assert stream in (lane >> 4, (lane >> 4) + 4)         # both parts of a stream in ONE lane: no exchange
        got[stream, lane & 15] += (1j if part else 1.0) * D[row, lane & 15]
        rows_read.add((stream, part, lane & 15))
    assert len(rows_read) == 2 * nt * 16
    assert np.max(np.abs(got - want)) <= 1e-12
    pad = np.ones_like(left, dtype=bool)
    for s, lane, kind, *_ in Lm:
        if kind:
            pad[lane & 15, 4 * s + (lane >> 4)] = False
    assert np.all(left[pad] == 0.0)
