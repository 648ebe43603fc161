"""CPU: the canonical-phase SVD / GMD oracle (oracle.mimo.canonical_svd, scheme_filters(canonical=True),
chains.chain_mimo_scheme(mmse=, canonical=)) against LAPACK's own pair, and the conditions on the inputs under which
tests/test_gpu_mimo_flat_exact.py may demand EQUAL per-realization counts from the complex128 kernels.

The device routine (csrc/mimo_svd.hpp: jacobi_svd) makes the largest-magnitude entry of every right singular vector real
and positive; canonical_svd states that in NumPy.  It is LAPACK's decomposition up to one unit-modulus factor per singular
pair, so everything that does not depend on the phases (S, the GMD's R, G H W) must agree with the LAPACK-phase oracle that
tests/test_oracle_golden.py pins to the reference, and the filters themselves must differ by a diagonal phase matrix only.

The conditions (pivot lead, singular-value gap, distance of every estimate from its decision border) are properties of the
chosen inputs, not measurements of any kernel: where they hold with orders of magnitude to spare, double-precision rounding
(1e-16, amplified by at most 1 / gap) cannot move a pivot, swap two columns or flip a decision."""
import math

import numpy as np
import pytest

from oracle import chains, mimo as omimo
from helpers import (FLAT_COLUMNS, FLAT_COUNT, FLAT_SNR, FORMS, FORM_COLUMNS, FORM_SHAPES, MMSE_CASES,
                     MMSE_COLUMNS, MMSE_SNR, SVD_GMD_CASES, decision_margins, flat_reference, relerr)

PIVOT_LEAD = 1e-6      # the pivot's modulus leads the runner-up's by at least this, relative (the kernel's tie band: 1e-12 in |.|^2)
SV_GAP = 1e-3          # adjacent singular values differ by at least this, relative
EST_MARGIN = 1e-9      # every complex128 estimate is at least this far from the border of its decision region


def _channels(n):
    """The 70 channels of the GPU tests (CHAN draws of realizations 3 .. 72; they do not depend on the column count)."""
    return flat_reference("svd", "qam", 16, n, n, 2, FLAT_SNR, False, True)["H"]


def _unit_diagonal(M, what):
    """M is diagonal with unit-modulus entries."""
    n = M.shape[0]
    assert np.max(np.abs(M - np.diag(np.diag(M)))) <= 1e-12, what
    assert np.max(np.abs(np.abs(np.diag(M)) - 1.0)) <= 1e-12, what
    return np.diag(M)


@pytest.mark.parametrize("n", [2, 3, 4])
def test_canonical_svd_is_lapacks_up_to_one_phase_per_pair(n):
    for r, H in enumerate(_channels(n)):
        U, S, V_H = omimo.canonical_svd(H)
        Ul, Sl, Vl_H = np.linalg.svd(H)
        assert np.array_equal(S, Sl) and np.all(np.diff(S) < 0)
        assert relerr((U * S) @ V_H, H) <= 1e-13
        assert relerr(U.conj().T @ U, np.eye(n)) <= 1e-13 and relerr(V_H @ V_H.conj().T, np.eye(n)) <= 1e-13
        V = V_H.conj().T
        for c in range(n):          # the stated convention: the pivot real and positive, the first of the largest
            p = int(np.argmax(np.abs(V[:, c])))
            assert abs(V[p, c].imag) <= 1e-15 and V[p, c].real > 0
            assert p == int(np.argmax(np.abs(Vl_H.conj().T[:, c])))
        Wc, Gc = omimo.scheme_filters("svd", H, canonical=True)
        Wl, Gl = omimo.scheme_filters("svd", H)
        d = _unit_diagonal(n * Wl.conj().T @ Wc, ("W", n, r))            # W_c = W_l D
        assert relerr(Wc, Wl * d[None, :]) <= 1e-13
        assert relerr(Gc, np.conj(d)[:, None] * Gl) <= 1e-13              # G_c = D^H G_l
        assert relerr(Gc @ H @ Wc, np.eye(n)) <= 1e-10


@pytest.mark.parametrize("n", [2, 3, 4])
def test_canonical_gmd(n):
    for r, H in enumerate(_channels(n)):
        Q, R, P = omimo.gmd(*omimo.canonical_svd(H))
        Ql, Rl, Pl = omimo.gmd(*np.linalg.svd(H))
        assert relerr(Q @ R @ P.conj().T, H) <= 1e-12
        assert relerr(Q.conj().T @ Q, np.eye(n)) <= 1e-12 and relerr(P.conj().T @ P, np.eye(n)) <= 1e-12
        assert np.array_equal(R, Rl)                                       # R depends on S only
        assert np.allclose(np.tril(R, -1), 0) and relerr(np.diag(R), np.full(n, np.prod(np.linalg.svd(H)[1]) ** (1.0 / n))) <= 1e-13
        W, G = omimo.scheme_filters("gmd", H, canonical=True)
        assert relerr(W, P / math.sqrt(n)) == 0.0
        assert relerr(G @ H @ W, np.eye(n)) <= 1e-9                        # zero forcing
        nv = 0.05
        Wm, Gm = omimo.scheme_filters("gmd", H, nv, canonical=True)
        Heq = Q @ R
        assert relerr(Wm, W) == 0.0
        assert relerr(Gm, math.sqrt(n) * np.linalg.solve(Heq.conj().T @ Heq + nv * np.eye(n), Heq.conj().T)) <= 1e-12
        assert relerr(Gm, G) > 1e-3                                        # the noise variance reached the filter


@pytest.mark.parametrize("n", [2, 3, 4])
def test_inputs_have_a_clear_pivot_and_distinct_singular_values(n):
    lead, gap = np.inf, np.inf
    for H in _channels(n):
        _, S, V_H = np.linalg.svd(H)
        for c in range(n):
            m = np.sort(np.abs(V_H.conj().T[:, c]))[::-1]
            lead = min(lead, (m[0] - m[1]) / m[0])
        gap = min(gap, float(np.min((S[:-1] - S[1:]) / S[:-1])))
    print("N = %d: smallest pivot lead %.3g, smallest singular-value gap %.3g" % (n, lead, gap))
    assert lead >= PIVOT_LEAD
    assert gap >= SV_GAP


def _exact_cases():
    out = []
    for scheme, n, mmse in SVD_GMD_CASES:
        for ns in FLAT_COLUMNS:
            out.append((scheme, "qam", 16, n, n, ns, FLAT_SNR, mmse, True))
    for scheme, nt, nr in MMSE_CASES:
        for ns in MMSE_COLUMNS:
            out.append((scheme, "qam", 16, nt, nr, ns, MMSE_SNR, True, False))
    for _id, mod, M, _method, snr in FORMS:
        for nt, nr in FORM_SHAPES:
            for ns in FORM_COLUMNS:
                out.append(("blast", mod, M, nt, nr, ns, snr, False, False))
    return sorted(set(out))


EXACT_CASES = _exact_cases()


@pytest.mark.parametrize("case", EXACT_CASES, ids=lambda c: "%s-%s%d-%dx%d-%d-%gdB%s" % (c[0], c[1], c[2], c[3], c[4], c[5], c[6],
                                                                                          "-mmse" if c[7] else ""))
def test_no_estimate_sits_on_a_decision_border(case):
    """Every complex128 estimate of every case the GPU tests demand equal counts for is at least 1e-9 from the border of
    its decision region, and the case makes errors at all."""
    ref = flat_reference(*case)
    margin = float(np.min(decision_margins(ref["table"], ref["est"])))
    print("%s: smallest decision margin %.3g, %d symbol errors" % (case, margin, int(ref["se"].sum())))
    assert margin >= EST_MARGIN
    assert ref["se"].max() > 0
    assert len(ref["se"]) == FLAT_COUNT and ref["nsym"] == case[5] * case[3]


@pytest.mark.parametrize("scheme,n,mmse", SVD_GMD_CASES)
def test_canonical_and_lapack_phases_give_other_decisions(scheme, n, mmse):
    """The phases matter: on the same draws the canonical and the LAPACK-phase links decide differently in some
    realization, so a kernel with another phase convention cannot pass the exact comparison."""
    a = flat_reference(scheme, "qam", 16, n, n, 130, FLAT_SNR, mmse, True)
    b = flat_reference(scheme, "qam", 16, n, n, 130, FLAT_SNR, mmse, False)
    assert not np.array_equal(a["se"], b["se"])
    # ... while both are the same link statistically: the channel gains |G H W| = I and the noise power per stream agree
    assert abs(int(a["se"].sum()) - int(b["se"].sum())) <= 0.1 * int(b["se"].sum())


@pytest.mark.parametrize("scheme,nt,nr", MMSE_CASES)
def test_mmse_and_zero_forcing_decide_differently(scheme, nt, nr):
    for ns in MMSE_COLUMNS:
        a = flat_reference(scheme, "qam", 16, nt, nr, ns, MMSE_SNR, True, False)
        b = flat_reference(scheme, "qam", 16, nt, nr, ns, MMSE_SNR, False, False)
        assert not np.array_equal(a["se"], b["se"])


def test_default_path_is_unchanged():
    """mmse=False, canonical=False: the chain the golden fixture pins (the reference's own formulas on LAPACK's pair)."""
    for scheme, n in (("svd", 3), ("gmd", 4)):
        out = chains.chain_mimo_scheme(chains.PhiloxRng(1, 5), scheme, "qam", 16, n, n, 20, 12.0)
        H = out["H"]
        U, S, V_H = np.linalg.svd(H)
        W, G = omimo.scheme_filters(scheme, H)
        assert np.array_equal(out["W"], W) and np.array_equal(out["G_H"], G)
        if scheme == "svd":
            assert np.array_equal(W, V_H.conj().T / math.sqrt(n))


def emulate_complex64(ref, W, G):
    """est = A d + G n in NumPy complex64, A = G H W and G rounded from the complex128 oracle: the decisions a complex64
    statement of the same link takes, for comparison with the complex128 ones.  W, G: [count, ., .] stacks."""
    table = ref["table"]
    nt = ref["H"].shape[2]
    se = []
    for r in range(len(ref["se"])):
        A = (G[r] @ ref["H"][r] @ W[r]).astype(np.complex64)
        G32 = G[r].astype(np.complex64)
        idx = ref["idx"][r]
        d = table[idx].astype(np.complex64).reshape(nt, -1)
        n32 = (math.sqrt(ref["noise_var"]) * ref["noise"][r]).astype(np.complex64)
        est = (A @ d + G32 @ n32).reshape(-1)
        dec = np.argmin(np.abs(est[:, None] - table.astype(np.complex64)[None, :]), axis=1)
        se.append(int(np.count_nonzero(dec != idx)))
    return np.array(se)


@pytest.mark.parametrize("scheme,n,mmse", SVD_GMD_CASES)
def test_the_reference_alone_stays_inside_the_complex64_bound(scheme, n, mmse):
    """Before the GPU tests rely on the complex64 bound (totals within 1e-4 of the symbols, at most 3 per realization): the
    oracle's own link evaluated in complex64 stays inside it against its complex128 decisions."""
    for ns in FLAT_COLUMNS:
        ref = flat_reference(scheme, "qam", 16, n, n, ns, FLAT_SNR, mmse, True)
        nv = ref["noise_var"] if mmse else 0.0
        WG = [omimo.scheme_filters(scheme, H, nv, canonical=True) for H in ref["H"]]
        se32 = emulate_complex64(ref, [w for w, _ in WG], [g for _, g in WG])
        diff = se32 - ref["se"]
        print("%s N=%d mmse=%d columns=%d: complex64 emulation %d vs %d symbol errors, max per realization %d"
              % (scheme, n, mmse, ns, se32.sum(), ref["se"].sum(), np.max(np.abs(diff))))
        assert abs(int(diff.sum())) / (FLAT_COUNT * ref["nsym"]) <= 1e-4
        assert np.max(np.abs(diff)) <= 3
