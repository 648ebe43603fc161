"""The 50-digit MIMO-operator oracle (tests/mimo_ops_oracle.py) checked on the CPU: it agrees with oracle/mimo.py, every
input class has the property it claims, the NumPy errors that the GPU bounds are built from are finite and non-zero,
and the rank-deficiency tolerance of the operator kernels separates the deficient class from every other one."""
import mpmath as mp
import numpy as np
import pytest

import mimo_ops_oracle as mo
from oracle import mimo as omimo


def c128(x):
    return np.asarray(x).astype(np.complex128)


# ---- the oracle against oracle/mimo.py -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", mo.SIZES)
def test_oracle_agrees_with_numpy_oracle_on_rayleigh(n):
    o = mo.oracle("rayleigh", n, n, "f64")
    R50 = mo.oracle_gmd_R("rayleigh", n, "f64")
    for i in range(mo.PER_CLASS):
        H = o["H"][i]
        U, S, Vh = omimo.canonical_svd(H)
        assert np.max(np.abs(S - o["S"][i].astype(float))) <= 1e-12
        assert np.max(np.abs(U - c128(o["U"][i]))) <= 1e-12 and np.max(np.abs(Vh - c128(o["Vh"][i]))) <= 1e-12
        W, G = omimo.scheme_filters("svd", H, canonical=True)
        assert np.max(np.abs(W - c128(o["W"][i]))) <= 1e-12 and np.max(np.abs(G - c128(o["G"][i]))) <= 1e-12
        Q, R, P = omimo.gmd(U, S, Vh)
        Qm, Rm, Pm = mo.gmd(*o["usv"][i])
        assert np.max(np.abs(R - R50[i].astype(float))) <= 1e-12
        assert np.max(np.abs(Q - c128(mo.to_ld(Qm)))) <= 1e-12 and np.max(np.abs(P - c128(mo.to_ld(Pm)))) <= 1e-12
        # the 50-digit GMD is one: Q R P^H = H, Q and P unitary, R upper triangular with a constant diagonal
        assert mp.mnorm(Qm * Rm * Pm.transpose_conj() - o["Hm"][i], 1) <= mp.mpf(10) ** -45
        assert mp.mnorm(Qm.transpose_conj() * Qm - mp.eye(n), 1) <= mp.mpf(10) ** -45
        Wg, Gg = omimo.scheme_filters("gmd", H, 0.05, canonical=True)
        assert np.max(np.abs(Gg - c128(mo.to_ld(mo.blast_filter(Qm * Rm, 0.05))))) <= 1e-12


@pytest.mark.parametrize("nr,nt", mo.BLAST_SHAPES)
def test_blast_oracle_agrees_with_numpy_oracle_on_rayleigh(nr, nt):
    o = mo.oracle("rayleigh", nr, nt, "f64")
    for nv in (0.0, 0.1):
        G50 = mo.oracle_blast("rayleigh", nr, nt, "f64", nv)
        for i in range(mo.PER_CLASS):
            assert np.max(np.abs(omimo.blast_receive_filter(o["H"][i], nv) - c128(G50[i]))) <= 1e-12


def test_post_processing_sinrs_oracle_agrees_with_numpy_oracle():
    rs = np.random.RandomState(3)
    for nr, nt, ns, nv in ((3, 2, 2, 0.07), (4, 4, 3, 0.0)):
        H, W, G = (rs.randn(*s) + 1j * rs.randn(*s) for s in ((nr, nt), (nt, ns), (ns, nr)))
        got = mo.post_processing_linear_sinrs(mo.to_mp(H), mo.to_mp(W), mo.to_mp(G), nv)
        want = omimo.post_processing_linear_sinrs(H, W, G, nv)
        assert np.max(np.abs(np.array([float(v) for v in got]) / want - 1)) <= 1e-12


# ---- every class has the property it claims ------------------------------------------------------------------------
@pytest.mark.parametrize("nr,nt", mo.BLAST_SHAPES)
def test_classes_have_their_spectra(nr, nt):
    for cls in mo.CLASSES:
        H, meta = mo.matrices(cls, nr, nt)
        assert H.shape == (mo.PER_CLASS, nr, nt) and H.dtype == np.complex128 and np.all(np.isfinite(H))
        S = mo.oracle(cls, nr, nt, "f64")["S"]
        for i in range(mo.PER_CLASS):
            if meta["sigma"][i] is not None:                 # the spectrum set by construction, to a few roundings
                want = np.array(sorted(meta["sigma"][i], reverse=True))
                assert np.max(np.abs(S[i].astype(float) - want)) <= 8 * 2.0 ** -52 * want[0], (cls, i)
            if meta["cond"][i] is not None and np.isfinite(meta["cond"][i]):
                assert abs(float(S[i][0] / S[i][-1]) / meta["cond"][i] - 1) <= 0.01, (cls, i)
    assert np.all(mo.matrices("real", nr, nt)[0].imag == 0)
    assert np.array_equal(mo.matrices("identity", nr, nt)[0][0], np.eye(nr, nt))
    ray, sc = mo.matrices("rayleigh", nr, nt)[0], mo.matrices("scaled", nr, nt)[0]
    half = mo.PER_CLASS // 2
    assert np.array_equal(sc[:half], ray[:half] * 2.0 ** -40) and np.array_equal(sc[half:], ray[half:] * 2.0 ** 40)
    d = mo.matrices("diagonal", nr, nt)[0]
    assert np.all(d.imag == 0) and all(np.count_nonzero(m) == nt for m in d)
    if nt > 2:
        assert any(list(np.abs(np.diag(m[:nt]))) != sorted(np.abs(np.diag(m[:nt])), reverse=True) for m in d)
    if nt > 1:
        assert sorted(set(c for c in mo.matrices("graded", nr, nt)[1]["cond"])) == sorted(mo.GRADED_CONDS)


@pytest.mark.parametrize("nr,nt", mo.BLAST_SHAPES)
def test_deficient_has_the_constructed_rank(nr, nt):
    """sigma_{rank+1} / sigma_1 <= 1e-15 at 50 digits after the product was rounded to complex128, and sigma_rank is not small."""
    H, meta = mo.matrices("deficient", nr, nt)
    S = mo.oracle("deficient", nr, nt, "f64")["S"]
    assert set(meta["rank"]) == (set(range(1, nt)) if nt > 1 else {0})
    for i in range(mo.PER_CLASS):
        r = meta["rank"][i]
        assert r < nt
        if r == 0:
            assert not H[i].any()
            continue
        assert S[i][r] <= 1e-15 * S[i][0], (i, r, S[i])
        assert S[i][r - 1] >= 1e-3 * S[i][0], (i, r, S[i])


@pytest.mark.parametrize("n", mo.SIZES)
def test_gm_hit_has_a_sigma_at_the_geometric_mean(n):
    for S in mo.oracle("gm_hit", n, n, "f64")["S"]:
        bar = float(np.prod(S) ** (np.longdouble(1) / n))
        assert min(abs(float(s) - bar) for s in S) <= 1e-15 * bar, S


# ---- the NumPy errors the GPU bounds are built from ----------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_numpy_errors_are_finite_and_nonzero(dt):
    """bound = 8 max(e_np, eps scale): e_np = 0 or inf on a whole class would leave the floor, or nothing, as the bound."""
    for cls in mo.CLASSES:
        if cls == "deficient":
            continue
        for n in mo.SIZES:
            o = mo.oracle(cls, n, n, dt)
            e_S = max(mo.maxerr(mo.np_svd(o["H"][i], dt)[1], o["S"][i]) for i in range(mo.PER_CLASS))
            e_U = max(mo.unitarity(mo.np_svd(o["H"][i], dt)[0]) for i in range(mo.PER_CLASS))
            assert np.isfinite(e_S) and np.isfinite(e_U), (cls, n)
            # (LAPACK returns these two exactly: there the floor eps * scale IS the bound)
            assert (e_S > 0 and e_U > 0) or cls in ("identity", "diagonal"), (cls, n)
            if cls in ("rayleigh", "graded"):
                e_W = max(mo.maxerr(mo.np_svd_filters(o["H"][i], dt)[0], o["W"][i]) for i in range(mo.PER_CLASS))
                assert np.isfinite(e_W) and e_W > 0, (cls, n)
        for nr, nt in mo.BLAST_SHAPES:
            o = mo.oracle(cls, nr, nt, dt)
            kmax = 1e6 if dt == "f64" else 1e2
            for nv in (0.0, 0.1):
                G50 = mo.oracle_blast(cls, nr, nt, dt, nv)
                e = [mo.maxerr(mo.np_blast_filter(o["H"][i], nv, dt), G50[i]) for i in range(mo.PER_CLASS)
                     if o["cond"][i] <= 1.01 * kmax]
                assert e and np.all(np.isfinite(e)), (cls, nr, nt, nv)
                assert max(e) > 0 or cls in ("identity", "diagonal", "unitary") or nt == 1, (cls, nr, nt, nv)


# ---- the rank-deficiency tolerance of the operator kernels ---------------------------------------------------------
RANK_TOL = {"f64": 2.0 ** -42, "f32": 2.0 ** -34}          # kRankTol in csrc/kernels_mimo.hip


def pivot_ratios(H, nv):
    """The Cholesky of blast_filter_t in NumPy complex128 (the operator kernels eliminate in f64 for both dtypes; the
    device contracts multiply-adds differently): pivot_j / A[j][j], up to the first pivot that is not positive."""
    nr, nt = H.shape
    L = np.zeros((nt, nt), complex)
    out = []
    for j in range(nt):
        for i in range(j, nt):
            a = 0j
            for r in range(nr):
                a = a + H[r, j] * np.conj(H[r, i])
            if i == j:
                a = a.real + nv
                ajj = a
            for k in range(j):
                a = a - L[i, k] * np.conj(L[j, k])
            if i == j:
                out.append(a.real / ajj if ajj > 0 else 0.0)
                if not a.real > 0:
                    return out
                L[j, j] = np.sqrt(a.real)
            else:
                L[i, j] = a / L[j, j]
    return out


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_rank_tolerance_separates_deficient_from_the_rest(dt, capsys):
    """Normalised by the column's own diagonal entry, the smallest pivot ratio of every deficient matrix lies at least a
    factor 32 below the tolerance and that of every other class (graded up to cond 1e6 in f64, 1e2 in f32) at least a
    factor 4 above it.  (Normalised by the largest diagonal entry instead, the regular side comes 4 to 10 times closer.)"""
    tol = RANK_TOL[dt]
    worst_def, best_reg, best_reg_max = 0.0, np.inf, np.inf
    for cls in mo.CLASSES:
        for nr, nt in mo.BLAST_SHAPES:
            H, _ = mo.rounded(cls, nr, nt, dt)
            cond = mo.oracle(cls, nr, nt, dt)["cond"]
            for i in range(mo.PER_CLASS):
                r = min(pivot_ratios(H[i], 0.0))
                if cls == "deficient":
                    worst_def = max(worst_def, r)
                    assert min(pivot_ratios(H[i], 0.1)) > 1e-3        # H^H H + nv I is not deficient
                elif cond[i] <= 1.01 * (1e6 if dt == "f64" else 1e2):
                    best_reg = min(best_reg, r)
                    g = np.sum(np.abs(H[i]) ** 2, axis=0)
                    best_reg_max = min(best_reg_max, r * g.min() / g.max())
    with capsys.disabled():
        print("\n[%s] pivot / A_jj: deficient <= %.3g, others >= %.3g (>= %.3g against the largest diagonal entry), tolerance %.3g"
              % (dt, worst_def, best_reg, best_reg_max, tol))
    assert worst_def * 32 <= tol <= best_reg / 4
