"""CPU: the 50-digit oracle of the 3-user 2x2 IA solvers (tests/ia3_oracle.py, tests/golden/g10_ia3_envelope.npz) tied to
oracle/ia.py and to the reference's own results, and the conditions under which tests/test_gpu_ia3_envelope.py may compare
the kernel tightly, shown from the oracles alone.  No GPU."""
import numpy as np
import pytest

import ia3_oracle as o
import ia_general_oracle as iao
from conftest import load_golden
from oracle import ia as oia

RAYLEIGH = [c for c in o.CASES if c["cls"] == "rayleigh"]


def _want(fx, r):
    return dict(PF=iao.herm_unpack(fx["PF"][r]), PU=iao.herm_unpack(fx["PU"][r]), sinr=fx["sinr"][r],
                capacity=float(fx["capacity"][r]))


def test_fixture_covers_the_case_table():
    fx = o.load_fixture()
    assert list(fx) == [c["name"] for c in o.CASES]
    for c in o.CASES:
        assert all(v.shape[0] == c["n_real"] for v in fx[c["name"]].values()), c["name"]
    # rayleigh: every solver x start x regime (alt-min refuses its own start)
    assert len([c for c in RAYLEIGH if c["solver"] != "closed_form" and c["noise_var"] == 0.01]) == (4 * 4 - 1) * 2
    assert {c["cls"] for c in o.CASES} | {"scaled"} == set(o.CLASSES) | {"scaled"} and len(o.CLASSES) == 13
    assert {c["noise_var"] for c in o.CASES} == {0.01, 0.0, 1e3}


@pytest.mark.parametrize("case", RAYLEIGH, ids=lambda c: c["name"])
def test_numpy_oracle_against_mp(case):
    """oracle/ia.py at f64 against the mp result on generic channels, to the tolerance tests/test_oracle_golden.py holds it
    to against the reference: 1e-9 for the closed form, 1e-7 for the iterative solvers; MMSE at the 1.5e-8 of its secant."""
    f = o.load_fixture()[case["name"]]
    tol = 1e-9 if case["solver"] == "closed_form" else (1.5e-8 if case["solver"] == "mmse" else 1e-7)
    for r in range(case["n_real"]):
        big_H, F_init = o.draw(case, r)
        got = o.numpy_solve(case, big_H, F_init)
        e = o.errors(got, _want(f, r))
        print("NP-MP %s r%d %s (stored %s)" % (case["name"], r, e, f["e_np"][r]))
        assert f["skipped"][r] == 0 and np.all(e <= tol), (case["name"], r, e)
        if o.iterations_pinned(f):
            assert got["iterations"] == f["iterations"][r]


def test_closed_form_reproduces_the_reference():
    """The mp closed form on the channels of c5_ia (written by the reference itself): F -- LAPACK's phase included --, U,
    SINRs and capacity.  This ties the oracle to pyphysim, not only to its restatement."""
    import mpmath as mp
    z = load_golden("c5_ia")
    worst = 0.0
    for ci in range(int(z["n_cases"])):
        for r in range(int(z["n_real"])):
            g = {k: z["case%d_r%d_%s" % (ci, r, k)] for k in ("big_H", "noise_var", "F", "U", "sinr", "sum_capacity")}
            cf = o.closed_form(iao._blocks(g["big_H"], 3, 2, 2), mp.mpf(float(g["noise_var"])))
            c = cf["cands"][cf["choice"]]
            F, U = o._F_array(c["F"]), np.array([[complex(u[0, 0]), complex(u[0, 1])] for u in c["U"]])
            e = [iao.relmax(F, g["F"]), iao.relmax(U, g["U"]), iao.relmax([float(s[0]) for s in c["sinr"]], g["sinr"]),
                 abs(float(c["cap"]) - float(g["sum_capacity"])) / float(g["sum_capacity"])]
            worst = max(worst, max(e))
            assert max(e) <= 1e-9, (ci, r, e)
    print("closed form against c5_ia: worst relative error %.2e" % worst)


ONE_PER_CLASS = [[c for c in o.CASES if c["cls"] == cls][0]["name"] for cls in sorted(o.CLASSES)]
CURRENT = ONE_PER_CLASS + ["near_repeated1e-09-closed_form", "graded1e+10-closed_form", "orth_start-min_leakage-fix-rel0-it8",
                           "direct_identity-mmse-svd-rel0-it8", "cross_identity-max_sinr-closed_form-rel0-it8",
                           "rayleigh-min_leakage-alt_min-rel0-it8"]


@pytest.mark.parametrize("name", CURRENT)
def test_fixture_is_current(name):
    """One case per class (and one per added start) recomputed at 50 digits from its seed equals the stored bits."""
    c, f = o.CASE_BY_NAME[name], o.load_fixture()[name]
    for r in range(c["n_real"]):
        got = o.run_case(c, r)
        for key in ("sinr", "capacity", "iterations", "skipped", "margins"):
            assert np.array_equal(np.asarray(got[key], dtype=np.float64), f[key][r], equal_nan=True), (name, r, key)
        for key in ("PF", "PU"):
            assert np.array_equal(iao.herm_pack(got[key]), f[key][r], equal_nan=True), (name, r, key)
        assert np.array_equal(np.stack([got["F"].real, got["F"].imag], axis=-1), f["F"][r], equal_nan=True)
        if c["solver"] == "closed_form":
            assert np.array_equal(got["cand_capacity"], f["cand_capacity"][r], equal_nan=True) and got["choice"] == f["choice"][r]


def test_strict_share():
    """Every realization of every rayleigh case is strict; in every other class at least 2 of 3 of every case are, except
    the cases whose class names the reason (o.NOT_STRICT_BY_CLASS), pinned here by name."""
    fx = o.load_fixture()
    worst_bound = 0.0
    for c in o.CASES:
        f = fx[c["name"]]
        strict = o.strict_realizations(c, f)
        if c["name"] in o.NOT_STRICT_BY_CLASS:
            continue
        assert strict.sum() >= (3 if c["cls"] == "rayleigh" else 2), (c["name"], f["kappa"].max(axis=0), f["margins"].min(axis=0))
        assert np.all(np.isfinite(f["e_np"][strict])), c["name"]
        worst_bound = max(worst_bound, float(o.bounds(f, strict).max()))
    print("strict set: bounds <= %.3g" % worst_bound)
    # e_np is at most the 1.5e-8 of the MMSE secant, kappa x 2^-52 at most 1e6 x 2^-52
    assert worst_bound <= 16 * 1.5e-8
    assert sorted(o.NOT_STRICT_BY_CLASS) == sorted(
        ["real_pair-closed_form", "near_repeated1e-06-closed_form", "near_repeated1e-09-closed_form",
         "graded1e+08-closed_form", "graded1e+10-closed_form", "graded1e+10-max_sinr-fix-rel0-it8", "graded1e+10-mmse-fix-rel0-it8",
         "cross_equal-closed_form", "cross_equal-min_leakage-closed_form-rel0-it8", "cross_equal-max_sinr-closed_form-rel0-it8",
         "orth_start-alt_min-fix-rel0-it8", "orth_start-min_leakage-fix-rel0-it8"]
        + ["%s-%s-fix-rel0-it8" % (cls, s) for cls in ("diagonal", "singular") for s in o.SOLVERS
           if (cls, s) not in (("singular", "alt_min"), ("singular", "min_leakage"))]
        + ["diagonal-closed_form", "singular-closed_form"]
        + ["%s-%s-svd-rel0-it8" % (cls, s) for cls in ("direct_identity", "direct_unitary") for s in o.SOLVERS])


def test_the_named_reasons_hold():
    """real_pair: the two candidates are complex conjugates of one another and tie; diagonal and singular: the closed form
    has no solution at 50 digits; near_repeated: the gap is the one asked for; graded: the condition number is."""
    fx = o.load_fixture()
    m = o._M
    f = fx["real_pair-closed_form"]
    assert np.all(f["margins"][:, m["tie"]] <= 1e-40) and np.all(f["skipped"] == 0)
    PF = iao.herm_unpack(f["cand_PF"])
    assert np.array_equal(PF[:, 0], np.conj(PF[:, 1]))
    assert np.array_equal(f["cand_capacity"][:, 0], f["cand_capacity"][:, 1])
    for name in ("diagonal-closed_form", "singular-closed_form"):
        assert np.all(fx[name]["skipped"] == 1) and np.all(o.may_skip(fx[name])), name
    assert np.all(fx["diagonal-closed_form"]["margins"][:, m["feasible"]] == 0)
    assert np.all(fx["singular-closed_form"]["margins"][:, m["cond"]] > 1e40)
    for g in (1e-3, 1e-6, 1e-9):
        gap = fx["near_repeated%g-closed_form" % g]["margins"][:, m["gap"]]
        assert np.all(np.abs(gap / g - 1) <= 2e-3), (g, gap)           # (the one rounding of H21 moves a 1e-9 gap by ~1e-7 of it)
    for cond in (1e2, 1e4, 1e6, 1e8, 1e10):
        got = fx["graded%g-closed_form" % cond]["margins"][:, m["cond"]]
        assert np.all(np.abs(got / cond - 1) <= 1e-5) and np.all(fx["graded%g-closed_form" % cond]["skipped"] == 0)
    for name in ("cross_identity-closed_form", "cross_equal-closed_form"):
        assert np.all(fx[name]["margins"][:, m["gap"]] == np.inf), name   # E = I: the canonical basis, no comparison
        F = o.cplx(fx[name]["cand_F"])
        assert np.array_equal(F[:, 0, 0], np.tile([1, 0], (3, 1))) and np.array_equal(F[:, 1, 0], np.tile([0, 1], (3, 1)))
    # no realization outside diagonal / singular may be flagged by the kernel
    for c in o.CASES:
        if c["cls"] not in ("diagonal", "singular") or c["solver"] != "closed_form":
            assert not np.any(o.may_skip(fx[c["name"]])) or c["cls"] == "graded", c["name"]


def test_orth_start_meets_a_scalar_covariance():
    """The first interference covariance at receiver 1 is I / 2 exactly, in f64."""
    c = o.CASE_BY_NAME["orth_start-min_leakage-fix-rel0-it8"]
    for r in range(3):
        big_H, F = o.draw(c, r)
        H = oia.split_blocks(big_H, 3, 2, 2)
        a, b = H[0][1] @ F[1], H[0][2] @ F[2]
        assert np.array_equal(np.outer(a, a.conj()) + np.outer(b, b.conj()), 0.5 * np.eye(2))
        assert np.allclose(np.linalg.norm(F, axis=1), 1.0, atol=1e-15)


def test_mmse_mu_beats_the_secant():
    """The mp MMSE precoder meets |V|^2 = 1 to 40 digits where mu > 0; oracle/ia.py's secant stops at 1.5e-8."""
    import mpmath as mp
    rs = np.random.RandomState(5)
    a = iao.to_mp(iao.randn_c(rs, 2, 2))
    A, b = a * a.H, iao.to_mp(iao.randn_c(rs, 2, 1)) * 3
    rec = {k: [] for k in o.MARGINS}
    v = o._mmse_precoder(A, b, rec)
    assert rec["mu0"][0] > 1 and abs(o._norm(v) ** 2 - 1) <= mp.mpf(10) ** -40
    v0 = o._mmse_precoder(A, b / 100, rec)                       # the mu = 0 branch: V = A^-1 b
    assert o._norm(v0) < 1 and o._norm(A * v0 - b / 100) <= mp.mpf(10) ** -45
    sing = iao.to_mp(np.array([[1.0, 0.0], [0.0, 1e-6]]))         # smax / smin = 1e6 > 5e4: loaded by mean / 100
    v1 = o._mmse_precoder(sing, iao.to_mp(np.array([[1e-3], [1e-3]])), rec)
    load = (1 + 1e-6) / 200
    assert abs(complex(v1[1, 0]) - 1e-3 / (1e-6 + load)) <= 1e-12
