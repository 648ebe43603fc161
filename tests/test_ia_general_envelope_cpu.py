"""CPU: the conditions under which tests/test_gpu_ia_general_envelope.py may compare the kernel tightly, shown from the
oracles alone (tests/golden/g7_ia_envelope.npz, tests/ia_general_oracle.py).  No GPU.

A strict case is one whose every realization has, in the 50-digit oracle, sensitivity <= 1e-8 under a 1e-14 relative
perturbation of the channel and every decision margin >= 1e-6; the slack set is shown to be the other population."""
import numpy as np
import pytest

import ia_general_oracle as iao

STRICT = [c for c in iao.CASES if c["kind"] in ("strict", "select")]
SLACK = [c for c in iao.CASES if c["kind"] == "slack"]


def test_fixture_covers_the_case_table():
    fx = iao.load_fixture()
    assert list(fx) == [c["name"] for c in iao.CASES]
    for c in iao.CASES:
        assert all(v.shape[0] == c["n_real"] for v in fx[c["name"]].values()), c["name"]
    assert len(STRICT) >= 9 * 3 * 2 + 6 * 3 + 7 * 2 + 5 + 3 and len(SLACK) == 14


def test_strict_condition():
    """No realization of a strict case left out; the bound that follows is orders below the old 1e-6."""
    fx = iao.load_fixture()
    worst_kappa, worst_margin, worst_bound = 0.0, np.inf, 0.0
    for c in STRICT:
        f = fx[c["name"]]
        assert np.all(np.isfinite(f["kappa"])) and np.all(np.isfinite(f["e_np"])), c["name"]
        assert np.all(f["kappa"] * iao.PERTURBATION <= iao.STRICT_SENSITIVITY), (c["name"], f["kappa"].max())
        assert np.all(f["margins"][:, :4] >= iao.STRICT_MARGIN), (c["name"], f["margins"].min(axis=0))
        assert iao.is_strict(f)
        worst_kappa = max(worst_kappa, float(f["kappa"].max()))
        worst_margin = min(worst_margin, float(f["margins"][:, :4].min()))
        worst_bound = max(worst_bound, float(iao.bounds(c, f).max()))
    print("strict set: kappa <= %.3g, margins >= %.3g, bounds <= %.3g" % (worst_kappa, worst_margin, worst_bound))


def test_bounds_are_orders_below_the_old_tolerance():
    """16 x max(e_np, kappa x 2^-52) <= 1e-10 against the 1e-6 of tests/test_gpu_ia_general.py -- except where the f64
    oracle itself loses the answer: alt-min and min-leakage with two streams per user, run until the leakage (the two
    smallest eigenvalues the precoder is read from) has sunk below the rounding noise of the matrix.  mp at 50 digits still
    resolves the pair; f64 keeps its span and loses the split between the two streams (and LAPACK's general `eig`, which
    the reference calls, stops returning orthogonal vectors).  There e_np makes the bound vacuous; what tests the kernel
    (which reads the precoder from the factor and keeps the split) is the iteration count, equal to mp's, and the leakage
    check of the GPU file.  The list is pinned so that no other case joins it unnoticed."""
    fx = iao.load_fixture()
    vacuous = []
    for c in STRICT:
        if iao.bounds(c, fx[c["name"]]).max() > 1e-10:
            vacuous.append(c["name"])
            assert c["algo"] in ("alt_min", "min_leakage") and max(c["Ns"]) > 1, c["name"]
    print("bound above 1e-10:", vacuous)
    assert len(vacuous) <= 10


def test_iteration_counts_pinned_except_finite_convergence():
    """rel = 0 stops on `dmax > 0`.  Where the iterate converges in finitely many steps (two users on 2x2 or four on 4x4
    with one stream: one update aligns exactly; Nt = 1: the precoder is a number of modulus 1) that is decided by the last
    bit, in any arithmetic, and the iteration count is not a property of the algorithm.  Such a case keeps every other
    comparison; it is recognised by its rel = 1e-6 twin stopping within three iterations."""
    fx = iao.load_fixture()
    loose = [c["name"] for c in STRICT if not iao.iterations_pinned(fx[c["name"]])]
    print("iteration count not pinned:", loose)
    for name in loose:
        c = iao.CASE_BY_NAME[name]
        assert c["rel"] == 0.0 and c["noise_var"] > 0 and not c["select"]
        twin = "strict-%s-K%d-%dx%d-Ns%s-fix-rel1e-06-it80" % (c["algo"], c["K"], c["nr"], c["nt"], "".join(map(str, c["Ns"])))
        assert fx[twin]["iterations"].max() <= 3, (name, fx[twin]["iterations"])
    assert len(loose) <= 20


def test_slack_set_is_the_other_population():
    """Spare receive dimensions: any basis of the null space is 'the' answer, and SINRs and capacity (in most shapes the
    precoders too) move by orders more than the strict set allows."""
    fx = iao.load_fixture()
    for c in SLACK:
        moved = fx[c["name"]]["kappa"].max() * iao.PERTURBATION
        assert moved >= 1e-4, (c["name"], moved)
        assert np.nanmax(np.abs(fx[c["name"]]["cost"][:, 1:])) <= 1e-30      # zero leakage from the first update on


@pytest.mark.parametrize("name", ["strict-%s-K2-2x2-Ns11-fix-rel0-it8" % a for a in iao.ALGOS]
                         + ["strict-%s-K4-2x2-Ns1111-fix-rel1e-06-it80" % a for a in iao.ALGOS])
def test_fixture_is_current(name):
    """(2,2,2,1) and (4,2,2,1) recomputed at 50 digits equal the stored values."""
    c, f = iao.CASE_BY_NAME[name], iao.load_fixture()[name]
    for r in range(c["n_real"]):
        got = iao.run_case(c, r)
        assert np.array_equal(iao.herm_pack(got["PF"]), f["PF"][r]) and np.array_equal(iao.herm_pack(got["PU"]), f["PU"][r])
        assert np.array_equal(got["sinr"], f["sinr"][r]) and got["capacity"] == f["capacity"][r]
        assert got["iterations"] == f["iterations"][r] and np.array_equal(got["Ns_final"], f["Ns_final"][r])
        assert np.array_equal(got["margins"], f["margins"][r])


@pytest.mark.parametrize("case", STRICT, ids=lambda c: c["name"])
def test_numpy_oracle_against_mp(case):
    """The f64 NumPy oracle on every strict case: the same decisions as the mp oracle, and the stored e_np."""
    f = iao.load_fixture()[case["name"]]
    for r in range(case["n_real"]):
        big_H, F_init = iao.draw(case, r)
        got = iao.numpy_solve(case, big_H, F_init)
        assert np.array_equal(got["Ns_final"], f["Ns_final"][r])
        if iao.iterations_pinned(f) and iao.bounds(case, f).max() <= 1e-10:   # (f64 has lost the iterate: see above)
            assert got["iterations"] == f["iterations"][r]
        want = dict(PF=iao.herm_unpack(f["PF"][r]), PU=iao.herm_unpack(f["PU"][r]), sinr=f["sinr"][r],
                    capacity=f["capacity"][r])
        if "every_capacity" in f:
            want["every_capacity"] = f["every_capacity"][r]
        e = iao.errors(got, want)
        # e_np is this very number on the machine that wrote the fixture; another LAPACK build may round differently
        assert np.all(e <= iao.bounds(case, f)), (e, f["e_np"][r])


def test_batch_problems_diverge():
    """The 130 problems of the batching test stop at three or more different iterations, so one wave truly diverges."""
    case = iao.BATCH_CASES[0]
    its = [iao.numpy_solve(case, *iao.draw(case, r))["iterations"] for r in range(case["n_real"])]
    assert len(set(its)) >= 3 and len(set(its[:64])) >= 3
    assert max(its) <= case["max_iterations"]


def test_cost_matches_in_both_arithmetics():
    case = iao.CASE_BY_NAME["strict-alt_min-K3-5x4-Ns222-fix-rel0-it8"]
    big_H, F = iao.draw(case, 0)
    a = iao.cost(big_H, F, case["Ns"])
    b = iao.cost(big_H, F, case["Ns"], use_mp=True)
    assert a > 0.1 and abs(a - b) <= 1e-13 * np.linalg.norm(big_H, "fro") ** 2
    assert abs(b - iao.load_fixture()[case["name"]]["cost"][0, 0]) <= 1e-15 * b


def test_hermitian_packing_round_trips():
    rs = np.random.RandomState(1)
    a, b = iao.randn_c(rs, 5, 5), iao.randn_c(rs, 5, 5)
    P = np.stack([a + a.conj().T, b + b.conj().T])
    assert np.array_equal(iao.herm_unpack(iao.herm_pack(P)), P)
