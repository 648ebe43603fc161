"""GPU: the whole argument envelope of Engine.ia_solve_general (csrc/kernels_ia_general.hip) against the 50-digit reference
of tests/ia_general_oracle.py (tests/golden/g7_ia_envelope.npz): K = 2, 3 and 4, both capacities, Nt > Nr and Nr > Nt,
per-user stream counts, the three algorithms, both starts, the selection wrappers, noise_var = 0, scaled channels,
ragged batches, and every argument the C entry point refuses.

The strict bound of a case and quantity is 16 x max(e_np, kappa x 2^-52) at the case's worst realization: the error of
the f64 NumPy oracle against the mp result and the conditioning of the answer, never anything the kernel produced.
DESIGN.md (section "IA envelope") holds the kernel's measured error next to every bound; each test prints both."""
import itertools

import numpy as np
import pytest

import ia_general_oracle as iao
from oracle import ia as oia

pytestmark = pytest.mark.gpu

STRICT = [c["name"] for c in iao.CASES if c["kind"] in ("strict", "select")]
EVERY = [c["name"] for c in iao.CASES]
LEAKAGE = [c["name"] for c in iao.CASES if c["algo"] != "max_sinr" and not c["select"] and c["rel"] == 0.0]


def _D(case):
    return 4 if max(case["nr"], case["nt"]) <= 4 else 6


def _inputs(case, n=None):
    reals = [iao.draw(case, r) for r in range(case["n_real"] if n is None else n)]
    H = np.stack([h for h, _ in reals])
    F0 = np.stack([iao.pad_F(f, _D(case)) for _, f in reals])
    return H, F0


def _solve(engine, case, H, F0, **over):
    kw = dict(max_iterations=case["max_iterations"], relative_factor=case["rel"], noise_var=case["noise_var"])
    kw.update(over)
    fix = case["init"] == "fix" and case["select"] != "brute"
    return engine.ia_solve_general(case["algo"], H, case["K"], case["nr"], case["nt"], case["Ns"], kw["noise_var"],
                                   kw["max_iterations"], kw["relative_factor"], F_init=F0 if fix else None,
                                   select=case["select"])


def _unpad(case, sol, i):
    ns = [int(n) for n in sol["Ns"][i]]
    F = [np.asarray(sol["F"][i][k][:case["nt"], :ns[k]]) for k in range(case["K"])]
    U = [np.asarray(sol["U"][i][k][:ns[k], :case["nr"]]) for k in range(case["K"])]
    return ns, F, U


def _summary(case, sol, i):
    ns, F, U = _unpad(case, sol, i)
    out = dict(PF=np.stack([f @ f.conj().T for f in F]), PU=np.stack([u.conj().T @ u for u in U]),
               sinr=np.asarray(sol["sinr"][i][:, :max(case["nr"], case["nt"])]), capacity=float(sol["capacity"][i]))
    if "every_capacity" in sol:
        out["every_capacity"] = np.asarray(sol["every_capacity"][i])
    return out


def _want(fx, i):
    out = dict(PF=iao.herm_unpack(fx["PF"][i]), PU=iao.herm_unpack(fx["PU"][i]), sinr=fx["sinr"][i],
               capacity=float(fx["capacity"][i]))
    if "every_capacity" in fx:
        out["every_capacity"] = fx["every_capacity"][i]
    return out


def _strict_compare(case, fx, sol, tag="", quantities=None):
    """Ns, skipped, iterations equal; every quantity within the case's bound.  Prints measured error and bound."""
    bound = iao.bounds(case, fx)
    worst = np.zeros(len(bound))
    for i in range(case["n_real"]):
        worst = np.maximum(worst, iao.errors(_summary(case, sol, i), _want(fx, i)))
    names = iao.QUANTITIES + (("every_capacity",) if len(bound) > len(iao.QUANTITIES) else ())
    print("ENVELOPE %s%s iterations %s/%s %s" % (case["name"], tag, sol["iterations"].tolist(), fx["iterations"].astype(int).tolist(),
                                                " ".join("%s %.2e/%.2e" % (q, e, b) for q, e, b in zip(names, worst, bound))))
    for i in range(case["n_real"]):
        assert int(sol["skipped"][i]) == 0
        assert [int(n) for n in sol["Ns"][i]] == [int(n) for n in fx["Ns_final"][i]]
        if iao.iterations_pinned(fx):
            assert int(sol["iterations"][i]) == int(fx["iterations"][i])
    for q, e, b in zip(names, worst, bound):
        if quantities is None or q in quantities:
            assert e <= b, (case["name"], q, e, b)


@pytest.mark.parametrize("name", STRICT)
def test_strict_against_mp(engine, name):
    """Among them the cases that need the precoder read from the stacked factor (hsvd_right) and not from the formed
    matrix: alt-min and min-leakage with a two-stream user, run until the leakage is below the rounding noise of that
    matrix.  With the formed matrix the kernel ran 80 iterations at (4,4,4,(2,1,1,1)) where mp stops after 45, 44 and 72,
    and missed the capacity at (3,5,4,2) by 4.7e-2 against 2.6e-2; oracle.ia still does (its e_np is the bound there)."""
    case, fx = iao.CASE_BY_NAME[name], iao.load_fixture()[name]
    assert iao.is_strict(fx)
    H, F0 = _inputs(case)
    sol = _solve(engine, case, H, F0)
    if case["select"] == "brute":
        assert sol["every_capacity"].shape[1] == int(np.prod(case["Ns"])) == fx["every_capacity"].shape[1]
        assert len(list(itertools.product(*[range(1, n + 1) for n in case["Ns"]]))) == sol["every_capacity"].shape[1]
    _strict_compare(case, fx, sol)


@pytest.mark.parametrize("name", EVERY)
def test_self_consistency(engine, name):
    """What holds whether or not the answer is unique: unit-norm precoders, zero forcing of the own streams, the SINRs and
    the capacity of the kernel's own F and U, everything finite."""
    case = iao.CASE_BY_NAME[name]
    H, F0 = _inputs(case)
    sol = _solve(engine, case, H, F0)
    for v in sol.values():
        assert np.all(np.isfinite(v))
    K, nr, nt = case["K"], case["nr"], case["nt"]
    for i in range(case["n_real"]):
        assert int(sol["skipped"][i]) == 0
        ns, F, U = _unpad(case, sol, i)
        Hb = oia.split_blocks(H[i], K, nr, nt)
        want = oia.calc_SINR(Hb, F, U, case["noise_var"])
        for k in range(K):
            assert abs(np.linalg.norm(F[k], "fro") - 1.0) <= 1e-14
            assert np.max(np.abs(U[k] @ Hb[k][k] @ F[k] - np.eye(ns[k]))) <= 1e-8
            assert iao.relmax(sol["sinr"][i][k][:ns[k]], want[k]) <= 1e-9
            assert np.all(sol["sinr"][i][k][ns[k]:] == 0)
        cap = float(sum(np.sum(np.log2(1 + s)) for s in want))
        assert abs(sol["capacity"][i] - cap) <= 1e-9 * cap


@pytest.mark.parametrize("name", LEAKAGE)
def test_leakage_never_rises(engine, name):
    """alt-min and min-leakage minimise the same leakage in turn: cost_{n+1} <= cost_n + 1e-12 |big_H|_F^2 over
    max_iterations = 1, 2, 3, 5, 8 from the same start, and in the slack set (spare receive dimensions) every cost is
    zero to that accuracy.  A Jacobi that returns a wrong vector from a repeated eigenvalue fails here."""
    case = iao.CASE_BY_NAME[name]
    H, F0 = _inputs(case)
    costs = []
    for n in (1, 2, 3, 5, 8):
        sol = _solve(engine, case, H, F0, max_iterations=n, relative_factor=0.0)
        costs.append([iao.cost(H[i], _unpad(case, sol, i)[1], case["Ns"])
                      for i in range(case["n_real"])])
    costs = np.array(costs)
    tol = 1e-12 * np.array([np.linalg.norm(h, "fro") ** 2 for h in H])
    print("LEAKAGE %s max rise %.2e max cost %.2e tol %.2e" % (name, np.max(costs[1:] - costs[:-1]), costs.max(), tol.min()))
    assert np.all(costs[1:] <= costs[:-1] + tol)
    if case["kind"] == "slack":
        assert np.all(costs <= tol)


def test_brute_force_limit(engine):
    """256 combinations run (the fixture's K = 4, 4x4, Ns = 4 case above); 320 are refused before anything is launched."""
    case = iao.CASE_BY_NAME[[n for n in STRICT if "brute" in n][0]]
    H, F0 = _inputs(case)
    _solve(engine, case, H, F0)
    assert engine.last_kernel().startswith("ia_general<4> K=4")
    rs = np.random.RandomState(5)
    big = iao.randn_c(rs, 24, 24)
    with pytest.raises(ValueError, match="320 stream combinations"):
        engine.ia_solve_general("max_sinr", big, 4, 6, 6, (5, 4, 4, 4), 0.01, 1, 1e-6, select="brute")
    assert engine.last_kernel() == ""
    out = engine.ia_solve_general("max_sinr", big, 4, 6, 6, (4, 4, 4, 4), 0.01, 1, 1e-6, select="brute")
    assert out["every_capacity"].shape == (1, 256) and np.all(np.isfinite(out["every_capacity"]))
    assert engine.last_kernel() == "ia_general<6> K=4 6x6"


@pytest.mark.parametrize("which", [0, 1])
def test_batches_equal_single_calls(engine, which):
    """130 distinct problems whose lanes stop at different iterations: batches of 1, 63, 64, 65 and 130 are bit-equal to
    the same problems solved one per call (ragged tail, second block, divergence inside a wave)."""
    case = iao.BATCH_CASES[which]
    H, F0 = _inputs(case)
    single = [_solve(engine, case, H[i:i + 1], F0[i:i + 1]) for i in range(case["n_real"])]
    single = {k: np.concatenate([s[k] for s in single]) for k in single[0]}
    if which == 0:       # (tests/test_ia_general_envelope_cpu.py shows the same of the oracle's counts)
        assert len(set(single["iterations"][:64].tolist())) >= 3
    assert np.all(single["skipped"] == 0)
    for n in (1, 63, 64, 65, 130):
        got = _solve(engine, case, H[:n], F0[:n])
        for k, v in got.items():
            assert v.shape[0] == n
            assert v.tobytes() == np.ascontiguousarray(single[k][:n]).tobytes(), (n, k)


SCALED = [n for n in STRICT if ("K4-3x3" in n or "K3-5x3" in n) and "rel1e-06" in n]


@pytest.mark.parametrize("alpha", [2.0 ** -40, 2.0 ** 20, 1e-6])
@pytest.mark.parametrize("name", SCALED)
def test_scaled_channel(engine, name, alpha):
    """H -> alpha H with noise_var -> alpha^2 noise_var is the same problem (a path loss): the same decisions, and F F^H,
    SINRs and capacity within the strict bound of the unscaled case.  (heig and solve hold absolute thresholds.)"""
    case, fx = iao.CASE_BY_NAME[name], iao.load_fixture()[name]
    H, F0 = _inputs(case)
    sol = _solve(engine, case, alpha * H, F0, noise_var=alpha * alpha * case["noise_var"])
    _strict_compare(case, fx, sol, " alpha=%g" % alpha, ("capacity", "sinr", "PF"))
    if alpha in (2.0 ** -40, 2.0 ** 20):
        base = _solve(engine, case, H, F0)
        same = all(np.array_equal(sol[k], base[k]) for k in ("F", "sinr", "capacity", "iterations", "Ns"))
        print("SCALE %s alpha=%g bit-equal to the unscaled run: %s" % (name, alpha, same))


def test_zero_noise_rank_deficient(engine):
    """noise_var = 0 at K = 3, 4x4, one stream: the max-SINR matrix B has rank 2 in 4 dimensions.  Every output is finite
    or the realization is flagged; never a NaN that passes as a result."""
    case = dict(iao.CASE_BY_NAME["strict-max_sinr-K4-4x4-Ns1111-fix-rel0-it8"], K=3, Ns=[1, 1, 1], n_real=40, noise_var=0.0,
                seed=4411)
    H, F0 = _inputs(case)
    sol = _solve(engine, case, H, F0)
    flagged = sol["skipped"] != 0
    print("ZERO-NOISE flagged %d of %d, capacity %.3g .. %.3g" % (flagged.sum(), flagged.size,
                                                                 np.nanmin(sol["capacity"]), np.nanmax(sol["capacity"])))
    for k in ("F", "U", "sinr", "capacity"):
        v = sol[k].reshape(flagged.size, -1)
        assert np.all(np.isfinite(v[~flagged])), k


def test_envelope_errors(engine):
    """Every argument outside the envelope is refused through the engine, and nothing is launched."""
    rs = np.random.RandomState(3)
    good = iao.randn_c(rs, 9, 9)
    engine.ia_solve_general("max_sinr", good, 3, 3, 3, 1, 0.01, 2, 0.0)
    assert engine.last_kernel() == "ia_general<4> K=3 3x3"

    def refused(match, *a, **kw):
        with pytest.raises(ValueError, match=match):
            engine.ia_solve_general(*a, **kw)
        assert engine.last_kernel() == ""

    refused(r"K must be in \[2, 4\]", "max_sinr", iao.randn_c(rs, 2, 2), 1, 2, 2, 1, 0.01)
    refused(r"K must be in \[2, 4\]", "max_sinr", iao.randn_c(rs, 10, 10), 5, 2, 2, 1, 0.01)
    refused(r"\[1, 6\]", "max_sinr", iao.randn_c(rs, 21, 9), 3, 7, 3, 1, 0.01, F_init=np.zeros((1, 4, 6, 6)))
    refused(r"\[1, 6\]", "max_sinr", iao.randn_c(rs, 9, 21), 3, 3, 7, 1, 0.01, F_init=np.zeros((1, 4, 6, 6)))
    refused("Ns", "max_sinr", good, 3, 3, 3, 0, 0.01)
    refused("Ns", "max_sinr", good, 3, 3, 3, (1, 4, 1), 0.01)
    refused("Ns", "max_sinr", iao.randn_c(rs, 6, 12), 3, 2, 4, 3, 0.01, F_init=np.zeros((1, 4, 4, 4)))
    refused("svd", "max_sinr", iao.randn_c(rs, 6, 12), 3, 2, 4, 1, 0.01)
    refused("svd", "max_sinr", iao.randn_c(rs, 6, 12), 3, 2, 4, 1, 0.01, select="brute")     # brute force starts from 'svd'
    refused("bad solver settings", "max_sinr", good, 3, 3, 3, 1, 0.01, 0)
    refused("bad solver settings", "max_sinr", good, 3, 3, 3, 1, -0.01)
    refused("bad solver settings", "max_sinr", good, 3, 3, 3, 1, 0.01, 5, -1e-6)
    with pytest.raises(ValueError, match="F_init must be"):
        engine.ia_solve_general("max_sinr", good, 3, 3, 3, 1, 0.01, F_init=np.zeros((1, 3, 6, 6)))
    with pytest.raises(ValueError, match="one value per user"):
        engine.ia_solve_general("max_sinr", good, 3, 3, 3, (1, 1), 0.01)


def test_F_init_padding(engine):
    """A K-user start is padded to the 4 users and the D = 6 capacity of the library: [b, K, nt, ns], [b, K, 6, 6] and
    [b, 4, 6, 6] give the same bits."""
    case = iao.CASE_BY_NAME["strict-min_leakage-K3-5x4-Ns222-fix-rel0-it8"]
    H, F0 = _inputs(case)
    assert F0.shape[1:] == (4, 6, 6)
    full = _solve(engine, case, H, F0)
    for small in (F0[:, :3], F0[:, :3, :4, :2], F0[:, :, :4, :2]):
        got = engine.ia_solve_general(case["algo"], H, 3, 5, 4, case["Ns"], case["noise_var"], 8, 0.0,
                                      F_init=np.ascontiguousarray(small))
        for k in full:
            assert np.array_equal(full[k], got[k]), k
