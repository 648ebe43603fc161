"""GPU: the fused estimation-error pipeline mcle_run_pilot_mse (csrc/kernels_estimators.hip) against the NumPy restatement
under common random numbers (tests/estimators_oracle.py, draw ledger of DESIGN section 4), the staged route through the
two operators, split and grid invariance, the ledger statistic against the exact moments, and the simulator on top."""
import numpy as np
import pytest

import estimators_oracle as eo
from pyphysim_amd.simulators import PilotEstimationSimulator

pytestmark = pytest.mark.gpu

TOL = {"f64": 1e-11, "f32": 2e-5}
SEED = 20261018


def run(engine, cfg, first, count, dtype, seed=SEED):
    return engine.run_pilot_mse(cfg["nr"], cfg["nt"], cfg["n_pilots"], cfg["noise_power"], seed, first, count,
                                pilot_power=cfg["pilot_power"], alpha=cfg["alpha"], pilots=cfg["pilots"],
                                chan_factor=cfg["L"], cov=cfg["cov"], dtype=dtype, per_realization=True)


def fixed_pilots(nt, P, power):
    return np.sqrt(power) * np.exp(2j * np.pi * np.random.RandomState(3).rand(nt, P))


C67 = eo.toeplitz_cov(67, 0.7)
PARITY = {
    "B": eo.ledger_case("B"),
    "nr67": eo.default_cfg(nr=67, nt=1, n_pilots=33, pilot_power=1.5, noise_power=0.5, alpha=0.7,
                           pilots=fixed_pilots(1, 33, 1.5), L=np.linalg.cholesky(C67), cov=0.49 * C67),
}


@pytest.fixture(scope="module")
def parity_want():
    """The restatement of the 32 parity realizations of both cases, computed once."""
    return {k: eo.pilot_mse(SEED, np.arange(32), cfg) for k, cfg in PARITY.items()}


def worst(got, want):
    return float(np.max(np.abs(got - want) / want))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_ls_recovers_the_channel_without_noise(engine, dtype):
    cfg = eo.default_cfg(nr=17, nt=3, n_pilots=7, noise_power=0.0, pilot_power=1.5, alpha=0.7)
    res, e_ls, e_mm, pw = run(engine, cfg, 0, 64, dtype)
    assert e_ls.shape == pw.shape == (64,) and e_mm is None and res["err_mmse"] is None and np.all(pw > 0)
    w = float(np.max(e_ls / pw))
    print(dtype, "worst err / pow %.3g" % w, engine.last_kernel())
    assert w <= TOL[dtype] ** 2
    assert engine.last_kernel() == "pilot_mse %s b4 ls" % dtype
    want = eo.pilot_mse(SEED, np.arange(64), cfg)
    assert worst(pw, want["pow"]) <= TOL[dtype]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("case", ["B", "nr67"])
def test_parity_under_common_random_numbers(engine, parity_want, case, dtype):
    want = parity_want[case]
    assert np.min(want["err_ls"] / want["pow"]) > 1e-2 and np.min(want["err_mmse"] / want["pow"]) > 1e-2
    res, e_ls, e_mm, pw = run(engine, PARITY[case], 0, 32, dtype)
    errs = [worst(e_ls, want["err_ls"]), worst(e_mm, want["err_mmse"]), worst(pw, want["pow"])]
    print(case, dtype, "err_ls %.3g err_mmse %.3g pow %.3g (element-wise relative)" % tuple(errs), engine.last_kernel())
    assert max(errs) <= TOL[dtype]
    assert engine.last_kernel() == "pilot_mse %s b16 ls+mmse gl" % dtype
    assert res["n_realizations"] == 32 and res["err_ls"] == np.cumsum(e_ls)[-1] and res["err_mmse"] == np.cumsum(e_mm)[-1]
    assert res["pow"] == np.cumsum(pw)[-1]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nt", [2, 3, 8])
def test_parity_of_the_ls_estimator_with_several_transmit_antennas(engine, nt, dtype):
    """nt = 2, 3, 8: 8, 4 and 2 realizations per wavefront, nt below and at its power of two; 13 realizations leave a tail."""
    cfg = eo.default_cfg(nr=5, nt=nt, n_pilots=11, noise_power=0.5, pilot_power=1.5, alpha=0.7)
    want = eo.pilot_mse(SEED, np.arange(13), cfg)
    res, e_ls, e_mm, pw = run(engine, cfg, 0, 13, dtype)
    errs = [worst(e_ls, want["err_ls"]), worst(pw, want["pow"])]
    print(nt, dtype, "err_ls %.3g pow %.3g" % tuple(errs), engine.last_kernel())
    assert max(errs) <= TOL[dtype]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("case", ["B", "nr67"])
def test_staged_route_meets_the_same_tolerances(engine, parity_want, case, dtype):
    """The restatement's Y through mcle_ls_estimate and mcle_mmse_estimate, errors formed on the host."""
    want, cfg = parity_want[case], PARITY[case]
    ls = engine.ls_estimate(want["Y"], want["s"], dtype=dtype).astype(np.complex128)
    mm = engine.mmse_estimate(want["Y"], want["s"], cfg["noise_power"], cfg["cov"], dtype=dtype).astype(np.complex128)
    e_ls = np.sum(np.abs(ls - want["h"]) ** 2, axis=(1, 2))
    e_mm = np.sum(np.abs(mm - want["h"]) ** 2, axis=(1, 2))
    errs = [worst(e_ls, want["err_ls"]), worst(e_mm, want["err_mmse"])]
    print(case, dtype, "staged err_ls %.3g err_mmse %.3g" % tuple(errs))
    assert max(errs) <= TOL[dtype]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_split_invariance(engine, dtype):
    for cfg in (PARITY["B"], eo.default_cfg(nr=5, nt=3, n_pilots=11)):
        _, e_ls, e_mm, pw = run(engine, cfg, 0, 32, dtype)
        a, b = run(engine, cfg, 0, 5, dtype), run(engine, cfg, 5, 27, dtype)
        for whole, i in ((e_ls, 1), (e_mm, 2), (pw, 3)):
            if whole is not None:
                assert np.array_equal(np.concatenate([a[i], b[i]]), whole), i


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_grid_invariance_with_more_realizations_than_the_grid_holds(engine, dtype):
    """At nr = 3 the launcher's grid is min(tiles, 8 x compute units x grid_oversub) one-wavefront workgroups of 16
    realizations a trip.  `count` makes every wavefront take two or three trips with grid_oversub = 1 (the planes of the
    previous tile reused, the masked tail in a later trip) and one with 8; all give the same arrays bit for bit."""
    cfg = eo.ledger_case("A")
    per_trip = 8 * engine.n_cu * 16
    count = 2 * per_trip + 37
    with engine.options(grid_oversub=1):
        _, e_ls, e_mm, pw = run(engine, cfg, 0, count, dtype)
    assert np.all(pw > 0) and np.all(e_ls > 0) and np.all(e_mm > 0)
    with engine.options(grid_oversub=8):
        _, l8, m8, p8 = run(engine, cfg, 0, count, dtype)
    assert np.array_equal(l8, e_ls) and np.array_equal(m8, e_mm) and np.array_equal(p8, pw)
    rows = np.array([0, per_trip - 1, per_trip, 2 * per_trip + 5, count - 1])
    want = eo.pilot_mse(SEED, rows, cfg)
    for got, key in ((e_ls, "err_ls"), (e_mm, "err_mmse"), (pw, "pow")):
        assert worst(got[rows], want[key]) <= TOL[dtype], key


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("case", ["A", "B"])
def test_ledger_statistic_meets_the_exact_moments(engine, case, dtype):
    """Realizations 0 .. 4095 of seed 7, the CPU test's bar on the GPU's sums: each mean within 4 sigma of its exact value."""
    cfg = eo.ledger_case(case)
    res, e_ls, e_mm, pw = run(engine, cfg, 0, 4096, dtype, seed=7)
    for key, (mean, var) in (("err_mmse", eo.mmse_error_moments(cfg)), ("err_ls", eo.ls_error_moments(cfg))):
        dev = (res[key] / 4096 - mean) / np.sqrt(var / 4096)
        print(case, dtype, key, "mean %.6g exact %.6g deviation %+.2f sigma" % (res[key] / 4096, mean, dev))
        assert abs(dev) <= 4.0, (case, key, dev)


def test_simulator_equals_the_engine_sums(engine):
    C0 = eo.toeplitz_cov(16, 0.9)
    kw = dict(Nr=16, Nt=1, num_pilots=8, pilot_power=1.5, alpha=0.7, C=C0, rep_max=512, seed=7, dtype="f64", engine=engine,
              common_random_numbers=True)
    sim = PilotEstimationSimulator([0.0, 10.0], batch_size=64, **kw)
    sim.simulate()
    assert set(sim.results.get_result_names()) >= {"mse_ls", "mse_mmse", "channel_power", "elapsed_time"}
    for i, snr in enumerate((0.0, 10.0)):
        res = engine.run_pilot_mse(16, 1, 8, 10.0 ** (-snr / 10.0), 7, 0, 512, pilot_power=1.5, alpha=0.7,
                                   chan_factor=np.linalg.cholesky(C0), cov=0.49 * C0, dtype="f64")
        # (the simulator's sums are exact, the engine's rounded at every addition)
        assert sim.results.get_result_values_list("mse_ls")[i] == pytest.approx(res["err_ls"] / (0.49 * 512), rel=1e-13)
        assert sim.results.get_result_values_list("mse_mmse")[i] == pytest.approx(res["err_mmse"] / 512, rel=1e-13)
        assert sim.results.get_result_values_list("channel_power")[i] == pytest.approx(res["pow"] / 512, rel=1e-13)
    ls, mm = sim.results.get_result_values_list("mse_ls"), sim.results.get_result_values_list("mse_mmse")
    assert ls[1] < ls[0] and mm[1] < mm[0] and mm[0] < 0.49 * ls[0]
    big = PilotEstimationSimulator([0.0, 10.0], batch_size=1024, **kw)       # one batch against eight
    big.simulate()
    for name in ("mse_ls", "mse_mmse", "channel_power"):
        assert big.results.get_result_values_list(name) == sim.results.get_result_values_list(name), name


def test_simulator_without_a_covariance_runs_ls_only(engine):
    sim = PilotEstimationSimulator([5.0], Nr=8, Nt=2, num_pilots=6, rep_max=256, seed=1, batch_size=100, dtype="f32",
                                   engine=engine, random_pilots=False)
    sim.simulate()
    names = set(sim.results.get_result_names())
    assert {"mse_ls", "channel_power"} <= names and "mse_mmse" not in names
    # orthogonal fixed pilots: E err_ls = nr nt noise_power / (P pilot_power); E pow = nr nt
    mse = sim.results.get_result_values_list("mse_ls")[0]
    want = 8 * 2 * 10.0 ** -0.5 / 6
    assert abs(mse - want) <= 6.0 * want / np.sqrt(16 * 256.0)
    with pytest.raises(ValueError, match="Nt = 1"):
        PilotEstimationSimulator([5.0], Nr=8, Nt=2, C=np.eye(8), engine=engine)


def test_every_argument_rule_is_refused(engine):
    ok = eo.ledger_case("A")

    def refused(word, dtype="f64", **kw):
        with pytest.raises(ValueError, match=word):
            run(engine, dict(ok, **kw), 0, 4, dtype)
        assert engine.last_kernel() == ""

    refused("needs nt = 1", nt=2)
    refused("at least nt", nt=8, n_pilots=7, cov=None)
    refused("nr must be", nr=129, cov=None)
    refused("nr must be", nr=0, cov=None)
    refused("nt must be", nt=9, n_pilots=16, cov=None)
    refused("at most 256", n_pilots=257)
    refused("noise_power", noise_power=-0.5)
    refused("pilot_power", pilot_power=0.0)
    refused("alpha", alpha=float("inf"))
    refused("cov holds", cov=np.full((3, 3), np.nan))
    refused("chan_factor holds", L=np.full((3, 3), np.inf))
    refused("singular", noise_power=0.0, cov=np.zeros((3, 3)))
    import ctypes
    from pyphysim_amd import _lib
    cfg = _lib.PilotMseCfg()
    cfg.nr, cfg.nt, cfg.n_pilots, cfg.random_pilots = 3, 1, 10, 0
    cfg.pilot_power, cfg.noise_power, cfg.alpha = 1.0, 0.5, 1.0
    out = engine.empty(4, np.float64)
    rc = engine.lib.mcle_run_pilot_mse(engine.ctx, _lib.MCLE_F64, ctypes.byref(cfg), 1, 0, 4, out.ptr, None, out.ptr)
    assert rc == -1 and "d_pilots" in engine.lib.mcle_last_error().decode() and engine.last_kernel() == ""
    res, e_ls, e_mm, pw = run(engine, ok, 0, 0, "f64")
    assert e_ls.shape == (0,) and res["n_realizations"] == 0 and engine.last_kernel() == ""
    res = run(engine, ok, 0, 4, "f64")[0]
    assert engine.last_kernel() == "pilot_mse f64 b16 ls+mmse"
