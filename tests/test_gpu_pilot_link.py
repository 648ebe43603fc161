"""GPU: the flat Blast link with pilot-estimated and with perfect channel state (csrc/pipeline_mimo_pilot.hip:
mcle_run_mimo_pilot_link) against the NumPy restatement under common random numbers (tests/pilot_link_oracle.py, the draw ledger of
DESIGN section 4).  tests/test_pilot_link_oracle_cpu.py (no GPU) holds the conditions that make "exactly" a fair demand: every
realization's smallest decision gap is >= 1e-9 (1.25e-6 on these cases), the estimate by a second route moves no est by more than
1e-3 of it (2.3e-13), and estimated and perfect CSI give other counts, so a kernel that used H twice cannot pass.

complex128: per-realization symbol and bit error counts of BOTH counter blocks equal to the restatement; complex64: the rule
helpers.check applies to the flat pipeline.  |H^ - H|^2 and |H|^2 are formed in the f64 set-up kernel in either arithmetic and
held element-wise at 1e-11 relative, the f64 bar of tests/test_gpu_pilot_mse.py."""
import numpy as np
import pytest

import estimators_oracle as eo
import pilot_link_oracle as po
from helpers import check
from pyphysim_amd import _lib
from pyphysim_amd._lib import McleError
from pyphysim_amd.simulators import PilotMimoSimulator

pytestmark = pytest.mark.gpu
DTYPES = [("f64", True), ("f32", False)]
TOL = 1e-11


def run(engine, cfg, first, count, dtype, seed=None, method=_lib.DEMOD_MINDIST, **kw):
    engine.set_constellation(po.table(), _lib.CONST_QAM)
    args = dict(pilot_power=cfg["pilot_power"], alpha=cfg["alpha"], pilots=cfg["pilots"], chan_factor=cfg["L"], cov=cfg["cov"],
                estimator=cfg["estimator"], mmse=cfg["mmse"], method=method, dtype=dtype, per_realization=True)
    args.update(kw)
    return engine.run_mimo_pilot_link(cfg["nt"], cfg["nr"], cfg["P"], cfg["n_symbols"], cfg["noise_var"],
                                      cfg["seed"] if seed is None else seed, first, count, **args)


def worst(got, want):
    return float(np.max(np.abs(got - want) / want))


def check_blocks(out, ref, exact, tag):
    c_est, c_perf, se, be, err, pw = out
    se, be = se.astype(np.int64), be.astype(np.int64)
    for b, cnt in enumerate((c_est, c_perf)):
        print("%s block %d: device %d / restatement %d symbol errors, %d / %d bit errors, largest difference in a realization %d"
              % (tag, b, se[b].sum(), ref["se"][b].sum(), be[b].sum(), ref["be"][b].sum(), np.max(np.abs(se[b] - ref["se"][b]))))
    errs = (worst(err, ref["err"]), worst(pw, ref["pow"]))
    print("%s err %.3g pow %.3g (element-wise relative)" % ((tag,) + errs))
    for b, cnt in enumerate((c_est, c_perf)):
        check(cnt, se[b], be[b], ref["se"][b], ref["be"][b], ref["n_symbols"], ref["n_bits"], exact)
    assert max(errs) <= TOL


@pytest.mark.parametrize("dt,exact", DTYPES)
@pytest.mark.parametrize("name", sorted(po.ALL_CASES))
def test_parity_under_common_random_numbers(engine, name, dt, exact):
    cfg, ref = po.ALL_CASES[name], po.reference(name)
    # (tests/test_gpu_pilot_mse.py guards its bar by err / pow > 1e-2, which no case of this link meets in every realization: the
    #  guard is the modelled rounding of err itself, test_pilot_link_oracle_cpu.py)
    assert po.err_rounding_bound(cfg, ref) <= 0.5 * TOL and ref["se"].max() > 0
    out = run(engine, cfg, po.FIRST, po.COUNT, dt)
    assert engine.last_kernel() == "mimo_pilot_link %s %s" % (dt, cfg["estimator"])
    check_blocks(out, ref, exact, "%s %s" % (name, dt))


@pytest.mark.parametrize("dt,exact", DTYPES)
@pytest.mark.parametrize("name", ["1x4-p3", "2x2-p2-dft", "3x4-p7", "4x4-p9", "4x4-p16"])
def test_perfect_csi_block_is_run_mimo_flat(engine, name, dt, exact):
    """L = I, alpha = 1: block 1 is mcle_run_mimo_flat('blast') on the same seed and range, realization by realization."""
    cfg = po.PARITY_CASES[name]
    c_est, c_perf, se, be, err, pw = run(engine, cfg, po.FIRST, po.COUNT, dt)
    flat, fse, fbe = engine.run_mimo_flat("blast", cfg["nt"], cfg["nr"], cfg["n_symbols"], cfg["noise_var"], po.SEED, po.FIRST,
                                          po.COUNT, mmse=cfg["mmse"], dtype=dt, per_realization=True)
    print(name, dt, "block 1 %d / run_mimo_flat %d symbol errors" % (c_perf["sym_errors"], flat["sym_errors"]))
    if exact:
        assert c_perf == flat and np.array_equal(se[1], fse) and np.array_equal(be[1], fbe)
    else:
        check(c_perf, se[1].astype(np.int64), be[1].astype(np.int64), fse.astype(np.int64), fbe.astype(np.int64),
              flat["n_symbols"], flat["n_bits"], False)


@pytest.mark.parametrize("dt,exact", DTYPES)
def test_noise_free_link_has_no_errors(engine, dt, exact):
    for name in ("3x4-p7", "2x2-p2-dft"):
        cfg = dict(po.PARITY_CASES[name], noise_var=0.0)
        c_est, c_perf, se, be, err, pw = run(engine, cfg, 0, 64, dt)
        w = float(np.max(err / pw))
        print(name, dt, "worst err / pow %.3g" % w)
        assert w <= TOL ** 2 and np.all(pw > 0)
        for cnt in (c_est, c_perf):
            assert cnt["n_realizations"] == 64 and cnt["n_skipped"] == 0 and cnt["sym_errors"] == 0 and cnt["bit_errors"] == 0
        assert not se.any() and not be.any()


@pytest.mark.parametrize("dt,exact", DTYPES)
def test_qam_slicer_gives_the_min_distance_counts(engine, dt, exact):
    name = "4x4-p9"
    cfg, ref = po.PARITY_CASES[name], po.reference(name)
    out = run(engine, cfg, po.FIRST, po.COUNT, dt, method=_lib.DEMOD_QAM_SLICER)
    check_blocks(out, ref, exact, "%s %s slicer" % (name, dt))
    if exact:
        md = run(engine, cfg, po.FIRST, po.COUNT, dt)
        assert out[0] == md[0] and out[1] == md[1] and np.array_equal(out[2], md[2]) and np.array_equal(out[3], md[3])


@pytest.mark.parametrize("dt,exact", DTYPES)
def test_split_invariance(engine, dt, exact):
    for name in ("2x3-p5", "mmse-est-1x4"):
        cfg = po.ALL_CASES[name]
        whole = run(engine, cfg, 3, 70, dt)
        a, b = run(engine, cfg, 3, 5, dt), run(engine, cfg, 8, 65, dt)
        for i in (2, 3):
            assert np.array_equal(np.concatenate([a[i], b[i]], axis=1), whole[i]), (name, i)
        for i in (4, 5):
            assert np.array_equal(np.concatenate([a[i], b[i]]), whole[i]), (name, i)
        for blk in (0, 1):
            for key in ("n_realizations", "sym_errors", "sym_errors_sq", "bit_errors", "bit_errors_sq"):
                assert a[blk][key] + b[blk][key] == whole[blk][key], (name, blk, key)


@pytest.mark.parametrize("dt,exact", DTYPES)
def test_grid_invariance_with_more_chunks_than_the_grid_holds(engine, dt, exact):
    """With grid_oversub = 1 the walk's grid is (2 complex128 | 3 complex64) workgroups of four wavefronts per compute unit and a
    wavefront takes 16 realizations a trip: `count` gives every wavefront two or three trips, and a single one with 8."""
    cfg = po.make_case(2, 2, 3, 2, 16.0, 1.5, True)
    per_trip = engine.n_cu * (2 if exact else 3) * 4 * 16
    count = 2 * per_trip + 37
    with engine.options(grid_oversub=1):
        one = run(engine, cfg, 0, count, dt)
    with engine.options(grid_oversub=8):
        eight = run(engine, cfg, 0, count, dt)
    assert one[0] == eight[0] and one[1] == eight[1]
    assert one[0]["n_realizations"] == count and one[0]["sym_errors"] > one[1]["sym_errors"] > 0
    for i in (2, 3, 4, 5):
        assert np.array_equal(one[i], eight[i]), i
    rows = [0, per_trip - 1, per_trip, 2 * per_trip + 5, count - 1]
    for r in rows:
        want = po.run(cfg, r, 1)
        if exact:
            assert np.array_equal(one[2][:, r], want["se"][:, 0]) and np.array_equal(one[3][:, r], want["be"][:, 0]), r
        assert worst(one[4][r:r + 1], want["err"]) <= TOL and worst(one[5][r:r + 1], want["pow"]) <= TOL, r


@pytest.mark.parametrize("dt,exact", DTYPES)
def test_realization_index_carries_past_two_to_the_32(engine, dt, exact):
    cfg = po.PARITY_CASES["2x3-p5"]
    first, count = 2 ** 32 - 5, 12
    ref = po.run(cfg, first, count)
    check_blocks(run(engine, cfg, first, count, dt), ref, exact, "2x3-p5 %s across 2^32" % dt)


def test_zero_realizations_return_zero_counters(engine):
    cfg = po.PARITY_CASES["2x3-p5"]
    run(engine, cfg, 0, 4, "f64")
    c_est, c_perf, se, be, err, pw = run(engine, cfg, 0, 0, "f64")
    assert se.shape == be.shape == (2, 0) and err.shape == pw.shape == (0,)
    assert not any(c_est.values()) and not any(c_perf.values()) and engine.last_kernel() == ""


@pytest.mark.parametrize("dt,exact", DTYPES)
def test_ledger_statistic_meets_the_exact_moments(engine, dt, exact):
    """Realizations 0 .. 4095 of seed 7: the mean LS error within 4 sigma of its exact value (estimators_oracle)."""
    mom = eo.default_cfg(nr=3, nt=1, n_pilots=10, pilot_power=1.5, noise_power=0.5)
    cfg = po.make_case(1, 3, 10, 2, 0.0, 1.5, noise_var=0.5)
    err = run(engine, cfg, 0, 4096, dt, seed=7)[4]
    mean, var = eo.ls_error_moments(mom)
    dev = (np.cumsum(err)[-1] / 4096 - mean) / np.sqrt(var / 4096)
    print(dt, "mean err %.6g exact %.6g deviation %+.2f sigma" % (err.mean(), mean, dev))
    assert abs(dev) <= 4.0


def test_more_pilots_cost_fewer_errors(engine):
    """The first parity case's settings over 20 000 realizations in complex64: with one pilot the estimated-CSI link makes at
    least the errors of the perfect-CSI one, and its errors fall as the pilots go 1, 4, 16, 64."""
    base = po.PARITY_CASES["1x1-p1"]
    errors = []
    for P in (1, 4, 16, 64):
        c_est, c_perf = run(engine, dict(base, P=P), 0, 20000, "f32", per_realization=False)
        print("P = %d: %d symbol errors with estimated CSI, %d with perfect CSI" % (P, c_est["sym_errors"], c_perf["sym_errors"]))
        assert c_est["n_realizations"] == c_perf["n_realizations"] == 20000
        errors.append((c_est["sym_errors"], c_perf["sym_errors"]))
    assert errors[0][0] >= errors[0][1] > 0
    assert len({e[1] for e in errors}) == 1                      # the perfect-CSI half does not see the pilots
    assert errors[0][0] > errors[1][0] > errors[2][0] > errors[3][0] >= errors[3][1]


def test_every_argument_rule_is_refused(engine):
    ok = po.PARITY_CASES["2x3-p5"]
    run(engine, ok, 0, 4, "f64")
    assert engine.last_kernel() == "mimo_pilot_link f64 ls"

    def refused(word, **kw):
        with pytest.raises((McleError, ValueError), match=word):
            run(engine, dict(ok, **kw), 0, 4, "f64")
        assert engine.last_kernel() == ""

    refused("nt <= nr", nt=3, nr=2)
    refused("nt <= nr", nr=5)
    refused("n_pilots must be", P=1)
    refused("n_pilots must be", P=257)
    refused("n_symbols", n_symbols=0)
    refused("needs nt = 1", estimator="mmse", cov=np.eye(3))
    refused("needs d_mmse_matrix", nt=1, estimator="mmse", cov=None)
    refused("pilot_power", pilot_power=0.0)
    refused("pilot_power", pilot_power=-1.0)
    refused("Noise variance", noise_var=-0.5)
    refused("alpha", alpha=float("nan"))
    refused(r"pilots must be \[nt, n_pilots\]", pilots=po.dft_pilots(2, 4, 1.0))
    refused(r"chan_factor must be", L=np.eye(2))
    with pytest.raises(ValueError, match="estimator must be"):
        run(engine, dict(ok, estimator="zf"), 0, 4, "f64")
    with pytest.raises((McleError, ValueError), match="at most 2\\^31-1"):
        engine.run_mimo_pilot_link(2, 3, 5, 51, 0.1, 1, 0, 2 ** 31)
    assert engine.last_kernel() == ""
    run(engine, ok, 0, 4, "f32")
    assert engine.last_kernel() == "mimo_pilot_link f32 ls"


def test_simulator_equals_the_engine_sums(engine):
    kw = dict(Nr=3, Nt=2, num_pilots=5, NSymbs=51, M=16, pilot_power=2.0, mmse=True, rep_max=512, seed=7, dtype="f64",
              engine=engine, common_random_numbers=True, demod="mindist")
    sim = PilotMimoSimulator([10.0, 16.0], batch_size=64, **kw)
    sim.simulate()
    names = {"ber", "ser", "ber_perfect_csi", "ser_perfect_csi", "mse", "channel_power", "elapsed_time"}
    assert set(sim.results.get_result_names()) >= names
    get = sim.results.get_result_values_list
    for i, snr in enumerate((10.0, 16.0)):
        engine.set_constellation(po.table(), _lib.CONST_QAM)
        c_est, c_perf, se, be, err, pw = engine.run_mimo_pilot_link(2, 3, 5, 51, 10.0 ** (-snr / 10.0), 7, 0, 512, pilot_power=2.0,
                                                                    mmse=True, dtype="f64", per_realization=True)
        assert get("ser")[i] == c_est["sym_errors"] / (512 * 102) and get("ber")[i] == c_est["bit_errors"] / (512 * 408)
        assert get("ser_perfect_csi")[i] == c_perf["sym_errors"] / (512 * 102)
        assert get("ber_perfect_csi")[i] == c_perf["bit_errors"] / (512 * 408)
        # (the simulator's sums are exact, the cumulative sum rounds at every addition)
        assert get("mse")[i] == pytest.approx(np.cumsum(err)[-1] / 512, rel=1e-13)
        assert get("channel_power")[i] == pytest.approx(np.cumsum(pw)[-1] / 512, rel=1e-13)
    assert get("ser")[0] > get("ser_perfect_csi")[0] > get("ser_perfect_csi")[1] and get("mse")[0] > get("mse")[1]
    big = PilotMimoSimulator([10.0, 16.0], batch_size=4096, **kw)            # one batch against eight
    big.simulate()
    for name in names - {"elapsed_time"}:
        assert big.results.get_result_values_list(name) == get(name), name


def test_simulator_with_the_mmse_estimator_and_fixed_pilots(engine):
    C = eo.toeplitz_cov(4, 0.9)
    sim = PilotMimoSimulator([12.0], Nr=4, Nt=1, num_pilots=6, NSymbs=20, M=16, alpha=0.7, C=C, estimator="mmse",
                             random_pilots=False, rep_max=256, seed=3, batch_size=100, dtype="f32", engine=engine)
    sim.simulate()
    assert engine.last_kernel() == "mimo_pilot_link f32 mmse"
    ser, perfect = sim.results.get_result_values_list("ser")[0], sim.results.get_result_values_list("ser_perfect_csi")[0]
    assert 0 < perfect <= ser < 0.5 and sim.results.get_result_values_list("mse")[0] > 0
    with pytest.raises(ValueError, match="Nt = 1"):
        PilotMimoSimulator([5.0], Nr=4, Nt=2, C=np.eye(4), estimator="mmse", engine=engine)
    with pytest.raises(ValueError, match="covariance"):
        PilotMimoSimulator([5.0], Nr=4, Nt=1, estimator="mmse", engine=engine)
