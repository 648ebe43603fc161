"""GPU: the fused estimation-error pipeline mcle_run_chanest (csrc/kernels_chanest.hip) against the NumPy restatement
under common random numbers (tests/chanest_oracle.py, draw ledger of DESIGN section 4), the staged route through
mcle_cazac_estimate, split invariance and the simulator on top."""
import numpy as np
import pytest

import chanest_oracle as co
from pyphysim_amd import reference_signals as rs
from pyphysim_amd.simulators import ChannelEstimationSimulator

pytestmark = pytest.mark.gpu

F64_TOL, F32_TOL = 1e-11, 2e-5
TOL = {"f64": F64_TOL, "f32": F32_TOL}
SEED = 20261018


def srs_users(root_index, ne, shifts):
    root = rs.RootSequence(root_index=root_index, size=ne)
    return np.stack([rs.SrsUeSequence(root, s).seq_array() for s in shifts])


def run(engine, cfg, first, count, dtype):
    return engine.run_chanest(cfg["ref_seqs"], cfg["n_rx"], cfg["num_taps_to_keep"], cfg["size_multiplier"], cfg["noise_var"],
                              cfg["tap_power"], cfg["tap_delay"], SEED, first, count, dtype=dtype, per_realization=True)


PROFILE = dict(tap_power=list(10.0 ** (np.array([0.0, -3.0, -6.0, -9.0]) / 10.0)), tap_delay=[0, 1, 2, 4])
PARITY = dict(ref_seqs=srs_users(25, 150, (0, 3, 6)), n_rx=4, size_multiplier=2, num_taps_to_keep=15, noise_var=0.1, **PROFILE)


@pytest.fixture(scope="module")
def parity_want():
    """The restatement of the 32 parity realizations, computed once."""
    both = [co.chanest_realization(SEED, r, PARITY) for r in range(32)]
    return np.array([b[0] for b in both]), np.array([b[1] for b in both])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_exact_recovery_without_noise(engine, dtype):
    """Shifts (0, 2, 5) move a user's taps by multiples of Ne / 8 = 6: no other user's tap falls into the window 0 .. 5."""
    cfg = dict(ref_seqs=srs_users(7, 48, (0, 2, 5)), n_rx=2, size_multiplier=2, num_taps_to_keep=5, noise_var=0.0, **PROFILE)
    res, err, pw = run(engine, cfg, 0, 64, dtype)
    assert err.shape == pw.shape == (64, 3) and np.all(pw > 0)
    worst = float(np.max(err / pw))
    print(dtype, "worst err / pow %.3g" % worst, engine.last_kernel())
    assert worst <= TOL[dtype] ** 2
    assert engine.last_kernel().startswith("chanest " + dtype)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_parity_under_common_random_numbers(engine, parity_want, dtype):
    want_err, want_pow = parity_want
    res, err, pw = run(engine, PARITY, 0, 32, dtype)
    e_err = float(np.max(np.abs(err - want_err) / want_err))             # per realization and user, relative to that entry
    e_pow = float(np.max(np.abs(pw - want_pow) / want_pow))
    print(dtype, "err %.3g pow %.3g (element-wise relative)" % (e_err, e_pow), "nmse", (err.sum(0) / pw.sum(0)).tolist())
    assert e_err <= TOL[dtype] and e_pow <= TOL[dtype]
    assert np.array_equal(res["err"], np.cumsum(err, axis=0)[-1]) and res["n_realizations"] == 32


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_staged_route_meets_the_same_tolerances(engine, parity_want, dtype):
    """The same draws formed on the host, mcle_cazac_estimate for every user, errors summed on the host."""
    want_err, want_pow = parity_want
    seqs = PARITY["ref_seqs"]
    H, Y = [], []
    for r in range(32):
        h, y = co.chanest_channels(*co.chanest_draws(SEED, r, PARITY), PARITY)
        H.append(h), Y.append(y)
    H, Y = np.array(H), np.array(Y)                                          # [32, 3, 4, 300], [32, 4, 150]
    err = np.empty((32, 3))
    for u in range(3):
        est = engine.cazac_estimate(seqs[u], Y, 15, size_multiplier=2, dtype=dtype)
        err[:, u] = (np.abs(est.astype(np.complex128) - H[:, u]) ** 2).sum((1, 2))
    e = float(np.max(np.abs(err - want_err) / want_err))
    print(dtype, "staged err %.3g (element-wise relative)" % e)
    assert e <= TOL[dtype]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_split_invariance(engine, dtype):
    _, err, pw = run(engine, PARITY, 0, 32, dtype)
    _, e1, p1 = run(engine, PARITY, 0, 5, dtype)
    _, e2, p2 = run(engine, PARITY, 5, 27, dtype)
    assert np.array_equal(np.concatenate([e1, e2]), err) and np.array_equal(np.concatenate([p1, p2]), pw)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_grid_invariance_with_more_realizations_than_the_grid_holds(engine, dtype):
    """The launcher's grid is min(workgroups needed, 2 x compute units x grid_oversub) workgroups of four wavefronts, one
    realization per wavefront and trip.  `count` is chosen from the device's compute units so that grid_oversub = 1 makes
    every wavefront take three or four trips of the grid-stride loop (LDS of the previous realization reused, the output
    rows of a later one written) while grid_oversub = 8 holds all of them in one trip; a split run shifts which wavefront
    gets which realization.  All three give the same arrays bit for bit, and the last rows equal the restatement."""
    cfg = dict(ref_seqs=srs_users(7, 48, (0, 2, 5)), n_rx=2, size_multiplier=2, num_taps_to_keep=5, noise_var=0.05, **PROFILE)
    per_trip = 2 * engine.n_cu * 4
    count = 3 * per_trip + 37
    with engine.options(grid_oversub=1):
        _, err, pw = run(engine, cfg, 0, count, dtype)
    assert count > per_trip and np.all(pw > 0) and np.all(err > 0)
    with engine.options(grid_oversub=8):
        _, e8, p8 = run(engine, cfg, 0, count, dtype)
    assert np.array_equal(e8, err) and np.array_equal(p8, pw)
    cut = per_trip + 3
    with engine.options(grid_oversub=1):
        _, e1, p1 = run(engine, cfg, 0, cut, dtype)
        _, e2, p2 = run(engine, cfg, cut, count - cut, dtype)
    assert np.array_equal(np.concatenate([e1, e2]), err) and np.array_equal(np.concatenate([p1, p2]), pw)
    for r in (0, per_trip - 1, per_trip, 2 * per_trip + 5, count - 1):          # first trip, both sides of a wrap, the tail
        want_err, want_pow = co.chanest_realization(SEED, r, cfg)
        assert np.max(np.abs(err[r] - want_err) / want_err) <= TOL[dtype], r
        assert np.max(np.abs(pw[r] - want_pow) / want_pow) <= TOL[dtype], r


def test_argument_rules(engine):
    bad = dict(PARITY, tap_delay=[0, 1, 2, 150])
    with pytest.raises(ValueError, match="tap delays"):
        run(engine, bad, 0, 4, "f64")
    with pytest.raises(ValueError, match="n_rx"):
        run(engine, dict(PARITY, n_rx=5), 0, 4, "f64")
    assert engine.last_kernel() == ""
    res, err, pw = run(engine, PARITY, 0, 0, "f64")
    assert err.shape == (0, 3) and res["n_realizations"] == 0


def test_simulator_equals_the_engine_sums(engine):
    sim = ChannelEstimationSimulator(SNR=[0.0, 10.0], n_users=3, shifts=(0, 3, 6), Ne=150, size_multiplier=2,
                                     num_taps_to_keep=15, Nr=4, root_index=25, rep_max=48, seed=3, batch_size=64,
                                     dtype="f64", engine=engine, common_random_numbers=True)
    sim.simulate()
    for i, snr in enumerate((0.0, 10.0)):
        res = engine.run_chanest(sim.ref_seqs, 4, 15, 2, 10.0 ** (-snr / 10.0), sim._tap_power, sim._tap_delay, 3, 0, 48,
                                 dtype="f64")
        for u in range(3):
            got = sim.results.get_result_values_list("nmse_user%d" % u)[i]
            assert got == res["err"][u] / res["pow"][u], (snr, u)
    nm = np.array([sim.results.get_result_values_list("nmse_user%d" % u) for u in range(3)])
    assert np.all(nm[:, 1] < nm[:, 0]) and np.all(nm > 0)
    assert len(sim.results.get_result_values_list("elapsed_time")) == 2
