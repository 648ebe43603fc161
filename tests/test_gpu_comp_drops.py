"""GPU: the CoMP link fed per-repetition user drops (csrc/pipeline_hex.hip -> csrc/pipeline_comp.hip) -- the resident path-loss
records of Engine.run_hex_drops as mcle_run_comp's d_pathloss, and simulators.CompSimulator's user_positioning_method, at
K = 3, 2 x 2 antennas, 50 symbols, 64 repetitions.  Everything here is an identity: the records either stay on the device or
make the round trip through the host, and the link must not notice."""
import numpy as np
import pytest

import hex_oracle as ho
from pyphysim_amd import modulators, pathloss
from pyphysim_amd.simulators import CompSimulator

pytestmark = pytest.mark.gpu

K, R, E, NS, REPS = 3, 2, 1, 50, 64
VARIANTS = ("None", "capacity")
SIM = dict(SNR=[10.0], Pe_dBm=[-60.0], modulator="psk", M=4, K=K, Nr=R, ext_int_rank=E, NSymbs=NS, packet_length=20,
           variants=VARIANTS, rep_max=REPS, seed=5, dtype="f64")


def sim_state(sim):
    return {name: [(r._value, r._total, r._result_sum, r._result_squared_sum, r.num_updates) for r in results]
            for name, results in ((n, sim.results[n]) for n in sim.results.get_result_names()) if name != "elapsed_time"}


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_resident_records_equal_their_host_copy(engine, dtype):
    modulators.PSK(4, engine=engine)._bind()
    out = engine.run_hex_drops(K, 1.0, 1, seed=77, first=3, count=REPS, n_ext=E, dtype=dtype, records=True)
    rec = out["records"]
    assert tuple(rec.shape) == (REPS, K, K + E) and not out["flags"].any()
    host = rec.get()
    assert np.all((host > 0) & (host <= 1.0)) and np.array_equal(host[..., :K].argmax(axis=2), np.tile(np.arange(K), (REPS, 1)))
    for variant in VARIANTS:
        args = (K, R, E, NS, 2.0e-3, 2.3e-15, 1.0e-9, 77, 3, REPS)
        kw = dict(variant=variant, packet_length=20, dtype=dtype, per_realization=True)
        res_d, arr_d = engine.run_comp(*args, pathloss_per_realization=rec, **kw)
        res_h, arr_h = engine.run_comp(*args, pathloss_per_realization=host, **kw)
        assert res_d == res_h and res_d["n_realizations"] == REPS
        for name in arr_d:
            assert np.array_equal(arr_d[name], arr_h[name]), (variant, name)
    # the path loss matters: the same call without it counts differently
    _, arr_0 = engine.run_comp(*args, **kw)
    assert not np.array_equal(arr_0["sinr"], arr_d["sinr"])


def test_random_positioning_equals_the_callable_on_the_same_records(engine):
    rand = CompSimulator(user_positioning_method="Random", batch_size=64, engine=engine, **SIM)
    rand.simulate()
    assert rand.runned_reps == [REPS]
    params = rand.params.get_unpacked_params_list()[0]
    calls = []

    def records(first, count):
        calls.append((first, count))
        return rand.drop_records(engine, params, first, count).get()

    host = CompSimulator(pathloss=records, batch_size=64, engine=engine, **SIM)
    host.simulate()
    assert calls == [(0, REPS)] and host.path_loss_border == rand.path_loss_border
    want = sim_state(host)
    assert sim_state(rand) == want and set(want) >= {"ber_None", "ser_capacity", "sinr_None", "spec_effic_capacity"}
    small = CompSimulator(user_positioning_method="Random", batch_size=16, engine=engine, **SIM)
    small.simulate()
    got = sim_state(small)
    for name in want:                      # sums over batches are formed in another order: the counts exactly, the sums to 1e-12
        for a, b in zip(got[name], want[name]):
            assert a[1] == b[1] and a[4] == b[4] and a == pytest.approx(b, rel=1e-12), name
    for name in ("ber_None", "ser_None", "ber_capacity", "ser_capacity"):
        assert [a[:2] for a in got[name]] == [b[:2] for b in want[name]], name


def test_symmetric_far_away_equals_the_fixed_matrix(engine):
    fx = ho.load_fixture()
    pl, plint = fx["border_app_pl3gpp"], fx["border_app_plint3gpp"]
    far = CompSimulator(user_positioning_method="Symmetric Far Away", batch_size=64, engine=engine, **SIM)
    assert np.max(np.abs(far._pl - pl) / pl) <= 1e-12 and np.max(np.abs(far._ple[:, 0] - plint) / plint) <= 1e-12
    far.simulate()
    fixed = CompSimulator(pathloss=pl, pathloss_ext=plint[:, None], batch_size=64, engine=engine,
                          path_loss_border=pathloss.PathLoss3GPP1().calc_path_loss(1.0), **SIM)
    fixed.simulate()
    a, b = sim_state(far), sim_state(fixed)
    for name in b:
        for x, y in zip(a[name], b[name]):
            assert x[1] == y[1] and x[4] == y[4] and x == pytest.approx(y, rel=1e-9), name
    for name in ("ber_None", "ser_None"):
        assert [x[:2] for x in a[name]] == [y[:2] for y in b[name]], name
