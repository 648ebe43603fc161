"""GPU: the indoor system-level kernels (csrc/pipeline_indoor.hip) -- the SINR heat-map operator mcle_indoor_sinr and the fused
user drops mcle_run_indoor_drops -- against the reference's own results (tests/golden/g8_metis.npz) and the NumPy restatement
tests/metis_oracle.py, in both arithmetics; and simulators.MetisDropSimulator on top of them.

Tolerances ("Indoor system level"): complex128's arithmetic (f64) holds the linear SINR and the capacity to 1e-12
relative.  For f32 the largest relative error of the linear SINR against the f64 oracle over the heat
maps, the injected drops and the Philox drops was measured (F32_MEASURED) and eight times it, rounded up to one
digit, is the bound: the factor covers a sum of up to 255 such terms in unspecified order and seeds not yet seen.
The association is exact against the fixture (its seeds leave a gap above 1e-3 between every user's two best gains); against
the restatement on Philox positions it is compared where the two best gains differ by more than TAU, and a drop with a user
inside the gap (or within 1e-9 side lengths of a room boundary) is left out whole when the unused APs are switched off, since
its loads may move -- at most 5 % of a case's drops."""
import functools

import numpy as np
import pytest

import metis_oracle as mo
from pyphysim_amd import metis, simulators

pytestmark = pytest.mark.gpu

F64_RTOL = 1e-12
F32_MEASURED = 3.09e-6       # largest relative error of the f32 linear SINR over tests 1, 3 and 4
F32_RTOL = 3e-5              # 8 x F32_MEASURED = 2.47e-5, rounded up to one digit
RTOL = {"f64": F64_RTOL, "f32": F32_RTOL}
TAU = {"f64": 1e-9, "f32": 4 * F32_RTOL}
HIST = dict(hist_bins=24, hist_lo_dB=-10.0, hist_step_dB=2.5)
DTYPES = ["f64", "f32"]


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(mo.load_fixture())


def relerr(got, want):
    want = np.asarray(want, dtype=float)
    return float(np.max(np.abs(np.asarray(got, dtype=float) - want) / np.abs(want)))


def lin(db):
    return 10.0 ** (np.asarray(db, dtype=float) / 10.0)


# ---- 1: the operator against the five heat maps ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", range(5))
def test_operator_against_the_heat_maps(engine, case, dtype):
    fx = fixture()
    row = fx["heat%d_cfg" % case]
    n, L = int(row[0]), float(row[2])
    pts = mo.heat_points(L, n)
    worst = 0.0
    for m, model in enumerate(mo.HEAT_MODELS):
        cfg = mo.cfg_from_row(row, assoc=0, **model)
        got = engine.indoor_sinr(pts, dtype=dtype, **mo.engine_kwargs(cfg))
        assert got.shape == (n, n, 15, 15)
        assert engine.last_kernel() == "indoor_sinr %s m%d a0" % (dtype, mo.MODEL_CODES[cfg["model"]])
        worst = max(worst, relerr(lin(got), lin(fx["heat%d_sinr" % case][m])))
    print("heat map %d %s: largest relative error of the linear SINR %.3g" % (case, dtype, worst))
    assert worst <= RTOL[dtype]
    if dtype == "f64":                 # the Python surface of the application returns the same four arrays
        scen = {"side_length": L, "single_wall_loss_dB": row[3], "num_rooms_per_side": n, "ap_decimation": int(row[1])}
        maps = metis.perform_simulation_SINR_heatmap(scen, {"Pt_dBm": row[4], "noise_power_dBm": row[5]}, engine=engine)
        assert len(maps) == 4 and relerr(lin(np.stack(maps)), lin(fx["heat%d_sinr" % case])) <= F64_RTOL


# ---- 2: chosen points -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("assoc", [0, 1])
def test_points_on_and_next_to_an_access_point(engine, assoc, dtype):
    """On the AP and 0.01 m / 0.0196 m from it the line-of-sight loss is clamped to 0 dB, at 0.0197 m it is not."""
    cfg = mo.base_cfg(12, 1, 10.0, assoc=assoc)
    ap = mo.rooms(10.0, 12)[5, 6]
    offsets = np.array([0.0, 0.01, 0.0196, 0.0197])
    pts = np.concatenate([ap + offsets, ap + 1j * offsets[1:], ap - offsets[1:] * (1 + 1j) / np.sqrt(2.0)])
    los_dB = mo.path_loss_dB(cfg, np.abs(pts - ap), np.zeros(pts.size, dtype=int))
    assert np.array_equal(los_dB[:4] > 0, [False, False, False, True]) and (los_dB > 0).sum() == 3
    want, want_assoc = mo.heat_map(cfg, pts)
    got, got_assoc = engine.indoor_sinr(pts, dtype=dtype, with_assoc=True, **mo.engine_kwargs(cfg))
    print("chosen points assoc %d %s: %.3g" % (assoc, dtype, relerr(lin(got), want)))
    assert np.array_equal(got_assoc, want_assoc) and np.all(got_assoc == 5 * 12 + 6)
    assert relerr(lin(got), want) <= RTOL[dtype]
    assert engine.last_kernel() == "indoor_sinr %s m2 a%d" % (dtype, assoc)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("assoc", [0, 1])
@pytest.mark.parametrize("model", range(4))
def test_exact_tie_takes_the_lowest_index(engine, model, assoc, dtype):
    """Two rooms per side, a checkerboard of two APs: the centre of room (0, 0) is exactly 10 m and one wall from both."""
    cfg = mo.base_cfg(2, 2, 10.0, assoc=assoc, **mo.HEAT_MODELS[model])
    pts = mo.rooms(10.0, 2)[[0, 1], [0, 1]]                   # both rooms without an AP
    g, d = mo.gains(cfg, pts)
    assert np.array_equal(d, [[10.0, 10.0], [10.0, 10.0]]) and np.array_equal(g[:, 0], g[:, 1])
    got, got_assoc = engine.indoor_sinr(pts, dtype=dtype, with_assoc=True, **mo.engine_kwargs(cfg))
    assert got_assoc.tolist() == [0, 0]
    assert relerr(lin(got), mo.heat_map(cfg, pts)[0]) <= RTOL[dtype]


# ---- 3: drops with injected positions against the reference -----------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", range(7))
def test_injected_drops_against_the_reference(engine, case, dtype):
    fx = fixture()
    row = fx["drop%d_cfg" % case]
    cfg = mo.cfg_from_row(row, assoc=1, active=1)
    U, drops = int(row[6]), int(row[7])
    pos = fx["drop%d_positions" % case]
    out = engine.run_indoor_drops(n_users=U, seed=1, first=0, count=drops, positions=pos, active=True, dtype=dtype,
                                  per_user=True, **mo.engine_kwargs(cfg))
    assert engine.last_kernel() == "indoor_drops %s m2 a1 t1 u%d" % (dtype, 1 if U <= 64 else 2 if U <= 128 else 4)
    assert np.array_equal(out["assoc"], fx["drop%d_assoc" % case])
    assert out["active_aps"].tolist() == [np.unique(a).size for a in fx["drop%d_assoc" % case]]
    e_sinr = relerr(lin(out["sinr_dB"]), lin(fx["drop%d_sinr_dB" % case]))
    e_cap = relerr(out["capacity"], fx["drop%d_capacity" % case])
    print("injected drops %d %s: SINR %.3g capacity %.3g" % (case, dtype, e_sinr, e_cap))
    assert e_sinr <= RTOL[dtype] and e_cap <= RTOL[dtype]
    assert relerr(out["sum_capacity"], fx["drop%d_capacity" % case].sum(axis=1)) <= RTOL[dtype]
    assert relerr(lin(out["min_sinr_dB"]), lin(fx["drop%d_sinr_dB" % case].min(axis=1))) <= RTOL[dtype]
    if case == 0 and dtype == "f64":          # the application's Python surface draws its own users: shapes and sanity
        scen = {"side_length": row[2], "single_wall_loss_dB": row[3], "num_rooms_per_side": int(row[0]),
                "ap_decimation": int(row[1])}
        s, c = metis.perform_simulation(scen, {"Pt_dBm": row[4], "noise_power_dBm": row[5]}, num_users=100, seed=3,
                                        engine=engine)
        assert s.shape == c.shape == (100,) and np.all(np.isfinite(s)) and np.all(c > 0)


# ---- 4 and 5: drops from Philox against the restatement; splits; integer bookkeeping ------------------------------------------
@functools.lru_cache(maxsize=None)
def philox_reference(case, assoc, active):
    n, dec, L, U, drops = mo.PHILOX_CASES[case]
    cfg = mo.base_cfg(n, dec, L, tx=0.1, noise=2.0e-14, assoc=assoc, active=active)
    pos = mo.philox_positions(mo.PHILOX_SEED, mo.PHILOX_FIRST, drops, U, n, L)
    outs = [mo.drop(cfg, p) for p in pos]
    ref = {k: np.stack([o[k] for o in outs]) for k in ("assoc", "sinr", "capacity", "gap", "margin", "load")}
    ref["active_aps"] = np.array([o["active_aps"] for o in outs])
    for v in ref.values():
        v.setflags(write=False)
    return cfg, ref


def run_drops(engine, cfg, U, first, count, dtype):
    return engine.run_indoor_drops(n_users=U, seed=mo.PHILOX_SEED, first=first, count=count, active=bool(cfg["active"]),
                                   dtype=dtype, per_user=True, **HIST, **mo.engine_kwargs(cfg))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case,assoc,active", [(0, 1, 1), (1, 1, 1), (0, 0, 0), (0, 1, 0)])
def test_philox_drops_against_the_restatement(engine, case, assoc, active, dtype):
    n, dec, L, U, drops = mo.PHILOX_CASES[case]
    cfg, ref = philox_reference(case, assoc, active)
    out = run_drops(engine, cfg, U, mo.PHILOX_FIRST, drops, dtype)
    assert engine.last_kernel() == "indoor_drops %s m2 a%d t%d u%d" % (dtype, assoc, active, 1 if U <= 64 else 2)
    safe = (ref["gap"] > TAU[dtype]) & (ref["margin"] > 2 * mo.ROOM_EDGE * L)         # [drops, U]
    keep = np.all(safe, axis=1, keepdims=True) & np.ones_like(safe) if active else safe
    left_out = int(np.sum(~np.all(keep, axis=1)))
    print("philox drops case %d a%d t%d %s: %d of %d drops hold a user left out" % (case, assoc, active, dtype, left_out, drops))
    assert left_out <= mo.GAP_CAP * drops
    assert np.array_equal(out["assoc"][keep], ref["assoc"][keep])
    whole = np.all(keep, axis=1)
    assert np.array_equal(out["active_aps"][whole], ref["active_aps"][whole])
    e_sinr = relerr(lin(out["sinr_dB"])[keep], ref["sinr"][keep])
    e_cap = relerr(out["capacity"][keep], ref["capacity"][keep])
    print("    SINR %.3g capacity %.3g" % (e_sinr, e_cap))
    assert e_sinr <= RTOL[dtype] and e_cap <= RTOL[dtype]
    assert relerr(out["sum_capacity"][whole], ref["capacity"].sum(axis=1)[whole]) <= RTOL[dtype]
    assert relerr(lin(out["min_sinr_dB"])[whole], ref["sinr"].min(axis=1)[whole]) <= RTOL[dtype]
    want_db = 10.0 * np.log10(ref["sinr"]).sum(axis=1)
    assert np.max(np.abs(out["sum_sinr_dB"] - want_db)[whole]) <= U * 10.0 * np.log10(1.0 + RTOL[dtype]) + 1e-9


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case,assoc,active", [(0, 1, 1), (1, 1, 1), (0, 0, 0)])
def test_splits_and_grids_change_no_bit(engine, case, assoc, active, dtype):
    n, dec, L, U, drops = mo.PHILOX_CASES[case]
    cfg, _ = philox_reference(case, assoc, active)
    first, cut = mo.PHILOX_FIRST, min(50, drops // 2)
    whole = run_drops(engine, cfg, U, first, drops, dtype)
    lo = run_drops(engine, cfg, U, first, cut, dtype)
    hi = run_drops(engine, cfg, U, first + cut, drops - cut, dtype)
    for k, v in whole.items():
        if k in ("hist", "load_hist"):
            assert np.array_equal(lo[k] + hi[k], v), k
        else:
            assert np.array_equal(np.concatenate([lo[k], hi[k]]), v, equal_nan=True), k
    for oversub in (1, 4):
        with engine.options(grid_oversub=oversub):
            again = run_drops(engine, cfg, U, first, drops, dtype)
        for k, v in whole.items():
            assert np.array_equal(again[k], v, equal_nan=True), (k, oversub)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case,assoc,active", [(0, 1, 1), (1, 1, 1), (0, 0, 0)])
def test_integer_bookkeeping_is_exact(engine, case, assoc, active, dtype):
    n, dec, L, U, drops = mo.PHILOX_CASES[case]
    cfg, _ = philox_reference(case, assoc, active)
    A = len(mo.ap_rooms(n, dec))
    out = run_drops(engine, cfg, U, mo.PHILOX_FIRST, drops, dtype)
    slots = mo.hist_slots(out["sinr_dB"], HIST["hist_lo_dB"], HIST["hist_step_dB"], HIST["hist_bins"])
    assert np.array_equal(out["hist"], np.bincount(slots, minlength=HIST["hist_bins"] + 2))
    assert int(out["hist"].sum()) == drops * U and np.count_nonzero(out["hist"]) >= 3
    k = np.arange(U + 1)
    assert int(out["load_hist"].sum()) == drops * A and int((k * out["load_hist"].astype(np.int64)).sum()) == drops * U
    loads = np.stack([np.bincount(a, minlength=A) for a in out["assoc"]])
    assert np.array_equal(out["load_hist"], np.bincount(loads.reshape(-1), minlength=U + 1))
    distinct = np.array([np.unique(a).size for a in out["assoc"]])
    assert np.array_equal(out["active_aps"], distinct if active else np.full(drops, A))
    # every output pointer may be NULL, and an empty range launches nothing
    bare = engine.run_indoor_drops(n_users=U, seed=mo.PHILOX_SEED, first=mo.PHILOX_FIRST, count=drops, active=bool(active),
                                   dtype=dtype, **mo.engine_kwargs(cfg))
    assert np.array_equal(bare["sum_capacity"], out["sum_capacity"]) and int(bare["hist"].sum()) == drops * U
    none = engine.run_indoor_drops(n_users=U, seed=1, first=0, count=0, dtype=dtype, **mo.engine_kwargs(cfg))
    assert none["sum_capacity"].size == 0 and int(none["hist"].sum()) == 0 and engine.last_kernel() == ""


def test_python_surface_refuses_what_the_library_refuses(engine):
    cfg = mo.engine_kwargs(mo.base_cfg(4, 4, 10.0))
    with pytest.raises(ValueError, match="n_users must be in"):
        engine.run_indoor_drops(n_users=257, seed=1, first=0, count=2, **cfg)
    with pytest.raises(ValueError, match="ap_decimation must be"):
        engine.indoor_sinr(np.zeros(3, dtype=complex), **dict(cfg, ap_decimation=3))
    with pytest.raises(ValueError, match="positions must hold"):
        engine.run_indoor_drops(n_users=4, seed=1, first=0, count=2, positions=np.zeros(7, dtype=complex), **cfg)
    assert engine.indoor_sinr(np.zeros((0, 2)), **cfg).shape == (0,)


# ---- 6: the simulator --------------------------------------------------------------------------------------------------------
SIM = dict(num_rooms_per_side=4, side_length=10.0, ap_decimation=[2, 4], num_users=37, rep_max=300, seed=9, dtype="f64",
           hist_bins=24, hist_lo_dB=-10.0, hist_step_dB=2.5)


def sim_state(sim):
    names = ("sinr_dB", "capacity", "sum_capacity", "active_aps")
    res = sim.results
    return ({k: [(r._value, r._total, r._result_sum, r._result_squared_sum, r.num_updates) for r in res[k]] for k in names},
            [r._value.tolist() for r in res["sinr_histogram"]])


def test_drop_simulator_equals_direct_calls(engine):
    sim = simulators.MetisDropSimulator(batch_size=128, engine=engine, **SIM)       # 128 does not divide 300
    sim.simulate()
    assert sim.runned_reps == [300, 300]
    floats, hists = sim_state(sim)
    for v, params in enumerate(sim.params.get_unpacked_params_list()):
        direct = engine.run_indoor_drops(seed=sim._seed_for(params), first=0, count=300, **sim.drop_args(params))
        U = 37
        assert hists[v] == direct["hist"].tolist() and sum(hists[v]) == 300 * U
        value, total, rsum, rsq, updates = floats["sum_capacity"][v]
        assert (total, updates) == (300, 300)
        assert value == pytest.approx(direct["sum_capacity"].sum(), rel=1e-12)
        assert rsq == pytest.approx(np.square(direct["sum_capacity"]).sum(), rel=1e-12)
        value, total, rsum, rsq, updates = floats["capacity"][v]
        assert total == 300 * U and value == pytest.approx(direct["sum_capacity"].sum(), rel=1e-12)
        value, total, rsum, rsq, updates = floats["sinr_dB"][v]
        assert total == 300 * U and value == pytest.approx(direct["sum_sinr_dB"].sum(), rel=1e-12)
        assert rsum == pytest.approx((direct["sum_sinr_dB"] / U).sum(), rel=1e-12)
        value, total, rsum, rsq, updates = floats["active_aps"][v]
        assert (value, total) == (int(direct["active_aps"].sum()), 300)
        assert rsq == float(np.square(direct["active_aps"].astype(np.int64)).sum())
        assert sim.results["sum_capacity"][v].get_result() == pytest.approx(direct["sum_capacity"].mean(), rel=1e-12)
    # fewer APs: fewer of them are on
    assert sim.results["active_aps"][0].get_result() > sim.results["active_aps"][1].get_result()


def test_drop_simulator_resumes_from_partial_results(engine, tmp_path):
    whole = simulators.MetisDropSimulator(batch_size=77, engine=engine, **SIM)
    whole.simulate()
    part = simulators.MetisDropSimulator(batch_size=50, engine=engine, **dict(SIM, rep_max=130))
    part.set_results_filename(str(tmp_path / "metis_{num_users}"))
    part.simulate()
    assert part.runned_reps == [130, 130]
    rest = simulators.MetisDropSimulator(batch_size=64, engine=engine, **SIM)
    rest.set_results_filename(str(tmp_path / "metis_{num_users}"))
    rest.simulate()
    assert rest.runned_reps == [300, 300]
    (f_whole, h_whole), (f_rest, h_rest) = sim_state(whole), sim_state(rest)
    assert h_whole == h_rest
    for name in f_whole:
        for a, b in zip(f_whole[name], f_rest[name]):
            assert a[1] == b[1] and a[4] == b[4]
            assert a[0] == pytest.approx(b[0], rel=1e-12) and a[2] == pytest.approx(b[2], rel=1e-12)
            assert a[3] == pytest.approx(b[3], rel=1e-12)
    assert f_whole["active_aps"] == f_rest["active_aps"]


# ---- 8: a wavefront that takes several drops; NULL outputs -----------------------------------------------------------------------
def loop_count(engine, turns=2):
    """Drops of one call that send every wavefront round the kernel's drop loop more than `turns` times with grid_oversub = 1:
    the launcher then starts at most 8 workgroups of four wavefronts per compute unit (csrc/pipeline_indoor.hip)."""
    return 4 * 8 * engine.n_cu * turns + 3617


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case,assoc,active", [(0, 1, 1), (1, 1, 1), (0, 0, 0)])
def test_a_wavefront_taking_several_drops_changes_no_bit(engine, case, assoc, active, dtype):
    """The tests above give every wavefront ONE drop (at most 300 drops against thousands of resident wavefronts).  Here one
    call with grid_oversub = 1 walks the loop two to three times per wavefront -- the per-drop re-zeroing of the user counts and
    the mask, and LDS histograms that gather several drops -- and must equal, bit for bit, the same range run in pieces of at
    most 4096 drops (1024 workgroups: one drop per wavefront); a few drops of the later turns against the restatement."""
    n, dec, L, U, _ = mo.PHILOX_CASES[case]
    cfg, _ = philox_reference(case, assoc, active)
    first, count = mo.PHILOX_FIRST, loop_count(engine)
    assert count > 2 * 4 * 8 * engine.n_cu and 4096 <= 4 * 8 * engine.n_cu
    with engine.options(grid_oversub=1):
        whole = run_drops(engine, cfg, U, first, count, dtype)
    pieces = [run_drops(engine, cfg, U, first + lo, min(4096, count - lo), dtype) for lo in range(0, count, 4096)]
    for k, v in whole.items():
        if k in ("hist", "load_hist"):
            assert np.array_equal(sum(p[k] for p in pieces), v), k
        else:
            assert np.array_equal(np.concatenate([p[k] for p in pieces]), v, equal_nan=True), k
    assert int(whole["hist"].sum()) == count * U
    turn = 4 * 8 * engine.n_cu
    for r in (0, turn - 1, turn, turn + 5, 2 * turn + 1, count - 1):             # drops of the first, second and third turn
        want = mo.drop(cfg, mo.philox_positions(mo.PHILOX_SEED, first + r, 1, U, n, L)[0])
        safe = (want["gap"] > TAU[dtype]) & (want["margin"] > 2 * mo.ROOM_EDGE * L)
        if active and not np.all(safe):
            continue
        assert np.array_equal(whole["assoc"][r][safe], want["assoc"][safe]), r
        assert relerr(lin(whole["sinr_dB"][r])[safe], want["sinr"][safe]) <= RTOL[dtype], r
        assert relerr(whole["capacity"][r][safe], want["capacity"][safe]) <= RTOL[dtype], r
        if np.all(safe):
            assert whole["active_aps"][r] == want["active_aps"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("active", [0, 1])
def test_every_output_pointer_may_be_null(engine, active, dtype):
    """Straight through the C ABI: all ten outputs NULL, then each of them alone, equal to the full call's array."""
    import ctypes
    from pyphysim_amd import _lib
    n, dec, L, U, _ = mo.PHILOX_CASES[0]
    cfg, _ = philox_reference(0, 1, active)
    count = 70
    full = run_drops(engine, cfg, U, mo.PHILOX_FIRST, count, dtype)
    c = engine._indoor_cfg(active=active, n_users=U, **HIST, **mo.engine_kwargs(cfg))
    names = ["hist", "load_hist", "sum_capacity", "sum_sinr_dB", "min_sinr_dB", "active_aps", "sinr_dB", "capacity", "assoc"]

    def call(ptrs):
        rc = engine.lib.mcle_run_indoor_drops(engine.ctx, _lib.dtype_code(dtype), ctypes.byref(c), mo.PHILOX_SEED,
                                              mo.PHILOX_FIRST, count, None, *ptrs)
        assert rc == 0, engine.lib.mcle_last_error()

    call([None] * 9)
    engine.sync()
    assert engine.last_kernel().startswith("indoor_drops %s m2 a1 t%d" % (dtype, active))
    for i, name in enumerate(names):
        want = full[name]
        buf = engine.zeros(want.shape, want.dtype)
        call([buf.ptr if j == i else None for j in range(9)])
        assert np.array_equal(buf.get(), want, equal_nan=True), name
