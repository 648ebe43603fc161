"""GPU: the hexagonal-cell system-level kernels (csrc/pipeline_hex.hip) -- the operator on injected points mcle_hex_gains and the
fused user drops mcle_run_hex_drops -- against the reference's own results (tests/golden/g9_hex.npz) and the NumPy statement
tests/hex_oracle.py, in both arithmetics; and simulators.HexDropSimulator on top of them.

Tolerances ("Hexagonal-cell system level"): f64 holds distances, gains, the linear SINR and the capacity to 1e-12
relative, the bound of the indoor kernels for the same arithmetic.  For f32 the largest relative error of the linear SINR
against the f64 fixture over all cases of test 1 was measured (F32_MEASURED) and eight times it, rounded up to one digit, is
the bound, as the indoor kernels set theirs.  Positions and flags are compared bit for bit in both arithmetics."""
import ctypes
import functools

import numpy as np
import pytest

import hex_oracle as ho
from pyphysim_amd import _lib, cell, simulators

pytestmark = pytest.mark.gpu

F64_RTOL = 1e-12
F32_MEASURED = 2.60e-6       # largest relative error of the f32 linear SINR over test 1
F32_RTOL = 3e-5              # 8 x F32_MEASURED = 2.08e-5, rounded up to one digit
RTOL = {"f64": F64_RTOL, "f32": F32_RTOL}
HIST = dict(hist_bins=24, hist_lo_dB=-20.0, hist_step_dB=2.5)
DTYPES = ["f64", "f32"]
N_PLACE = 9
# Philox cases: (cells, users per cell, min_dist_ratio, wrap, cell radius, n_ext, drops from first = 7)
PHILOX_SEED, PHILOX_FIRST = 20261021, 7
PHILOX_CASES = [(1, 1, 0.0, False, 1.0, 0, 40), (3, 1, 0.0, False, 1.0, 1, 130), (3, 2, 0.7, False, 0.35, 2, 130),
                (7, 5, 0.0, False, 1.0, 0, 20), (19, 1, 0.0, True, 1.0, 8, 20), (19, 5, 0.7, True, 1.0, 1, 6),
                (19, 13, 0.0, False, 0.35, 0, 3), (19, 13, 0.0, True, 0.35, 1, 2)]


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(ho.load_fixture())


def relerr(got, want):
    want = np.asarray(want, dtype=float)
    return float(np.max(np.abs(np.asarray(got, dtype=float) - want) / np.abs(want))) if want.size else 0.0


def lin(db):
    return 10.0 ** (np.asarray(db, dtype=float) / 10.0)


def slots(KU):
    return 1 if KU <= 64 else 2 if KU <= 128 else 4


def fixture_cfg(case, **kw):
    fx = fixture()
    K, U, ratio, r, S = fx["place%d_cfg" % case]
    tx, noise, pe = fx["powers"]
    return ho.base_cfg(int(K), float(r), int(U), float(ratio), tx=tx, noise=noise, pe=pe, **kw), int(S)


# ---- 1: the operator on the fixture's positions ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", range(N_PLACE))
def test_operator_against_the_reference(engine, case, dtype):
    fx = fixture()
    key = "place%d_" % case
    cfg, S = fixture_cfg(case)
    K = cfg["K"]
    pts = fx[key + "pos"]
    out = engine.hex_gains(pts, dtype=dtype, **ho.engine_kwargs(cfg))
    assert engine.last_kernel() == "hex_gains %s m1 w0" % dtype
    assert out["dist"].shape == pts.shape + (K,) and out["gain"].shape == pts.shape + (K + 1,)
    e_dist = relerr(out["dist"], fx[key + "dist"])
    e_gain = max(relerr(out["gain"][..., :K], fx[key + "pl3gpp"]), relerr(out["gain"][..., K], fx[key + "plint3gpp"]))
    ok = fx[key + "assoc_ok"]
    e_sinr = relerr(lin(out["sinr_dB"])[ok], fx[key + "sinr_best"][ok])
    print("operator case %d %s: distance %.3g gain %.3g SINR %.3g" % (case, dtype, e_dist, e_gain, e_sinr))
    assert e_dist <= F64_RTOL                                   # distances are f64 in either arithmetic
    assert e_gain <= RTOL[dtype] and e_sinr <= RTOL[dtype]
    assert np.array_equal(out["assoc"][ok], fx[key + "assoc"][ok])
    if key + "plfree" in fx:
        free = engine.hex_gains(pts, dtype=dtype, **ho.engine_kwargs(dict(cfg, **ho.MODELS["free"])))
        e_free = max(relerr(free["gain"][..., :K], fx[key + "plfree"]), relerr(free["gain"][..., K], fx[key + "plintfree"]))
        print("    free space: gain %.3g" % e_free)
        assert e_free <= RTOL[dtype]
    none = engine.hex_gains(pts[0], dtype=dtype, **ho.engine_kwargs(dict(cfg, model="none")))
    assert engine.last_kernel() == "hex_gains %s m0 w0" % dtype and np.all(none["gain"] == 1.0) and np.all(none["assoc"] == 0)
    assert relerr(lin(none["sinr_dB"]), cfg["tx"] / (cfg["tx"] * (K - 1) + cfg["pe"] + cfg["noise"])) <= RTOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_operator_with_wrap_around(engine, dtype):
    """No reference result exists (its distance matrix ignores the wrapped cells): the statement on the reference's wrapped
    position lists (held to the fixture by tests/test_hex_cpu.py)."""
    fx = fixture()
    pts = np.concatenate([fx["place%d_pos" % c].reshape(-1) for c in (6, 7)])
    cfg, _ = fixture_cfg(6, wrap=True)
    want, plain = ho.operator(cfg, pts), ho.operator(dict(cfg, wrap=False), pts)
    assert np.mean(want["dist"] < plain["dist"] * (1 - 1e-9)) > 0.05         # the wrapped copies are nearer for many pairs
    out = engine.hex_gains(pts, dtype=dtype, **ho.engine_kwargs(cfg))
    assert engine.last_kernel() == "hex_gains %s m1 w1" % dtype
    ok = want["gap"] > 1e-3
    e = (relerr(out["dist"], want["dist"]), relerr(out["gain"], want["gain"]), relerr(lin(out["sinr_dB"])[ok], want["sinr"][ok]))
    print("operator with wrap %s: distance %.3g gain %.3g SINR %.3g" % ((dtype,) + e))
    assert e[0] <= F64_RTOL and e[1] <= RTOL[dtype] and e[2] <= RTOL[dtype]
    assert np.array_equal(out["assoc"][ok], want["assoc"][ok])


# ---- 2: the clamp -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_clamp_on_a_base_station_and_on_the_far_vertex(engine, dtype):
    cl = cell.Cluster(1.0, 3)
    last = list(cl)[-1]
    far = last.vertices[np.argmax(np.abs(last.vertices - cl.pos))]
    inside = cl.cell_positions + 0.25
    pos = np.array([[cl.cell_positions[0], inside[1], inside[2]], [inside[0], inside[1], far]])      # [2 drops, 3 users]
    cfg = ho.base_cfg(3, 1.0, 1, tx=0.5, noise=1e-14, pe=1e-3, n_ext=2)
    out = engine.run_hex_drops(seed=1, first=0, count=2, positions=pos, dtype=dtype, per_user=True, records=True,
                               **ho.engine_kwargs(cfg, drops=True))
    rec = out["records"].get()
    assert rec.shape == (2, 3, 5) and np.all(out["flags"] == 0)
    assert rec[0, 0, 0] == 1.0                                  # on the base station: distance 0, loss clamped to 0 dB
    assert rec[1, 2, 3] == 1.0 and rec[1, 2, 4] == 1.0          # on the far vertex: the interferer at distance 0
    assert np.all(rec[..., 3] == rec[..., 4]) and np.all((rec > 0) & (rec <= 1.0))
    assert np.count_nonzero(rec == 1.0) == 3
    want = [ho.drop(cfg, p) for p in pos]
    assert relerr(rec, np.stack([w["records"] for w in want])) <= RTOL[dtype]
    assert relerr(lin(out["sinr_dB"]), np.stack([w["sinr"] for w in want])) <= RTOL[dtype]
    assert np.array_equal(out["positions"], pos)
    op = engine.hex_gains(pos, dtype=dtype, **ho.engine_kwargs(cfg))
    assert op["gain"][0, 0, 0] == 1.0 and op["gain"][1, 2, 3] == 1.0 and op["dist"][0, 0, 0] == 0.0


# ---- 3: drops from Philox against the statement -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def philox_reference(case):
    K, U, ratio, wrap, r, E, drops = PHILOX_CASES[case]
    cfg = ho.base_cfg(K, r, U, ratio, wrap=wrap, tx=0.2, noise=3.0e-14, pe=2.0e-9 if E else 0.0, n_ext=E)
    pos, flags = ho.philox_positions(cfg, PHILOX_SEED, PHILOX_FIRST, drops)
    outs = [ho.drop(cfg, p) for p in pos]
    ref = {k: np.stack([o[k] for o in outs]) for k in ("records", "sinr", "capacity")}
    ref.update(positions=pos, flags=flags)
    for v in ref.values():
        v.setflags(write=False)
    return cfg, ref


def run_drops(engine, cfg, first, count, dtype, per_user=True, records=True):
    out = engine.run_hex_drops(seed=PHILOX_SEED, first=first, count=count, dtype=dtype, per_user=per_user, records=records,
                               **HIST, **ho.engine_kwargs(cfg, drops=True))
    if records:
        out["records"] = out["records"].get()
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", range(len(PHILOX_CASES)))
def test_philox_drops_against_the_statement(engine, case, dtype):
    K, U, ratio, wrap, r, E, drops = PHILOX_CASES[case]
    cfg, ref = philox_reference(case)
    out = run_drops(engine, cfg, PHILOX_FIRST, drops, dtype)
    assert engine.last_kernel() == "hex_drops %s m1 u%d w%d" % (dtype, slots(K * U), wrap)
    assert same_bits(out["positions"], ref["positions"]) and np.array_equal(out["flags"], ref["flags"]) and not out["flags"].any()
    off = out["positions"] - np.repeat(cell.Cluster(r, K).cell_positions, U)[None, :]
    assert np.all(np.abs(off) >= ratio * r) and all(cell.inside_hexagon(o, r) for o in off.reshape(-1))
    e = (relerr(out["records"], ref["records"]), relerr(lin(out["sinr_dB"]), ref["sinr"]), relerr(out["capacity"], ref["capacity"]))
    print("philox drops case %d %s: records %.3g SINR %.3g capacity %.3g" % ((case, dtype) + e))
    assert out["records"].shape == (drops, K * U, K + E) and max(e) <= RTOL[dtype]
    assert relerr(out["sum_capacity"], ref["capacity"].sum(axis=1)) <= RTOL[dtype]
    assert relerr(lin(out["min_sinr_dB"]), ref["sinr"].min(axis=1)) <= RTOL[dtype]
    # exact bookkeeping on the kernel's own figures
    want = np.bincount(ho.hist_slots(out["sinr_dB"], HIST["hist_lo_dB"], HIST["hist_step_dB"], HIST["hist_bins"]),
                       minlength=HIST["hist_bins"] + 2)
    assert np.array_equal(out["hist"], want) and int(out["hist"].sum()) == drops * K * U
    assert np.array_equal(out["min_sinr_dB"], out["sinr_dB"].min(axis=1))
    assert np.allclose(out["capacity"], np.log2(1.0 + lin(out["sinr_dB"])), rtol=1e-12, atol=0)


# ---- 4: determinism ----------------------------------------------------------------------------------------------------------
def assert_same(whole, pieces):
    for k, v in whole.items():
        if k == "hist":
            assert np.array_equal(sum(p[k] for p in pieces), v), k
        else:
            assert same_bits(np.concatenate([p[k] for p in pieces]), v), k


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [1, 2, 5])
def test_splits_and_grids_change_no_bit(engine, case, dtype):
    cfg, _ = philox_reference(case)
    first, count, cut = 7, 130, 50
    whole = run_drops(engine, cfg, first, count, dtype)
    assert_same(whole, [run_drops(engine, cfg, first, cut, dtype), run_drops(engine, cfg, first + cut, count - cut, dtype)])
    for oversub in (1, 4):
        with engine.options(grid_oversub=oversub):
            assert_same(whole, [run_drops(engine, cfg, first, count, dtype)])


def loop_count(engine, turns=2):
    """Drops of one call that send every wavefront round the kernel's drop loop more than `turns` times with grid_oversub = 1:
    the launcher then starts at most 8 workgroups of four wavefronts per compute unit (csrc/pipeline_hex.hip)."""
    return 4 * 8 * engine.n_cu * turns + 3617


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case,full", [(1, True), (5, False)])
def test_a_wavefront_taking_several_drops_changes_no_bit(engine, case, full, dtype):
    """The tests above give every wavefront ONE drop.  Here one call with grid_oversub = 1 walks the loop two to three times
    per wavefront -- LDS histograms that gather several drops -- and must equal, bit for bit, the same range run in pieces
    of at most 4096 drops (one drop per wavefront); a few drops of the later turns against the statement.  The 95-user case
    leaves the per-user arrays and the records out (a gigabyte at this count)."""
    K, U, ratio, wrap, r, E, _ = PHILOX_CASES[case]
    cfg, _ = philox_reference(case)
    first, count = PHILOX_FIRST, loop_count(engine)
    assert count > 2 * 4 * 8 * engine.n_cu and 4096 <= 4 * 8 * engine.n_cu
    with engine.options(grid_oversub=1):
        whole = run_drops(engine, cfg, first, count, dtype, per_user=full, records=full)
    assert_same(whole, [run_drops(engine, cfg, first + lo, min(4096, count - lo), dtype, per_user=full, records=full)
                        for lo in range(0, count, 4096)])
    assert int(whole["hist"].sum()) == count * K * U and not whole["flags"].any()
    turn = 4 * 8 * engine.n_cu
    for d in (0, turn - 1, turn, turn + 5, 2 * turn + 1, count - 1):             # drops of the first, second and third turn
        pos, flag = ho.philox_drop(cfg, PHILOX_SEED, first + d)
        want = ho.drop(cfg, pos)
        assert relerr(whole["sum_capacity"][d], want["capacity"].sum()) <= RTOL[dtype], d
        assert relerr(lin(whole["min_sinr_dB"][d]), want["sinr"].min()) <= RTOL[dtype], d
        if full:
            assert same_bits(whole["positions"][d], pos) and relerr(whole["records"][d], want["records"]) <= RTOL[dtype], d


# ---- 5: NULL outputs, refusals -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_output_pointer_may_be_null(engine, dtype):
    """Straight through the C ABI: all eight outputs of the drops NULL, then each alone, then each NULL on its own, equal to the
    full call's arrays; the same for the operator's four."""
    cfg, _ = philox_reference(2)
    K, U, E, count = cfg["K"], cfg["U"], cfg["n_ext"], 70
    full = run_drops(engine, cfg, PHILOX_FIRST, count, dtype)
    full["pos_out"] = np.ascontiguousarray(full["positions"]).view(np.float64).reshape(count, K * U, 2)
    c = engine._hex_cfg(**HIST, **ho.engine_kwargs(cfg, drops=True))
    names = ["flags", "records", "pos_out", "sinr_dB", "capacity", "hist", "sum_capacity", "min_sinr_dB"]

    def call(ptrs):
        rc = engine.lib.mcle_run_hex_drops(engine.ctx, _lib.dtype_code(dtype), ctypes.byref(c), PHILOX_SEED, PHILOX_FIRST, count,
                                           None, *ptrs)
        assert rc == 0, engine.lib.mcle_last_error()

    call([None] * 8)
    engine.sync()
    assert engine.last_kernel() == "hex_drops %s m1 u1 w0" % dtype
    for i, name in enumerate(names):
        want = full[name]
        buf = engine.zeros(want.shape, want.dtype)
        call([buf.ptr if j == i else None for j in range(8)])
        assert same_bits(buf.get(), want), name
    for i, name in enumerate(names):                       # each NULL on its own: the other seven are written as in the full call
        bufs = [engine.zeros(full[n].shape, full[n].dtype) for n in names]
        call([None if j == i else b.ptr for j, b in enumerate(bufs)])
        for j, n in enumerate(names):
            assert j == i or same_bits(bufs[j].get(), full[n]), (name, n)
    pts = full["pos_out"].reshape(-1, 2)
    op = engine.hex_gains(pts, dtype=dtype, **ho.engine_kwargs(cfg))
    d_pts = engine.to_device(pts.reshape(-1))
    g = engine._hex_cfg(**ho.engine_kwargs(cfg))

    def gains(ptrs):
        rc = engine.lib.mcle_hex_gains(engine.ctx, _lib.dtype_code(dtype), ctypes.byref(g), d_pts.ptr, len(pts), *ptrs)
        assert rc == 0, engine.lib.mcle_last_error()

    gains([None] * 4)
    engine.sync()
    for i, name in enumerate(["dist", "gain", "sinr_dB", "assoc"]):
        buf = engine.zeros(op[name].shape, op[name].dtype)
        gains([buf.ptr if j == i else None for j in range(4)])
        assert same_bits(buf.get(), op[name]), name
        bufs = [engine.zeros(op[n].shape, op[n].dtype) for n in ("dist", "gain", "sinr_dB", "assoc")]
        gains([None if j == i else b.ptr for j, b in enumerate(bufs)])
        for j, n in enumerate(("dist", "gain", "sinr_dB", "assoc")):
            assert j == i or same_bits(bufs[j].get(), op[n]), (name, n)


def test_python_surface_refuses_what_the_library_refuses(engine):
    kw = ho.engine_kwargs(ho.base_cfg(7, 1.0, 2), drops=True)
    with pytest.raises(ValueError, match="users_per_cell must be"):
        engine.run_hex_drops(seed=1, first=0, count=2, **dict(kw, users_per_cell=37))
    with pytest.raises(ValueError, match="num_cells must be"):
        engine.run_hex_drops(seed=1, first=0, count=2, **dict(kw, num_cells=20))
    with pytest.raises(ValueError, match="wrap_around needs"):
        engine.run_hex_drops(seed=1, first=0, count=2, **dict(kw, wrap_around=True))
    with pytest.raises(ValueError, match="min_dist_ratio must be"):
        engine.run_hex_drops(seed=1, first=0, count=2, **dict(kw, min_dist_ratio=0.71))
    with pytest.raises(ValueError, match="positions must hold"):
        engine.run_hex_drops(seed=1, first=0, count=2, positions=np.zeros(7, dtype=complex), **kw)
    none = engine.run_hex_drops(seed=1, first=0, count=0, **kw)
    assert none["sum_capacity"].size == 0 and int(none["hist"].sum()) == 0 and engine.last_kernel() == ""
    kw = ho.engine_kwargs(ho.base_cfg(7, 1.0))
    assert engine.hex_gains(np.zeros((0, 2)), **kw)["sinr_dB"].shape == (0,)
    with pytest.raises(ValueError, match="n_ext must be"):
        engine.hex_gains(np.zeros(3, dtype=complex), **dict(kw, n_ext=9))


# ---- 6: the simulator --------------------------------------------------------------------------------------------------------
SIM = dict(num_cells=7, cell_radius=0.5, users_per_cell=[1, 5], Pt_dBm=30.0, noise_power_dBm=-100.0, min_dist_ratio=0.1,
           ext_power_dBm=-20.0, rep_max=300, seed=9, dtype="f64", hist_bins=24, hist_lo_dB=-20.0, hist_step_dB=2.5)


def test_drop_simulator_equals_direct_calls(engine):
    sim = simulators.HexDropSimulator(batch_size=128, engine=engine, **SIM)       # 128 does not divide 300
    sim.simulate()
    assert sim.runned_reps == [300, 300]
    res = sim.results
    for v, params in enumerate(sim.params.get_unpacked_params_list()):
        direct = engine.run_hex_drops(seed=sim._seed_for(params), first=0, count=300, per_user=True, **sim.drop_args(params))
        KU = 7 * int(params["users_per_cell"])
        assert res["sinr_histogram"][v]._value.tolist() == direct["hist"].tolist() and int(direct["hist"].sum()) == 300 * KU
        cap = res["sum_capacity"][v]
        assert (cap._total, cap.num_updates) == (300, 300)
        assert cap._value == pytest.approx(direct["sum_capacity"].sum(), rel=1e-12)
        assert cap._result_squared_sum == pytest.approx(np.square(direct["sum_capacity"]).sum(), rel=1e-12)
        assert res["capacity"][v]._total == 300 * KU
        assert res["capacity"][v].get_result() == pytest.approx(direct["capacity"].mean(), rel=1e-12)
        assert res["sinr_dB"][v].get_result() == pytest.approx(direct["sinr_dB"].mean(), rel=1e-12)
        assert res["min_sinr_dB"][v].get_result() == pytest.approx(direct["min_sinr_dB"].mean(), rel=1e-12)
    # more users per cell: the same mean capacity per user, a worse worst user
    assert res["min_sinr_dB"][0].get_result() > res["min_sinr_dB"][1].get_result()


def test_drop_simulator_resumes_from_partial_results(engine, tmp_path):
    whole = simulators.HexDropSimulator(batch_size=77, engine=engine, **SIM)
    whole.simulate()
    part = simulators.HexDropSimulator(batch_size=50, engine=engine, **dict(SIM, rep_max=130))
    part.set_results_filename(str(tmp_path / "hex_{users_per_cell}"))
    part.simulate()
    rest = simulators.HexDropSimulator(batch_size=64, engine=engine, **SIM)
    rest.set_results_filename(str(tmp_path / "hex_{users_per_cell}"))
    rest.simulate()
    assert rest.runned_reps == [300, 300]
    for name in ("sinr_dB", "capacity", "sum_capacity", "min_sinr_dB"):
        for a, b in zip(whole.results[name], rest.results[name]):
            assert a._total == b._total and a.num_updates == b.num_updates
            assert a._value == pytest.approx(b._value, rel=1e-12) and a._result_squared_sum == pytest.approx(b._result_squared_sum, rel=1e-12)
    assert [r._value.tolist() for r in whole.results["sinr_histogram"]] == [r._value.tolist() for r in rest.results["sinr_histogram"]]
