"""GPU: the fused IA link on general geometries (csrc/pipeline_ia_general.hip, mcle_run_ia_general /
Engine.run_ia_general).

The solver's eigenvector phases are not LAPACK's, so a link built on the NumPy solver's F and U is not comparable decision by
decision with the device's (tests/test_gpu_ia_general.py).  The comparison is staged, as tests/test_gpu_comp.py::staged_check
does it: the draws against the ledger (tests/ia_link_oracle.py), the solver inside the pipeline against the operator
Engine.ia_solve_general on the pipeline's own inputs (bitwise), and the link against ia_link_oracle.link evaluated in NumPy on
the device's solution and the oracle's data and noise draws.

Near ties: a realization holding a symbol whose margin (second-nearest minus nearest constellation distance) is below 1e-9
of the constellation's minimum distance is left out of the staged comparison; at most 1 of the 150 may be (asserted;
tests/test_ia_general_link_cpu.py shows with the NumPy solver that these operating points have none).

Every case sits at the common 15 dB and must make errors there (asserted).  With a converged max-SINR solution two would not
-- (4, 4, 4, 1) with 16-QAM and the BPSK case -- so the first stops after 2 iterations and the second selects over alternating
minimisation: tests/ia_link_oracle.py (LINK_CASES) has the figures."""
import ctypes

import numpy as np
import pytest

import ia_link_oracle as lo
from helpers import relerr

pytestmark = pytest.mark.gpu

SEED, FIRST, COUNT, NV = lo.SEED, lo.FIRST, lo.COUNT, lo.NOISE_VAR
_cache = {}


def bind(engine, mod, M):
    from pyphysim_amd import modulators
    m = {"qam": lambda: modulators.QAM(M, engine=engine), "bpsk": lambda: modulators.BPSK(engine=engine)}[mod]()
    m._bind()
    return m


def run(engine, c, dtype="f64", first=FIRST, count=COUNT, outputs=("big_H", "F_init", "F", "U", "sinr"), n_symbols=None):
    """One pipeline call of a case, shared between the tests that read it (never written to)."""
    key = (tuple(sorted((k, str(v)) for k, v in c.items())), dtype, first, count, outputs, n_symbols)
    if key not in _cache:
        bind(engine, c["mod"], c["M"])
        res, a = engine.run_ia_general(c["K"], c["nr"], c["nt"], c["Ns"], n_symbols or c["n_symbols"], NV, SEED, first, count,
                                       solver=c["solver"], select=c["select"], initialize_with=c["init"],
                                       max_iterations=c["max_iterations"], relative_factor=c["relative_factor"],
                                       method=1 if c["slicer"] else 0, dtype=dtype, per_realization=True, outputs=outputs)
        for v in a.values():
            v.setflags(write=False)
        _cache[key] = (res, a, engine.last_kernel())
    return _cache[key]


@pytest.mark.parametrize("shape", lo.DRAW_SHAPES, ids=str)
def test_draws_follow_the_ledger(engine, shape):
    K, nr, nt, Ns = shape
    c = lo.case(K, nr, nt, Ns, max_iterations=1, n_symbols=2)
    _, a, _ = run(engine, c, outputs=("big_H", "F_init"))
    D = lo.capacity(nr, nt)
    assert a["big_H"].shape == (COUNT, K * nr, K * nt) and a["F_init"].shape == (COUNT, K, D, D)
    worst_h = worst_f = 0.0
    for i in range(COUNT):
        worst_h = max(worst_h, relerr(a["big_H"][i], lo.draw_big_H(SEED, FIRST + i, K, nr, nt)))
        worst_f = max(worst_f, relerr(a["F_init"][i], lo.pad(lo.draw_start(SEED, FIRST + i, K, nt, Ns), D)[:K]))
    print("big_H %.2e, start %.2e" % (worst_h, worst_f))
    assert worst_h <= 1e-13 and worst_f <= 1e-13


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


@pytest.mark.parametrize("name", sorted(lo.SOLVER_CASES))
def test_solver_in_the_pipeline_is_the_operator(engine, name):
    c = lo.SOLVER_CASES[name]
    K, nr, nt = c["K"], c["nr"], c["nt"]
    D = lo.capacity(nr, nt)
    res, a, _ = run(engine, c, n_symbols=2)
    start = a["F_init"] if (c["init"] == "random" and c["select"] != "brute") else None
    sol = engine.ia_solve_general(c["solver"], a["big_H"], K, nr, nt, c["Ns"], NV, c["max_iterations"], c["relative_factor"],
                                  F_init=start, select=c["select"])
    assert np.array_equal(bits(sol["F"]), bits(a["F"])) and np.array_equal(bits(sol["U"]), bits(a["U"]))
    assert np.array_equal(sol["Ns"], a["ns"])
    assert np.array_equal(bits(sol["sinr"]), bits(a["sinr"][:, :, :D])) and not a["sinr"][:, :, D:].any()
    assert np.array_equal(bits(sol["capacity"]), bits(a["capacity"]))
    assert np.array_equal(sol["iterations"], a["iterations"])
    assert np.array_equal(sol["skipped"] != 0, a["sym_err"] == 0xFFFFFFFF)
    assert res["n_skipped"] == int((sol["skipped"] != 0).sum())


def staged(engine, name):
    c = lo.LINK_CASES[name]
    K, nr, nt, M, ns_sym = c["K"], c["nr"], c["nt"], c["M"], c["n_symbols"]
    Ns0 = lo.ns_list(K, c["Ns"])
    res, a, kernel = run(engine, c)
    D = lo.capacity(nr, nt)
    assert kernel == "ia_general_link f64 D%d %s" % (D, "pairs" if ns_sym % 2 == 0 else "single")
    table = lo.table_for(c["mod"], M)
    dmin = lo.min_distance(table)
    ok = a["sym_err"] != 0xFFFFFFFF
    # counters
    se, be = a["sym_err"][ok].astype(np.int64), a["bit_err"][ok].astype(np.int64)
    assert res["n_realizations"] == int(ok.sum()) and res["n_skipped"] == int((~ok).sum())
    assert res["sym_errors"] == int(se.sum()) and res["sym_errors_sq"] == int((se ** 2).sum())
    assert res["bit_errors"] == int(be.sum()) and res["bit_errors_sq"] == int((be ** 2).sum())
    assert res["n_symbols"] == ns_sym * sum(Ns0) and res["n_bits"] == ns_sym * sum(Ns0) * lo.omodem.level2bits(M)
    assert np.array_equal(se, a["stream_sym_err"][ok].reshape(int(ok.sum()), -1).sum(axis=1))
    assert np.array_equal(be, a["stream_bit_err"][ok].reshape(int(ok.sum()), -1).sum(axis=1))
    assert not a["stream_sym_err"][~ok].any() and not a["stream_bit_err"][~ok].any()
    assert np.all(a["ns"] >= 1) and np.all(a["ns"] <= np.array(Ns0))
    left_out = 0
    for i in range(COUNT):
        if not ok[i]:
            continue
        nsi = [int(v) for v in a["ns"][i]]
        F, U = lo.unpad(a["F"][i], a["U"][i], nsi, nr, nt)
        data, noise = lo.draw_link_inputs(SEED, FIRST + i, K, nr, nsi, ns_sym, M, NV)
        assert data.size == ns_sym * sum(nsi)                # the symbols the realization actually sent
        out = lo.link(a["big_H"][i], F, U, nsi, data, noise, table, slicer_M=M if c["slicer"] else None)
        if out["margin"].min() < 1e-9 * dmin:
            left_out += 1
            continue
        assert np.array_equal(a["stream_sym_err"][i], lo.to_slots(out["sym_err"], nsi)), (name, i)
        assert np.array_equal(a["stream_bit_err"][i], lo.to_slots(out["bit_err"], nsi)), (name, i)
        slots = np.arange(lo.SLOTS)[None, :] >= np.array(nsi)[:, None]
        assert not a["stream_sym_err"][i][slots].any() and not a["sinr"][i][slots].any()
    assert left_out <= 1, "near ties: %d of %d realizations left out" % (left_out, COUNT)
    return a


@pytest.mark.parametrize("name", sorted(lo.LINK_CASES))
def test_staged_equality_f64(engine, name):
    a = staged(engine, name)
    if name == "greedy-3x3x3x3":
        assert len(set(map(tuple, a["ns"].tolist()))) >= 3
    ok = a["sym_err"] != 0xFFFFFFFF
    print("%s: %d symbol errors" % (name, int(a["sym_err"][ok].sum())))
    assert a["sym_err"][ok].sum() > 0                         # an operating point at which the link makes errors


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_split_invariance(engine, dtype):
    c = lo.GREEDY_333
    names = ("big_H", "F_init", "F", "U", "sinr")
    _, whole, _ = run(engine, c, dtype=dtype)
    _, lo_part, _ = run(engine, c, dtype=dtype, first=FIRST, count=100 - FIRST)
    _, hi_part, _ = run(engine, c, dtype=dtype, first=100, count=FIRST + COUNT - 100)
    for k in whole:
        assert np.array_equal(bits(whole[k]), bits(np.concatenate([lo_part[k], hi_part[k]]))), k
    assert set(whole) == set(names) | {"sym_err", "bit_err", "stream_sym_err", "stream_bit_err", "ns", "capacity", "iterations"}


def test_count_zero_launches_nothing(engine):
    c = lo.GREEDY_333
    bind(engine, c["mod"], c["M"])
    res, a = engine.run_ia_general(c["K"], c["nr"], c["nt"], c["Ns"], 20, NV, SEED, FIRST, 0, select="greedy", per_realization=True)
    assert engine.last_kernel() == ""
    assert all(v == 0 for k, v in res.items()) and a["sym_err"].size == 0


@pytest.mark.parametrize("name", ["max_sinr-3x5x3x2", "greedy-3x3x3x3"])
def test_f32_against_f64(engine, name):
    c = lo.LINK_CASES[name]
    r64, a64, _ = run(engine, c, n_symbols=50, outputs=())
    r32, a32, kernel = run(engine, c, dtype="f32", n_symbols=50, outputs=())
    assert kernel == "ia_general_link f32 D%d pairs" % lo.capacity(c["nr"], c["nt"])
    assert np.array_equal(a32["ns"], a64["ns"]) and np.array_equal(a32["iterations"], a64["iterations"])
    assert np.array_equal(bits(a32["capacity"]), bits(a64["capacity"]))
    ok = a64["sym_err"] != 0xFFFFFFFF
    assert np.array_equal(ok, a32["sym_err"] != 0xFFFFFFFF)
    sent = 50 * int(a64["ns"][ok].sum())
    diff = abs(int(a32["sym_err"][ok].astype(np.int64).sum()) - int(a64["sym_err"][ok].astype(np.int64).sum()))
    print("%s: |sym_err32 - sym_err64| = %d of %d symbols" % (name, diff, sent))
    assert diff <= 1e-4 * sent


# ---- the envelope ------------------------------------------------------------------------------------------------
def good_cfg():
    return dict(K=3, nr=3, nt=3, ns=(2, 2, 2, 0), solver=3, initialize_with=0, max_iterations=5, stream_selection=0,
                noise_var=0.1, relative_factor=1e-6)


REFUSALS = [dict(K=1), dict(K=5), dict(nr=0), dict(nt=7), dict(solver=0), dict(solver=4), dict(initialize_with=1),
            dict(initialize_with=3, nr=2, ns=(2, 2, 2, 0)), dict(stream_selection=3), dict(stream_selection=2, nt=2),
            dict(max_iterations=0), dict(noise_var=-1.0), dict(relative_factor=-1.0), dict(ns=(2, 0, 2, 0)), dict(ns=(2, 4, 2, 0)),
            dict(K=4, nr=6, nt=6, ns=(6, 6, 6, 6), stream_selection=2)]


def make_cfg(**over):
    from pyphysim_amd import _lib
    kw = good_cfg()
    kw.update(over)
    cfg = _lib.IaGeneralCfg()
    for k, v in kw.items():
        if k == "ns":
            for i in range(4):
                cfg.ns[i] = v[i]
        else:
            setattr(cfg, k, v)
    return cfg


def call_run(engine, cfg, n_symbols, outs, dtype=1, method=0, count=4):
    p = lambda k: outs[k].ptr if k in outs else None
    return engine.lib.mcle_run_ia_general(engine.ctx, dtype, ctypes.byref(cfg), n_symbols, method, SEED, FIRST, count, p("cnt"),
                                          p("sym"), p("bit"), p("ssym"), p("sbit"), p("ns"), p("sinr"), p("cap"), p("it"),
                                          p("H"), p("Fi"), p("F"), p("U"))


def sentinel_outputs(engine, count=4):
    from pyphysim_amd import _lib
    shapes = dict(cnt=(ctypes.sizeof(_lib.Counters),), sym=(count * 4,), bit=(count * 4,), ssym=(count * 96,), sbit=(count * 96,),
                  ns=(count * 16,), sinr=(count * 192,), cap=(count * 8,), it=(count * 4,), H=(count * 36 * 36 * 16,),
                  Fi=(count * 2304,), F=(count * 2304,), U=(count * 2304,))
    outs = {k: engine.empty(s, np.uint8) for k, s in shapes.items()}
    for v in outs.values():
        v.set(np.full(v.shape, 0xAB, dtype=np.uint8))
    return outs


def untouched(outs):
    return all(np.all(v.get() == 0xAB) for v in outs.values())


@pytest.mark.parametrize("over", REFUSALS, ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_refusals_are_the_operators(engine, over):
    """Every refusal of mcle_ia_solve_general reaches the caller of mcle_run_ia_general in the same words, before anything
    is written."""
    bind(engine, "qam", 16)
    cfg = make_cfg(**over)
    dummy = engine.zeros(4 * 4 * 36 * 2, np.float64)
    rc = engine.lib.mcle_ia_solve_general(engine.ctx, ctypes.byref(cfg), dummy.ptr, dummy.ptr, dummy.ptr, dummy.ptr, None, None,
                                          None, None, None, None, 1)
    want = engine.lib.mcle_last_error().decode()
    assert rc == -1 and want
    outs = sentinel_outputs(engine)
    assert call_run(engine, cfg, 20, outs) == -1
    assert engine.lib.mcle_last_error().decode() == want
    assert engine.last_kernel() == "" and untouched(outs)


def test_own_refusals(engine):
    from pyphysim_amd import _lib
    bind(engine, "qam", 16)
    outs = sentinel_outputs(engine)
    assert call_run(engine, make_cfg(), 0, outs) == -1 and "n_symbols" in engine.lib.mcle_last_error().decode()
    assert call_run(engine, make_cfg(), -3, outs) == -1
    assert call_run(engine, make_cfg(), 20, outs, dtype=7) == -1
    assert call_run(engine, make_cfg(), 20, outs, method=9) == -1
    assert call_run(engine, make_cfg(), 1 << 30, outs) == -1 and "32-bit" in engine.lib.mcle_last_error().decode()
    engine.set_constellation(np.exp(2j * np.pi * np.arange(512) / 512.0), _lib.CONST_GENERIC)
    assert call_run(engine, make_cfg(), 20, outs) == -1 and "M <= 256" in engine.lib.mcle_last_error().decode()
    assert untouched(outs)
    bind(engine, "qam", 16)
    with pytest.raises(ValueError, match="n_symbols"):
        engine.run_ia_general(3, 3, 3, 2, 0, NV, SEED, FIRST, 4)
    with pytest.raises(ValueError, match="general-geometry solvers"):
        engine.run_ia_general(3, 3, 3, 2, 20, NV, SEED, FIRST, 4, solver="mmse")
    # every output may be NULL
    assert call_run(engine, make_cfg(), 20, {}) == 0
    engine.sync()
    assert engine.last_kernel() == "ia_general_link f64 D4 pairs"
