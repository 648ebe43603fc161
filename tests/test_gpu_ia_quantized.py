"""GPU: the fused limited-feedback IA pipeline mcle_run_ia_quantized (csrc/kernels_quant.hip + csrc/kernels_ia.hip) against the
NumPy restatement under common random numbers (tests/quant_oracle.py), the staged route, split / grid invariance, the draws it
shares with mcle_run_ia, the reference's single realizations (tests/golden/g6_quant_ia.npz) and QuantizedIaSimulator.

Indices follow the gap rule of tests/test_gpu_quantize.py (tolerance from the fixture, a realization with a link inside twice
the tolerance is left out, at most 1 % of the realizations: tests/test_quant_cpu.py asserts the precondition).  Iterative
solvers follow the rule tests/test_gpu_fuzz.py applies to iterative IA: exact outside outage (an eighth or more of the
realization's symbols wrong), max(2, 2 %) symbols and max(8, 4 %) bits inside; complex64 its tolerance on the totals."""
import functools

import numpy as np
import pytest

import quant_oracle as qo
from conftest import load_golden
from oracle import modem as omodem
from pyphysim_amd import _lib, simulators

pytestmark = pytest.mark.gpu

SEED, FIRST, COUNT = qo.PIPE_SEED, qo.PIPE_FIRST, qo.PIPE_COUNT
NSYMBS = 50
NP_DTYPE = {"f64": np.complex128, "f32": np.complex64}


def noise_var(snr_db):
    return 1.0 / float(omodem.dB2Linear(snr_db))


@functools.lru_cache(maxsize=None)
def tolerance(metric, dtype):
    return qo.distance_tolerance(load_golden("g6_quant_ia"), metric, NP_DTYPE[dtype])


@functools.lru_cache(maxsize=None)
def want(solver, metric, dtype, mod="bpsk", M=2, snr_db=15.0, count=COUNT, max_iterations=120):
    """The restatement of the case's realizations (complex128 arithmetic on the codebook as rounded to `dtype`), once."""
    cb = qo.pipeline_codebook(dtype=NP_DTYPE[dtype])
    return [qo.chain(SEED, FIRST + r, cb, metric, solver, mod, M, NSYMBS, snr_db, max_iterations) for r in range(count)]


def set_table(engine, mod, M):
    engine.set_constellation(qo.constellation(mod, M), _lib.CONST_QAM if mod == "qam" else _lib.CONST_GENERIC)


def run(engine, solver, metric, dtype, first=FIRST, count=COUNT, mod="bpsk", M=2, snr_db=15.0, max_iterations=120, cb=None):
    set_table(engine, mod, M)
    cb = qo.pipeline_codebook(dtype=NP_DTYPE[dtype]) if cb is None else cb
    return engine.run_ia_quantized(NSYMBS, noise_var(snr_db), SEED, first, count, cb, metric=metric, dtype=dtype, solver=solver,
                                   max_iterations=max_iterations, per_realization=True)


def compared_realizations(w, metric, dtype):
    tol = tolerance(metric, dtype)
    keep = np.array([bool(np.all(x["gap"] > 2 * tol)) for x in w])
    assert (~keep).sum() <= int(qo.GAP_CAP * len(w))
    return keep


def counts(w):
    se = np.array([x["symbol_errors"] if x["ok"] else 0xFFFFFFFF for x in w], dtype=np.int64)
    be = np.array([x["bit_errors"] if x["ok"] else 0 for x in w], dtype=np.int64)
    return se, be


@pytest.mark.parametrize("metric", qo.METRICS)
@pytest.mark.parametrize("mod,M,snr_db", [("bpsk", 2, 15.0), ("qam", 16, 25.0)])
def test_closed_form_complex128(engine, metric, mod, M, snr_db):
    w = want("closed_form", metric, "f64", mod, M, snr_db)
    res, se, be, cap, its, idx, dsum = run(engine, "closed_form", metric, "f64", mod=mod, M=M, snr_db=snr_db)
    keep = compared_realizations(w, metric, "f64")
    w_idx = np.stack([x["index"] for x in w])
    assert np.array_equal(idx[keep], w_idx[keep])
    w_se, w_be = counts(w)
    ok = np.array([x["ok"] for x in w])
    assert np.array_equal(se[keep].astype(np.int64), w_se[keep]) and np.array_equal(be[keep & ok].astype(np.int64), w_be[keep & ok])
    w_cap = np.array([x["sum_capacity"] if x["ok"] else np.nan for x in w])
    sel = keep & ok
    rel = np.abs(cap[sel] - w_cap[sel]) / np.abs(w_cap[sel])
    print("%s %s: %d of %d realizations compared, %d symbol errors, worst capacity error %.3g"
          % (metric, mod, keep.sum(), COUNT, int(w_se[sel].sum()), rel.max()))
    assert rel.max() <= 1e-9
    w_d = np.array([x["dist"].sum() for x in w])
    assert np.abs(dsum[keep] - w_d[keep]).max() <= 9 * tolerance(metric, "f64")
    assert res["n_realizations"] + res["n_skipped"] == COUNT
    assert res["n_symbols"] == 3 * NSYMBS and res["n_bits"] == 3 * NSYMBS * omodem.level2bits(M)


def check_iterative(se, be, w, keep, dtype, what):
    w_se, w_be = counts(w)
    ok = np.array([x["ok"] for x in w])
    assert np.array_equal(se[keep] == 0xFFFFFFFF, ~ok[keep]), what
    sel = keep & ok
    se, be, w_se, w_be = se[sel].astype(np.int64), be[sel].astype(np.int64), w_se[sel], w_be[sel]
    nsym = 3 * NSYMBS
    outage = w_se >= nsym // 8
    print("%s: %d realizations, %d in outage, symbol errors %d (restatement %d)" % (what, sel.sum(), outage.sum(), se.sum(), w_se.sum()))
    if dtype == "f64":
        assert np.array_equal(se[~outage], w_se[~outage]) and np.array_equal(be[~outage], w_be[~outage]), what
        assert np.all(np.abs(se[outage] - w_se[outage]) <= np.maximum(2, 0.02 * w_se[outage])), what
        assert np.all(np.abs(be[outage] - w_be[outage]) <= np.maximum(8, 0.04 * w_be[outage])), what
    else:
        n, nbits = int(sel.sum()), nsym
        slack_s, slack_b = 0.10 * float(w_se[outage].sum()), 0.25 * float(w_be[outage].sum())
        assert abs(int(se.sum()) - int(w_se.sum())) <= max(3, 1e-4 * n * nsym) + slack_s, what
        assert abs(int(be.sum()) - int(w_be.sum())) <= max(6, 1e-4 * n * nbits) + slack_b, what


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("solver,metric,max_it", [("max_sinr", "euclidean", 120), ("max_sinr", "chordal", 120),
                                                  ("alt_min", "euclidean", 40)])
def test_iterative_solvers(engine, solver, metric, max_it, dtype):
    n = 64
    w = want(solver, metric, dtype, count=n, max_iterations=max_it)
    res, se, be, cap, its, idx, dsum = run(engine, solver, metric, dtype, count=n, max_iterations=max_it)
    tol = tolerance(metric, dtype)
    keep = np.array([bool(np.all(x["gap"] > 2 * tol)) for x in w])
    assert (~keep).sum() <= max(1, int(qo.GAP_CAP * n))
    assert np.array_equal(idx[keep], np.stack([x["index"] for x in w])[keep])
    check_iterative(se, be, w, keep, dtype, "%s %s %s" % (solver, metric, dtype))


@pytest.mark.parametrize("metric", qo.METRICS)
def test_closed_form_complex64(engine, metric):
    w = want("closed_form", metric, "f32")
    res, se, be, cap, its, idx, dsum = run(engine, "closed_form", metric, "f32")
    keep = compared_realizations(w, metric, "f32")
    assert np.array_equal(idx[keep], np.stack([x["index"] for x in w])[keep])
    w_se, w_be = counts(w)
    ok = np.array([x["ok"] for x in w])
    sel = keep & ok
    nsym = 3 * NSYMBS
    outage = w_se[sel] >= nsym // 8
    slack_s, slack_b = 0.02 * float(w_se[sel][outage].sum()), 0.02 * float(w_be[sel][outage].sum())
    print("complex64 %s: symbol errors %d (restatement %d)" % (metric, int(se[sel].sum()), int(w_se[sel].sum())))
    assert abs(int(se[sel].sum()) - int(w_se[sel].sum())) <= max(3, 1e-4 * sel.sum() * nsym) + slack_s
    assert abs(int(be[sel].sum()) - int(w_be[sel].sum())) <= max(6, 1e-4 * sel.sum() * nsym) + slack_b
    w_cap = np.array([x["sum_capacity"] if x["ok"] else np.nan for x in w])
    assert (np.abs(cap[sel] - w_cap[sel]) / np.abs(w_cap[sel])).max() <= 1e-9      # (the solve is complex128 in either arithmetic)


@pytest.mark.parametrize("metric", qo.METRICS)
def test_fused_equals_staged(engine, metric):
    cb = qo.pipeline_codebook()
    nv = noise_var(15.0)
    res, se, be, cap, its, idx, dsum = run(engine, "closed_form", metric, "f64")
    H = engine.randn_c_batch(36, SEED, FIRST, COUNT, dtype="f64").get().reshape(COUNT, 6, 6)
    s_idx, s_Hq, s_dist = engine.quantize_links(H, cb, 3, 2, 2, metric=metric, dtype="f64", with_dist=True)
    assert np.array_equal(s_idx, idx)
    assert np.array_equal(np.cumsum(s_dist.reshape(COUNT, 9), axis=1)[:, -1], dsum)
    sol = engine.ia_closed_form(s_Hq, nv)
    assert np.array_equal(sol["skipped"] != 0, se == 0xFFFFFFFF)
    for r in range(0, COUNT, 7):
        if sol["skipped"][r]:
            continue
        F = [sol["F"][r, k].reshape(2, 1) for k in range(3)]
        U = [sol["U"][r, k].reshape(1, 2) for k in range(3)]
        c = float(np.sum(np.log2(1.0 + qo.true_sinr(H[r], F, U, nv))))
        assert abs(c - cap[r]) <= 1e-9 * abs(c)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("solver", ["closed_form", "max_sinr"])
def test_split_and_grid_invariance(engine, solver, dtype):
    n = 80
    whole = run(engine, solver, "euclidean", dtype, count=n, max_iterations=30)
    for a in (1, 7, 16, 63):
        lo = run(engine, solver, "euclidean", dtype, first=FIRST, count=a, max_iterations=30)
        hi = run(engine, solver, "euclidean", dtype, first=FIRST + a, count=n - a, max_iterations=30)
        for k in range(1, 7):
            assert np.array_equal(np.concatenate([lo[k], hi[k]]), whole[k], equal_nan=True), (a, k)
        for key in ("n_realizations", "n_skipped", "sym_errors", "bit_errors"):
            assert lo[0][key] + hi[0][key] == whole[0][key], (a, key)
    with engine.options(grid_oversub=1):
        one = run(engine, solver, "euclidean", dtype, count=n, max_iterations=30)
    for k in range(1, 7):
        assert np.array_equal(one[k], whole[k], equal_nan=True), k
    assert one[0] == whole[0]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_common_random_numbers_with_run_ia(engine, dtype):
    set_table(engine, "bpsk", 2)
    q = run(engine, "closed_form", "euclidean", dtype)
    p = engine.run_ia(NSYMBS, noise_var(15.0), SEED, FIRST, COUNT, dtype=dtype, solver="closed_form", per_realization=True)
    assert q[0]["n_symbols"] == p[0]["n_symbols"] and q[0]["n_bits"] == p[0]["n_bits"]
    assert q[0]["n_realizations"] + q[0]["n_skipped"] == p[0]["n_realizations"] + p[0]["n_skipped"] == COUNT
    # the drawn big_H, read back through randn_c_batch, is the one both pipelines use: the restatements of both, built on it,
    # reproduce the two pipelines' counts
    H = engine.randn_c_batch(36, SEED, FIRST, 8, dtype="f64").get().reshape(8, 6, 6)
    for r in range(8):
        # (the device's table-based Box-Muller is within an ulp or two of NumPy's libm: not bit for bit)
        assert np.abs(H[r] - qo.draw_big_H(SEED, FIRST + r)).max() <= 1e-14
    if dtype == "f64":
        from oracle import chains
        for r in range(8):
            c = chains.chain_ia(chains.PhiloxRng(SEED, FIRST + r), mod="bpsk", M=2, NSymbs=NSYMBS, snr_db=15.0)
            assert c["symbol_errors"] == p[1][r]
    # quantization costs capacity on the same draws
    assert q[0]["sum_capacity"] < p[0]["sum_capacity"]


def test_singular_quantized_system_is_skipped(engine):
    cb = np.array([[1, 0, 0, 0]], dtype=np.complex128)
    res, se, be, cap, its, idx, dsum = run(engine, "closed_form", "euclidean", "f64", count=64, cb=cb)
    assert res["n_skipped"] == 64 and res["n_realizations"] == 0
    assert np.all(se == 0xFFFFFFFF) and np.all(idx == 0)


def test_argument_rules(engine):
    set_table(engine, "bpsk", 2)
    cb = qo.pipeline_codebook()
    with pytest.raises(ValueError):
        engine.run_ia_quantized(NSYMBS, 0.1, SEED, 0, 4, cb, metric=2)
    with pytest.raises(ValueError):
        engine.run_ia_quantized(NSYMBS, 0.1, SEED, 0, 4, np.ones((8, 9), dtype=complex))
    with pytest.raises(ValueError):
        engine.run_ia_quantized(NSYMBS, 0.1, SEED, 0, 4, np.ones((4097, 4), dtype=complex))


@pytest.mark.parametrize("solver", ["closed_form", "max_sinr"])
def test_fixture_single_realizations_through_the_staged_route(engine, solver):
    """Channel, data and noise injected: quantize_links -> ia_closed_form / ia_iterative -> the staged link operators give the
    reference's decoded arrays and counts."""
    g = load_golden("g6_quant_ia")
    n, nsymbs, max_it = (int(x) for x in g["single_cfg"])
    nv = float(g["noise_var"])
    table = omodem.bpsk_constellation()
    set_table(engine, "bpsk", 2)
    for i in range(n):
        tag = "r%d_%s_" % (i, solver)
        big_H = g[tag + "big_H"]
        idx, Hq = engine.quantize_links(big_H, g["cb0_codebook"], 3, 2, 2, dtype="f64")
        assert np.array_equal(Hq, g[tag + "Hq"])
        if solver == "closed_form":
            sol = engine.ia_closed_form(Hq, nv)
        else:
            sol = engine.ia_iterative(solver, Hq, g[tag + "F_init"], nv, max_iterations=max_it)
            assert int(sol["iterations"][0]) == int(g[tag + "runned_iterations"])
        assert not sol["skipped"][0]
        np.testing.assert_allclose(sol["F"][0], g[tag + "F"], rtol=0, atol=1e-8)
        np.testing.assert_allclose(sol["U"][0], g[tag + "U"], rtol=0, atol=1e-8 * np.abs(g[tag + "U"]).max())
        sym = omodem.modulate(table, g[tag + "idx"])
        X = np.vstack([sol["F"][0, k].reshape(2, 1) @ sym[k:k + 1] for k in range(3)])
        Y = engine.mimo_channel(big_H[None], X[None], noise=g[tag + "noise"][None], noise_var=nv, dtype="f64")[0]
        np.testing.assert_allclose(Y, g[tag + "received"], rtol=0, atol=1e-9)
        est = np.vstack([sol["U"][0, k].reshape(1, 2) @ Y[2 * k:2 * k + 2] for k in range(3)])
        dec = np.asarray(engine.demodulate(est.reshape(-1), dtype="f64")).reshape(3, nsymbs)
        assert np.array_equal(dec, g[tag + "decoded"])
        assert int(np.sum(dec != g[tag + "idx"])) == int(g[tag + "symbol_errors"])
        F = [sol["F"][0, k].reshape(2, 1) for k in range(3)]
        U = [sol["U"][0, k].reshape(1, 2) for k in range(3)]
        np.testing.assert_allclose(np.sum(np.log2(1 + qo.true_sinr(big_H, F, U, nv))), float(g[tag + "sum_capacity"]), rtol=1e-9)


def test_quantized_ia_simulator(engine):
    cb = qo.pipeline_codebook()
    kw = dict(codebook=cb, rep_max=128, batch_size=32, seed=3, dtype="f64", engine=engine, max_iterations=40)
    sim = simulators.QuantizedIaSimulator([10.0, 15.0], **kw)
    sim.simulate()
    names = ("ber", "ser", "sum_capacity", "ia_runned_iterations", "quant_dist")
    for name in names:
        assert len(sim.results[name]) == 2, name
    # ber of a direct call with the same seed
    p = sim.params.get_unpacked_params_list()[1]
    set_table(engine, "bpsk", 2)
    direct = engine.run_ia_quantized(50, noise_var(15.0), sim._seed_for(p), 0, 128, cb, dtype="f64", solver="max_sinr",
                                     max_iterations=40)
    assert direct["n_skipped"] == 0
    assert sim.results["ber"][1].get_result() == direct["bit_errors"] / (direct["n_bits"] * direct["n_realizations"])
    assert abs(sim.results["quant_dist"][1].get_result() - direct["quant_dist"] / (9 * 128)) <= 1e-12
    # two "ranks" through the runner's sharding: every batch split by shard_range, each rank's counters added up with the
    # runner's own _add, the two ranks' sums added (what the one all-reduce per variation does), Results from the total
    assert all(r.get_result() == 0 for r in sim.results["num_skipped_reps"])        # the unsplit run took indices [0, 128)
    for vi, p in enumerate(sim.params.get_unpacked_params_list()):
        local = [None, None]
        for first in range(0, 128, 32):
            for rank in range(2):
                lo, cnt = sim.shard_range(first, 32, rank, 2)
                local[rank] = sim._add(local[rank], sim._run_batch(p, lo, cnt))
        total = sim._add(dict(local[0]), local[1])
        res = sim._results_from_counters(p, total)
        for name in ("ber", "ser", "ia_runned_iterations"):
            assert res[name][0].to_dict() == sim.results[name][vi].to_dict(), name
        for name in ("sum_capacity", "quant_dist"):
            a, b = res[name][0], sim.results[name][vi]
            assert abs(a.get_result() - b.get_result()) <= 1e-12 * abs(b.get_result()) and a.num_updates == b.num_updates
    # quantization costs capacity against the perfect-CSI simulator at the same seed and SNR
    perfect = simulators.IaSimulator([10.0, 15.0], modulator="bpsk", M=2, NSymbs=50, solver="max_sinr", max_iterations=40,
                                     rep_max=128, batch_size=32, seed=3, dtype="f64", engine=engine)
    perfect.simulate()
    for a, b in zip(sim.results["sum_capacity"], perfect.results["sum_capacity"]):
        assert a.get_result() < b.get_result()
    # a Grassmannian codebook of CodebookFinder, reshaped, with the metric that matches it
    from pyphysim_amd.codebooks import CodebookFinder
    finder = CodebookFinder(4, 1, 16, prng_seed=5, engine=engine)
    finder.find_codebook(200)
    gsim = simulators.QuantizedIaSimulator([15.0], codebook=np.asarray(finder.codebook).reshape(16, 4), metric="chordal", rep_max=64,
                                           batch_size=64, seed=3, dtype="f64", engine=engine, max_iterations=20)
    gsim.simulate()
    assert 0.0 < gsim.results["quant_dist"][0].get_result() < 1.0
