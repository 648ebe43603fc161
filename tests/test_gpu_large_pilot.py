"""GPU: the large-array Blast link with pilot-estimated next to perfect channel state (csrc/pipeline_mimo_large_pilot.hip:
mcle_run_mimo_large_pilot, 1 <= Nt <= 8, Nt <= Nr <= 16) against the NumPy restatement under common random numbers
(tests/pilot_link_oracle.py through tests/large_pilot_cases.py), and against the two entry points whose draws it shares:
mcle_run_mimo_large (block 1, every shape) and mcle_run_mimo_pilot_link (both blocks, up to 4 x 4).

tests/test_large_pilot_cpu.py (no GPU) holds what makes "exactly" a fair demand on these very inputs: every realization's smallest
decision gap is >= 1e-9 (5.6e-7), the smallest decision margin is >= 1e3 (7e5) times the difference between the restatement and the
kernels' formulation, the two blocks give other totals in every case (so a kernel that used H twice cannot pass), and the
formulation alone in NumPy complex64 changes 0 decisions.

complex128: per-realization symbol and bit error counts of BOTH blocks equal to the restatement.  complex64: at most 3 symbol
errors of difference in a realization in either block (the bound of tests/test_gpu_mimo_large.py) and the project's bound on the
totals (helpers.check).  |H^ - H|^2 and |H|^2 come from the f64 set-up kernel in either arithmetic: 1e-11 relative, element-wise."""
import ctypes

import numpy as np
import pytest

from oracle import chains
from oracle import modem as omodem

import pilot_link_oracle as po
from helpers import FORMS, check
from large_pilot_cases import CASES, COUNT, FIRST, NAMES, PLAIN, SEED, reference
from pyphysim_amd import _lib, simulators
from pyphysim_amd._lib import McleError

pytestmark = pytest.mark.gpu
DTYPES = [("f64", True), ("f32", False)]
TOL = 1e-11
KIND = {"qam": _lib.CONST_QAM, "bpsk": _lib.CONST_BPSK}
METHOD = {"mindist": _lib.DEMOD_MINDIST, "slicer": _lib.DEMOD_QAM_SLICER}
COUNTERS = ("n_realizations", "n_skipped", "sym_errors", "sym_errors_sq", "bit_errors", "bit_errors_sq")
SKIP = 0xFFFFFFFF


def _args(cfg, method, dtype, kw):
    args = dict(pilot_power=cfg["pilot_power"], alpha=cfg["alpha"], pilots=cfg["pilots"], chan_factor=cfg["L"], cov=cfg["cov"],
                estimator=cfg["estimator"], mmse=cfg["mmse"], method=method, dtype=dtype, per_realization=True)
    args.update(kw)
    return args


def run(engine, cfg, first, count, dtype, seed=None, method=_lib.DEMOD_MINDIST, table=True, **kw):
    if table:
        engine.set_constellation(po.table(), _lib.CONST_QAM)
    return engine.run_mimo_large_pilot_link(cfg["nt"], cfg["nr"], cfg["P"], cfg["n_symbols"], cfg["noise_var"],
                                            cfg["seed"] if seed is None else seed, first, count, **_args(cfg, method, dtype, kw))


def run_small(engine, cfg, first, count, dtype, **kw):
    engine.set_constellation(po.table(), _lib.CONST_QAM)
    return engine.run_mimo_pilot_link(cfg["nt"], cfg["nr"], cfg["P"], cfg["n_symbols"], cfg["noise_var"], cfg["seed"], first, count,
                                      **_args(cfg, _lib.DEMOD_MINDIST, dtype, kw))


def tag_of(cfg, dt):
    nt, nr = cfg["nt"], cfg["nr"]
    return "mimo_large_pilot_link %s %dx%d s%d %s" % (dt, nr, nt, 2 * (-(-nt // 4) - (-nr // 4)), cfg["estimator"])


def worst(got, want):
    return float(np.max(np.abs(got - want) / want))


def same(a, b):
    """two per_realization results: counter blocks, count arrays and err / pow equal bit for bit"""
    return a[0] == b[0] and a[1] == b[1] and all(np.array_equal(a[i], b[i]) for i in (2, 3, 4, 5))


@pytest.mark.parametrize("dt,exact", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_parity_under_common_random_numbers(engine, name, dt, exact):
    cfg, ref = CASES[name], reference(name)
    assert po.err_rounding_bound(cfg, ref) <= 0.5 * TOL and ref["se"].max() > 0
    c_est, c_perf, se, be, err, pw = run(engine, cfg, FIRST, COUNT, dt)
    assert engine.last_kernel() == tag_of(cfg, dt)
    se, be = se.astype(np.int64), be.astype(np.int64)
    assert se.shape == be.shape == (2, COUNT) and err.shape == pw.shape == (COUNT,)
    diff = [int(np.max(np.abs(se[b] - ref["se"][b]))) for b in (0, 1)]
    errs = (worst(err, ref["err"]), worst(pw, ref["pow"]))
    for b in (0, 1):
        print("%s %s block %d: device %d / restatement %d symbol errors, %d / %d bit errors, largest difference in a realization %d"
              % (name, dt, b, se[b].sum(), ref["se"][b].sum(), be[b].sum(), ref["be"][b].sum(), diff[b]))
    print("%s %s err %.3g pow %.3g (element-wise relative)" % ((name, dt) + errs))
    if not exact:
        assert max(diff) <= 3
    for b, cnt in enumerate((c_est, c_perf)):
        check(cnt, se[b], be[b], ref["se"][b], ref["be"][b], ref["n_symbols"], ref["n_bits"], exact)
    assert se[0].sum() != se[1].sum() and be[0].sum() != be[1].sum()          # a kernel that used one filter twice cannot pass
    assert max(errs) <= TOL


@pytest.mark.parametrize("dt,exact", DTYPES)
@pytest.mark.parametrize("name", PLAIN)
def test_perfect_csi_block_is_run_mimo_large(engine, name, dt, exact):
    """L = I, alpha = 1: block 1 is mcle_run_mimo_large on the same (seed, first, count), realization by realization, in EITHER
    arithmetic -- the perfect-CSI record is the one k_mimo_large_setup writes and its products are issued in the same order."""
    cfg = CASES[name]
    c_est, c_perf, se, be, err, pw = run(engine, cfg, FIRST, COUNT, dt)
    large, lse, lbe = engine.run_mimo_large(cfg["nt"], cfg["nr"], cfg["n_symbols"], cfg["noise_var"], SEED, FIRST, COUNT,
                                            mmse=cfg["mmse"], dtype=dt, per_realization=True)
    print(name, dt, "block 1 %d / run_mimo_large %d symbol errors" % (c_perf["sym_errors"], large["sym_errors"]))
    assert large["sym_errors"] > 0
    assert np.array_equal(se[1], lse) and np.array_equal(be[1], lbe) and c_perf == large


@pytest.mark.parametrize("name", ["1x4-p3", "4x4-p9", "mmse-est-1x4"])
def test_up_to_4x4_it_is_the_pilot_link(engine, name):
    cfg = po.ALL_CASES[name]
    big, small = run(engine, cfg, FIRST, COUNT, "f64"), run_small(engine, cfg, FIRST, COUNT, "f64")
    print(name, "symbol errors %d / %d with estimated CSI, %d / %d with perfect CSI; err %.3g pow %.3g"
          % (big[0]["sym_errors"], small[0]["sym_errors"], big[1]["sym_errors"], small[1]["sym_errors"], worst(big[4], small[4]),
             worst(big[5], small[5])))
    assert small[0]["sym_errors"] > 0 and small[0]["sym_errors"] != small[1]["sym_errors"]
    assert big[0] == small[0] and big[1] == small[1]
    assert np.array_equal(big[2], small[2]) and np.array_equal(big[3], small[3])
    assert worst(big[4], small[4]) <= TOL and worst(big[5], small[5]) <= TOL


@pytest.mark.parametrize("dt,exact", DTYPES)
def test_rank_deficient_fixed_pilots_are_skipped_as_the_pilot_link_skips_them(engine, dt, exact):
    """Two equal pilot rows at 2 x 2: s s^H is singular.  mcle_run_mimo_pilot_link finds that once per call on the host (no pivot
    above 1e-12 of the trace) and skips EVERY realization in both blocks: n_realizations 0, n_skipped = count, no errors booked,
    0xFFFFFFFF in every entry of the per-realization arrays.  The same is required here."""
    row = np.exp(2j * np.pi * np.array([0.0, 0.3, 0.55]))
    cfg = dict(po.make_case(2, 2, 3, 6, 16.0), pilots=np.stack([row, row]))
    for got in (run_small(engine, cfg, 0, 9, dt), run(engine, cfg, 0, 9, dt)):
        for cnt in got[:2]:
            assert cnt["n_realizations"] == 0 and cnt["n_skipped"] == 9 and cnt["sym_errors"] == 0 and cnt["bit_errors"] == 0
        assert np.all(got[2] == SKIP) and np.all(got[3] == SKIP) and got[2].shape == (2, 9)
    good = run(engine, dict(cfg, pilots=po.dft_pilots(2, 3, 1.0)), 0, 9, dt)
    assert good[0]["n_realizations"] == 9 and good[0]["n_skipped"] == 0 and not np.any(good[2] == SKIP)


@pytest.mark.parametrize("dt,exact", DTYPES)
def test_split_invariance(engine, dt, exact):
    for name in ("7x9-p12", "mmse-est-1x16", "4x16-p4-dft"):
        cfg = CASES[name]
        whole = run(engine, cfg, 3, 70, dt)
        a, b = run(engine, cfg, 3, 5, dt), run(engine, cfg, 8, 65, dt)
        for i in (2, 3):
            assert np.array_equal(np.concatenate([a[i], b[i]], axis=1), whole[i]), (name, i)
        for i in (4, 5):
            assert np.array_equal(np.concatenate([a[i], b[i]]), whole[i]), (name, i)
        for blk in (0, 1):
            for key in COUNTERS:
                assert a[blk][key] + b[blk][key] == whole[blk][key], (name, blk, key)
        totals = run(engine, cfg, 3, 70, dt, per_realization=False)
        assert len(totals) == 2
        for blk in (0, 1):
            assert totals[blk] == whole[blk]
            assert totals[blk]["sym_errors"] == int(whole[2][blk].sum()) and totals[blk]["bit_errors"] == int(whole[3][blk].sum())
            assert totals[blk]["sym_errors_sq"] == int((whole[2][blk].astype(np.int64) ** 2).sum())


@pytest.mark.parametrize("dt,exact", DTYPES)
def test_grid_invariance(engine, dt, exact):
    """grid_oversub = 1: (2 complex128 | 3 complex64) workgroups of four wavefronts per compute unit, 16 realizations a trip; `count`
    gives every wavefront two or three trips."""
    cfg = po.make_case(5, 6, 7, 2, 16.0, 1.5, True)
    per_trip = engine.n_cu * (2 if exact else 3) * 4 * 16
    count = 2 * per_trip + 37
    with engine.options(grid_oversub=1):
        one = run(engine, cfg, 0, count, dt)
    with engine.options(grid_oversub=8):
        eight = run(engine, cfg, 0, count, dt)
    assert same(one, eight)
    assert one[0]["n_realizations"] == count and one[0]["sym_errors"] > one[1]["sym_errors"] > 0
    for r in (0, per_trip - 1, per_trip, 2 * per_trip + 5, count - 1):
        want = po.run(cfg, r, 1)
        if exact:
            assert np.array_equal(one[2][:, r], want["se"][:, 0]) and np.array_equal(one[3][:, r], want["be"][:, 0]), r
        assert worst(one[4][r:r + 1], want["err"]) <= TOL and worst(one[5][r:r + 1], want["pow"]) <= TOL, r


def test_a_run_across_a_record_slice_equals_its_halves(engine):
    """8 x 16 in complex128: two records of 12 steps x 64 lanes x 8 bytes = 12 KiB per realization, 10 922 realizations per
    128 MiB slice; 12 000 realizations take two."""
    cfg = po.make_case(8, 16, 8, 2, 8.0)
    count = 12000
    assert (128 << 20) // (2 * 12 * 64 * 8) == 10922 < count
    whole = run(engine, cfg, 5, count, "f64")
    a, b = run(engine, cfg, 5, count // 2, "f64"), run(engine, cfg, 5 + count // 2, count // 2, "f64")
    for i in (2, 3):
        assert np.array_equal(np.concatenate([a[i], b[i]], axis=1), whole[i]), i
    for i in (4, 5):
        assert np.array_equal(np.concatenate([a[i], b[i]]), whole[i]), i
    for blk in (0, 1):
        for key in COUNTERS:
            assert a[blk][key] + b[blk][key] == whole[blk][key], (blk, key)
        assert whole[blk]["n_realizations"] == count and whole[blk]["n_skipped"] == 0
    assert whole[0]["sym_errors"] > whole[1]["sym_errors"] > 0
    for r in (10921, 10922, count - 1):                           # each side of the slice edge, the last one
        want = po.run(cfg, 5 + r, 1)
        assert np.array_equal(whole[2][:, r], want["se"][:, 0]) and np.array_equal(whole[3][:, r], want["be"][:, 0]), r
        assert worst(whole[4][r:r + 1], want["err"]) <= TOL, r


@pytest.mark.parametrize("dt,exact", DTYPES)
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f[0])
def test_every_decision_form(engine, form, dt, exact):
    """5 x 6 through every decision form of the large link (slicer, certificates, candidate grid, plain search; 64-QAM also with the
    certificates off).  tests/test_gpu_mimo_large.py holds every form of the large link to the oracle; here block 1 must BE that
    link in each form, in either arithmetic, and the forms that test holds to the same oracle in complex128 -- slicer and
    min-distance on 16-QAM, certificates on and off -- must give the same counts in both blocks."""
    _id, mod, M, method, snr = form
    cfg = po.make_case(5, 6, 7, 51, snr)
    engine.set_constellation(chains.constellation(mod, M), KIND.get(mod, _lib.CONST_GENERIC))
    bits = int(np.log2(M))

    def both():
        got = run(engine, cfg, FIRST, COUNT, dt, method=METHOD[method], table=False)
        large = engine.run_mimo_large(5, 6, 51, cfg["noise_var"], SEED, FIRST, COUNT, method=METHOD[method], dtype=dt,
                                      per_realization=True)
        print(_id, dt, "symbol errors: estimated %d, perfect %d, run_mimo_large %d"
              % (got[0]["sym_errors"], got[1]["sym_errors"], large[0]["sym_errors"]))
        assert got[1] == large[0] and np.array_equal(got[2][1], large[1]) and np.array_equal(got[3][1], large[2])
        assert got[0]["n_symbols"] == 5 * 51 and got[0]["n_bits"] == 5 * 51 * bits and got[0]["n_skipped"] == 0
        assert got[0]["sym_errors"] > got[1]["sym_errors"] > 0
        return got

    got = both()
    if M == 64:
        with engine.options(demod_nocert=1):
            plain = both()
        if exact:
            assert same(got, plain)
    if _id == "qam16-slicer" and exact:
        engine.set_constellation(chains.constellation(mod, M), KIND[mod])
        assert same(got, run(engine, cfg, FIRST, COUNT, dt, method=_lib.DEMOD_MINDIST, table=False))


def test_every_argument_rule_is_refused(engine):
    ok = CASES["7x9-p12"]
    run(engine, ok, 0, 4, "f64")
    assert engine.last_kernel() == tag_of(ok, "f64")

    def refused(word, **kw):
        run(engine, ok, 0, 4, "f64")
        with pytest.raises((McleError, ValueError), match=word):
            run(engine, dict(ok, **kw), 0, 4, "f64")
        assert engine.last_kernel() == ""

    refused("antenna counts", nt=9, nr=9, P=12)
    refused("antenna counts", nr=17)
    refused("antenna counts", nr=6)
    refused("antenna counts", nt=0)
    refused("n_pilots must be", P=6)
    refused("n_pilots must be", P=257)
    refused("n_symbols", n_symbols=0)
    refused("needs nt = 1", nt=2, nr=9, estimator="mmse", cov=np.eye(9))
    refused("needs d_mmse_matrix", nt=1, estimator="mmse", cov=None)
    refused("Noise variance", noise_var=-0.5)
    refused("Noise variance", noise_var=float("nan"))
    refused("pilot_power", pilot_power=0.0)
    refused("alpha", alpha=float("inf"))
    refused("draw positions are 32-bit", nr=16, n_symbols=2 ** 27)
    run(engine, ok, 0, 4, "f64")
    with pytest.raises((McleError, ValueError), match="at most 2\\^31-1"):
        run(engine, ok, 0, 2 ** 31, "f64", per_realization=False)
    assert engine.last_kernel() == ""
    run(engine, ok, 0, 4, "f32")
    assert engine.last_kernel() == tag_of(ok, "f32")


def test_a_refused_call_leaves_the_outputs_untouched(engine):
    """Every refusal straight through the C ABI with sentinel-filled outputs (fixed pilots without d_pilots is a call Engine cannot
    express): MCLE_E_INVAL, a message naming the rule, last_kernel cleared, no byte of any output changed.  count = 0 is no
    refusal and launches nothing either."""
    engine.set_constellation(po.table(), _lib.CONST_QAM)
    n = 8
    size = ctypes.sizeof(_lib.Counters)
    bufs = dict(cnt=engine.to_device(np.full(2 * size, 0xA5, np.uint8)), se=engine.to_device(np.full((2, n), 12345, np.uint32)),
                be=engine.to_device(np.full((2, n), 54321, np.uint32)), err=engine.to_device(np.full(n, -7.0)),
                pw=engine.to_device(np.full(n, -9.0)))
    before = {k: v.get().copy() for k, v in bufs.items()}
    pilots = engine.to_device(po.dft_pilots(8, 256, 1.0), np.complex128)           # large enough for every shape tried
    matrix = engine.to_device(np.eye(16), np.complex128)
    base = dict(nt=7, nr=9, P=12, n_symbols=34, estimator=0, random_pilots=1, noise_var=0.1, pilot_power=1.0, alpha=1.0)

    def call(count=n, d_pilots=None, d_B=None, **kw):
        c = dict(base, **kw)
        cfg = _lib.MimoPilotCfg(c["nt"], c["nr"], c["P"], c["n_symbols"], _lib.DEMOD_MINDIST, c["estimator"], c["random_pilots"], 0,
                                c["noise_var"], c["pilot_power"], c["alpha"])
        return engine.lib.mcle_run_mimo_large_pilot(engine.ctx, _lib.dtype_code("f64"), ctypes.byref(cfg), SEED, 0, count, d_pilots,
                                                    None, d_B, bufs["cnt"].ptr, bufs["se"].ptr, bufs["be"].ptr, bufs["err"].ptr,
                                                    bufs["pw"].ptr)

    def untouched():
        return all(np.array_equal(v.get(), before[k]) for k, v in bufs.items())

    rules = [(b"antenna counts", dict(nt=9, nr=9)), (b"antenna counts", dict(nr=17)), (b"antenna counts", dict(nr=6)),
             (b"n_pilots must be", dict(P=6)), (b"n_pilots must be", dict(P=257)), (b"n_symbols", dict(n_symbols=0)),
             (b"needs nt = 1", dict(nt=2, estimator=1, d_B=matrix.ptr)), (b"needs d_mmse_matrix", dict(nt=1, estimator=1)),
             (b"d_pilots", dict(random_pilots=0)), (b"Noise variance", dict(noise_var=-0.5)),
             (b"Noise variance", dict(noise_var=float("nan"))), (b"pilot_power", dict(pilot_power=0.0)),
             (b"alpha", dict(alpha=float("nan"))), (b"draw positions are 32-bit", dict(nr=16, n_symbols=2 ** 27)),
             (b"at most 2^31-1", dict(count=2 ** 31))]
    for word, kw in rules:
        assert call() == 0 and engine.last_kernel() == "mimo_large_pilot_link f64 9x7 s10 ls"
        for k, v in bufs.items():
            v.set(before[k])
        assert call(**kw) == -1, kw
        assert word in engine.lib.mcle_last_error(), (kw, engine.lib.mcle_last_error())
        assert engine.last_kernel() == "" and untouched(), kw
    assert call(count=0) == 0 and engine.last_kernel() == "" and untouched()
    assert call(d_pilots=pilots.ptr, random_pilots=0, P=256) == 0
    assert engine.last_kernel() == "mimo_large_pilot_link f64 9x7 s10 ls"
    se = bufs["se"].get()
    assert not np.any(se == 12345) and se.max() <= 7 * 34


def test_zero_realizations_return_zero_counters(engine):
    cfg = CASES["5x6-p5-dft"]
    run(engine, cfg, 0, 4, "f64")
    c_est, c_perf, se, be, err, pw = run(engine, cfg, 0, 0, "f64")
    assert se.shape == be.shape == (2, 0) and err.shape == pw.shape == (0,)
    assert not any(c_est.values()) and not any(c_perf.values()) and engine.last_kernel() == ""


def test_simulator(engine):
    kw = dict(Nt=4, Nr=16, num_pilots=8, NSymbs=50, rep_max=300, seed=11, dtype="f64", engine=engine, common_random_numbers=True)
    small = simulators.LargePilotMimoSimulator(SNR=[6, 12], batch_size=64, **kw)
    small.simulate()
    assert engine.last_kernel() == "mimo_large_pilot_link f64 16x4 s10 ls"
    big = simulators.LargePilotMimoSimulator(SNR=[6, 12], batch_size=300, **kw)
    big.simulate()
    names = ("ber", "ser", "ber_perfect_csi", "ser_perfect_csi", "mse", "channel_power")
    get = small.results.get_result_values_list
    assert isinstance(small, simulators.PilotMimoSimulator) and set(small.results.get_result_names()) >= set(names)
    for name in names:
        assert big.results.get_result_values_list(name) == get(name), name
    large = simulators.LargeMimoSimulator(SNR=[6, 12], Nt=4, Nr=16, NSymbs=50, rep_max=300, seed=11, dtype="f64", engine=engine,
                                          common_random_numbers=True, batch_size=300)
    large.simulate()
    print("ser %s, with perfect CSI %s, LargeMimoSimulator %s" % (get("ser"), get("ser_perfect_csi"),
                                                                  large.results.get_result_values_list("ser")))
    assert get("ser_perfect_csi") == large.results.get_result_values_list("ser")
    assert get("ber_perfect_csi") == large.results.get_result_values_list("ber")
    for i, snr in enumerate((6.0, 12.0)):
        assert get("ser")[i] > get("ser_perfect_csi")[i] > 0
        engine.set_constellation(po.table(), _lib.CONST_QAM)
        c_est, c_perf = engine.run_mimo_large_pilot_link(4, 16, 8, 50, 1.0 / float(omodem.dB2Linear(snr)), 11, 0, 300,
                                                         method=small.demod_method, dtype="f64")
        assert get("ser")[i] == c_est["sym_errors"] / (300 * 200) and get("ser_perfect_csi")[i] == c_perf["sym_errors"] / (300 * 200)
    assert get("mse")[0] > get("mse")[1] > 0
    for bad in (dict(Nt=9, Nr=9), dict(Nt=4, Nr=17), dict(Nt=5, Nr=4), dict(Nt=0, Nr=4)):
        with pytest.raises(ValueError, match="1 <= Nt <= 8 and Nt <= Nr <= 16"):
            simulators.LargePilotMimoSimulator(SNR=[6.0], engine=engine, **bad)
    with pytest.raises(ValueError, match="Nt = 1"):
        simulators.LargePilotMimoSimulator(SNR=[6.0], Nt=2, Nr=8, C=np.eye(8), estimator="mmse", engine=engine)
    with pytest.raises((McleError, ValueError), match="nt <= nr"):                  # the 4 x 4 entry point keeps its envelope
        engine.run_mimo_pilot_link(4, 16, 8, 50, 0.1, 11, 0, 8)
