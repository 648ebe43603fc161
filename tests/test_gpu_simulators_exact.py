"""GPU: simulate() of the nine first-generation simulators against the oracle chains, count by count.

The kernels behind these simulators are held to the oracle through Engine.run_* with arguments the tests build themselves;
this file holds what the simulator does between its constructor and that call and between the counters and the Results: the SNR
-> noise variance (BdSimulator: -> transmit power) map, the seed of a parameter variation (tests/simulator_cases.py states the
rule of DESIGN.md section 4 on its own), discretize_profile on the constructor's profile and its defaults, num_used_subcarriers or
fft_size, demod="auto", first_rep from batch to batch and the ragged last batch, MimoOfdmTdlSimulator's fused / staged choice,
IaSimulator's sums, and the device's sums of squares on their way into the Results.

Every case is tests/simulator_cases.py's: 37 realizations in batches of 16 at two SNR points, the oracle computed once per case
and shared.  tests/test_simulator_cases_cpu.py (no GPU) holds the conditions that make "equal" a fair demand in complex128 (no
decision within 1e-9 of a border) and that fail a simulator which ignores the variation index, the SNR or first_rep.

complex128 with demod="mindist": every integer equal.  The default dtype (complex64) with the default demodulator: the
project's bound for complex64, helpers.check(exact=False) -- totals within 1e-4 of the symbols / bits of the complex128 oracle;
each case prints its difference before it asserts (measured on an MI355X: 0 symbols and 0 bits in all 23 cases at both points).

'ia_runned_iterations' is held EXACTLY: tests/test_gpu_pipelines.py::test_ia_iterative_pipeline holds the per-realization
iteration counts of ('max_sinr', 'random') exactly, in both dtypes, so the mean of 37 of them is a quotient of equal integers.
'sum_capacity' to 1e-9 relative, the bound tests/test_gpu_ia_base.py holds a capacity to."""
import numpy as np
import pytest

import simulator_cases as sc
from pyphysim_amd import simulators

pytestmark = pytest.mark.gpu

COUNT_NAMES = {"symbol_errors", "num_symbols", "bit_errors", "num_bits", "ber", "ser", "elapsed_time", "num_skipped_reps"}


def make(engine, name, cls=None, **over):
    """The simulator of a case: complex128 and demod='mindist' unless `over` says otherwise (None: the constructor's default)."""
    cfg = sc.CASES[name]
    kw = dict(SNR=list(cfg["snr"]), seed=cfg["seed"], rep_max=sc.REP_MAX, batch_size=sc.BATCH, engine=engine, dtype="f64",
              demod="mindist")
    kw.update(cfg["ctor"])
    kw.update(over)
    kw = {k: v for k, v in kw.items() if v is not None}
    return (cls or getattr(simulators, cfg["sim"]))(**kw)


def totals(sim, i):
    get = lambda key: sim.results[key][i].get_result()
    return dict(se=get("symbol_errors"), be=get("bit_errors"), nsym=get("num_symbols"), nbits=get("num_bits"))


def check_counts(sim, refs, n_reps=None):
    """Every integer Result of every SNR point equal to the oracle's totals over the first n_reps[i] realizations (default: all
    37), the ratios equal to the quotients of those integers, nothing skipped."""
    n_reps = n_reps or [sc.REP_MAX] * len(refs)
    assert sim.runned_reps == list(n_reps) and COUNT_NAMES <= set(sim.results.get_result_names())
    for i, (ref, n) in enumerate(zip(refs, n_reps)):
        se, be = int(ref["se"][:n].sum()), int(ref["be"][:n].sum())
        got = totals(sim, i)
        assert got == dict(se=se, be=be, nsym=n * ref["nsym"], nbits=n * ref["nbits"]), (i, got, se, be)
        assert sim.results["ser"][i].get_result() == se / (n * ref["nsym"])
        assert sim.results["ber"][i].get_result() == be / (n * ref["nbits"])
        for key in ("symbol_errors", "num_symbols", "bit_errors", "num_bits", "ber", "ser"):
            assert sim.results[key][i].num_updates == n, key
        assert sim.results["num_skipped_reps"][i].get_result() == 0


@pytest.mark.parametrize("name", sc.NAMES)
def test_simulate_equals_the_oracle(engine, name, monkeypatch):
    cfg, refs = sc.CASES[name], sc.reference(name)
    sim = make(engine, name)
    fused_calls = []
    if cfg["sim"] == "MimoOfdmTdlSimulator":
        inner = engine.run_mimo_ofdm_tdl

        def served(*args, **kw):                       # (first_rep, count) of every call the fused entry point served
            out = inner(*args, **kw)
            fused_calls.append(tuple(args[10:12]))
            return out
        monkeypatch.setattr(engine, "run_mimo_ofdm_tdl", served)
    sim.simulate()
    check_counts(sim, refs)
    if cfg["sim"] == "MimoOfdmTdlSimulator":
        # 'auto': the fused kernel serves this configuration, batch by batch; False: the staged chain, never the fused entry
        batches = [(0, 16), (16, 16), (32, 5)]
        assert fused_calls == (batches * 2 if cfg["ctor"]["fused"] == "auto" else [])
        monkeypatch.undo()
    for i, (p, ref) in enumerate(zip(sim.params.get_unpacked_params_list(), refs)):
        assert p["SNR"] == cfg["snr"][i] and p.unpack_index == i
        # the device's sums of squares, through the batches, in the Results: those of one update per realization
        want = sc.sequential_results(ref)
        for key in ("ser", "ber", "symbol_errors"):
            sc.assert_same_statistics(sim.results[key][i], want[key])
        if cfg["detailed"]:
            c, se, be = sim._run_batch_detailed(p, 0, sc.REP_MAX)
            assert np.array_equal(se, ref["se"]) and np.array_equal(be, ref["be"])
            assert c["n_realizations"] == sc.REP_MAX and c["n_skipped"] == 0
            assert c["n_symbols"] == ref["nsym"] and c["n_bits"] == ref["nbits"]
            assert c["sym_errors_sq"] == int((ref["se"] ** 2).sum()) and c["bit_errors_sq"] == int((ref["be"] ** 2).sum())
            _, se_tail, be_tail = sim._run_batch_detailed(p, 32, 5)
            assert np.array_equal(se_tail, ref["se"][32:]) and np.array_equal(be_tail, ref["be"][32:])
        if cfg["sim"] == "IaSimulator":
            cap = sim.results["sum_capacity"][i]
            mean = float(np.mean(ref["cap"]))
            print("%s at %g dB: sum capacity %.12g, oracle %.12g" % (name, cfg["snr"][i], cap.get_result(), mean))
            assert cap.num_updates == sc.REP_MAX and abs(cap.get_result() - mean) <= 1e-9 * mean
            var = float(np.mean(ref["cap"] ** 2) - mean ** 2)
            assert abs(cap.get_result_var() - var) <= 1e-9 * float(np.mean(ref["cap"] ** 2))
            names = sim.results.get_result_names()
            assert ("ia_runned_iterations" in names) == (ref["its"] is not None)
            if ref["its"] is not None:
                its = sim.results["ia_runned_iterations"][i]
                assert its.num_updates == sc.REP_MAX and its.get_result() == int(ref["its"].sum()) / sc.REP_MAX
                assert its.to_dict()["result_squared_sum"] == int((ref["its"] ** 2).sum())


@pytest.mark.parametrize("name", sc.CRN)
def test_common_random_numbers(engine, name):
    """common_random_numbers=True: every SNR point on the base seed itself."""
    refs = sc.reference(name, True)
    sim = make(engine, name, common_random_numbers=True)
    sim.simulate()
    check_counts(sim, refs)
    if sc.CASES[name]["sim"] == "IaSimulator":
        for i, ref in enumerate(refs):
            assert sim.results["ia_runned_iterations"][i].get_result() == int(ref["its"].sum()) / sc.REP_MAX


@pytest.mark.parametrize("name", sc.QAM)
def test_demod_auto_is_the_slicer_and_gives_the_same_totals(engine, name):
    from pyphysim_amd import _lib
    sim = make(engine, name, demod=None)
    assert sim.demod_method == _lib.DEMOD_QAM_SLICER
    sim.simulate()
    check_counts(sim, sc.reference(name))


def test_demod_auto_of_the_other_modulations_is_the_minimum_distance():
    from pyphysim_amd import _lib
    for name in sc.NAMES:
        if name not in sc.QAM:
            assert make(None, name, demod=None).demod_method == _lib.DEMOD_MINDIST, name


@pytest.mark.parametrize("name", sc.NAMES)
def test_the_default_dtype_stays_inside_the_complex64_bound(engine, name):
    refs = sc.reference(name)
    sim = make(engine, name, dtype=None, demod=None)
    assert sim.dtype == "f32"
    sim.simulate()
    assert sim.runned_reps == [sc.REP_MAX] * 2
    for i, ref in enumerate(refs):
        got = totals(sim, i)
        d_se, d_be = got["se"] - int(ref["se"].sum()), got["be"] - int(ref["be"].sum())
        print("%s at %g dB, complex64: symbol errors %d (oracle %d, %+d = %.2g of the symbols), bit errors %d (oracle %d, %+d = "
              "%.2g of the bits)" % (name, sc.CASES[name]["snr"][i], got["se"], ref["se"].sum(), d_se,
                                     d_se / (sc.REP_MAX * ref["nsym"]), got["be"], ref["be"].sum(), d_be,
                                     d_be / (sc.REP_MAX * ref["nbits"])))
        assert got["nsym"] == sc.REP_MAX * ref["nsym"] and got["nbits"] == sc.REP_MAX * ref["nbits"]
        assert sim.results["num_skipped_reps"][i].get_result() == 0 and sim.results["ser"][i].num_updates == sc.REP_MAX
        assert abs(d_se) / (sc.REP_MAX * ref["nsym"]) <= 1e-4 and abs(d_be) / (sc.REP_MAX * ref["nbits"]) <= 1e-4
        assert sim.results["ser"][i].get_result() == got["se"] / got["nsym"]


@pytest.mark.parametrize("name", sc.EARLY_STOP)
def test_exact_early_stop_runs_the_oracles_prefix(engine, name):
    """exact_early_stop=True with a rule that stops at half the oracle's symbol errors: the realizations up to and including the
    first whose running total reaches the threshold, whatever the batch size."""
    cfg, refs = sc.CASES[name], sc.reference(name)
    threshold = {snr: int(ref["se"].sum()) // 2 for snr, ref in zip(cfg["snr"], refs)}
    n_reps = [sc.stop_prefix(ref, threshold[snr]) for snr, ref in zip(cfg["snr"], refs)]

    class Stop(getattr(simulators, cfg["sim"])):
        def _keep_going(self, params, results, rep):
            return results["symbol_errors"][-1].get_result() < threshold[float(params["SNR"])]

    runs = []
    for batch_size in (8, 1000):
        sim = make(engine, name, cls=Stop, batch_size=batch_size, exact_early_stop=True)
        sim.simulate()
        check_counts(sim, refs, n_reps)
        for i, ref in enumerate(refs):
            want = sc.sequential_results(dict(ref, se=ref["se"][:n_reps[i]], be=ref["be"][:n_reps[i]]))
            for key in ("ser", "ber", "symbol_errors"):
                sc.assert_same_statistics(sim.results[key][i], want[key])
        runs.append((sim.runned_reps, [sim.results[key][i].to_dict() for key in ("symbol_errors", "bit_errors", "ser", "ber")
                                       for i in range(2)]))
    assert runs[0] == runs[1]


@pytest.mark.parametrize("batch_size", sc.OTHER_BATCHES)
@pytest.mark.parametrize("name", sc.NAMES)
def test_batch_size_invariance(engine, name, batch_size):
    """One batch of 37, and seven of 5 with a ragged one of 2: the totals, and the sums of squares, of batches of 16."""
    refs = sc.reference(name)
    sim = make(engine, name, batch_size=batch_size)
    sim.simulate()
    check_counts(sim, refs)
    for i, ref in enumerate(refs):
        sc.assert_same_statistics(sim.results["symbol_errors"][i], sc.sequential_results(ref)["symbol_errors"])


def test_the_tdl_case_is_f1_of_the_simulator_tests():
    from test_gpu_simulators import F1_KW
    assert {k: v for k, v in F1_KW.items() if k != "snr_db"} == sc.F1
