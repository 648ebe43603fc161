"""GPU: simulators.GeneralIaSimulator on K = 3, 3 x 3, Ns = 3 with the greedy stream selection -- every Result against the
same quantity accumulated by hand from Engine.run_ia_general(per_realization=True) with reference-style Result.update calls
(apps/ia/simulate_greedy_ia.py:376-439).

Integer state (values, totals, update counts, the histogram) must be equal.  The running sums of ratios are floating-point
sums of at most 150 terms taken in a different order (per batch, pairwise) than the update calls take them: they must agree
to 150 x 2^-52 < 1e-13 relative, which is the bound asserted."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SNR = [10.0, 15.0]
REP, NSYMBS, NS = 150, 20, (3, 3, 3)


def simulate(engine, batch_size):
    from pyphysim_amd.simulators import GeneralIaSimulator
    sim = GeneralIaSimulator(SNR, K=3, Nr=3, Nt=3, Ns=3, solver="max_sinr", stream_selection="greedy", max_iterations=40,
                             modulator="qam", M=16, NSymbs=NSYMBS, rep_max=REP, seed=5, batch_size=batch_size, dtype="f64",
                             demod="mindist", engine=engine)
    sim.simulate()
    return sim


def by_hand(engine, sim, index):
    from pyphysim_amd.simulations import Result
    from pyphysim_amd.simulators import _GOLDEN
    seed = (sim.seed + (index + 1) * _GOLDEN) & 0xFFFFFFFFFFFFFFFF
    nv = 1.0 / 10.0 ** (SNR[index] / 10.0)
    sim._bind()
    _, a = engine.run_ia_general(3, 3, 3, 3, NSYMBS, nv, seed, 0, REP, solver="max_sinr", select="greedy", max_iterations=40,
                                 method=0, dtype="f64", per_realization=True)
    want = {n: Result(n, t) for n, t in (("symbol_errors", Result.SUMTYPE), ("num_symbols", Result.SUMTYPE),
                                         ("bit_errors", Result.SUMTYPE), ("num_bits", Result.SUMTYPE),
                                         ("ber", Result.RATIOTYPE), ("ser", Result.RATIOTYPE),
                                         ("sum_capacity", Result.RATIOTYPE), ("ia_runned_iterations", Result.RATIOTYPE))}
    want["stream_statistics"] = Result("stream_statistics", Result.CHOICETYPE, choice_num=27)
    assert not np.any(a["sym_err"] == 0xFFFFFFFF)          # (a flagged realization would make the simulator run a 151st)
    for i in range(REP):
        ns = a["ns"][i].astype(int)
        num_symbols = NSYMBS * int(ns.sum())
        num_bits = num_symbols * 4
        se, be = int(a["sym_err"][i]), int(a["bit_err"][i])
        want["symbol_errors"].update(se)
        want["num_symbols"].update(num_symbols)
        want["bit_errors"].update(be)
        want["num_bits"].update(num_bits)
        want["ber"].update(be, num_bits)
        want["ser"].update(se, num_symbols)
        want["sum_capacity"].update(float(a["capacity"][i]), 1)
        want["ia_runned_iterations"].update(int(a["iterations"][i]), 1)
        want["stream_statistics"].update(int(np.ravel_multi_index(ns - 1, NS)))
    return want, a


def same(got, want):
    assert got.name == want.name and got.type_code == want.type_code and got.num_updates == want.num_updates
    assert np.array_equal(np.asarray(got._value, dtype=float), np.asarray(want._value, dtype=float)) or \
        abs(got._value - want._value) <= 1e-13 * abs(want._value)            # (sum_capacity: a floating-point sum)
    assert got._total == want._total
    for att in ("_result_sum", "_result_squared_sum"):
        assert abs(getattr(got, att) - getattr(want, att)) <= 1e-13 * abs(getattr(want, att)), (got.name, att)


@pytest.fixture(scope="module")
def sims(engine):
    return simulate(engine, 64), simulate(engine, 150)


def test_results_equal_hand_accumulation(engine, sims):
    sim = sims[0]
    for index in range(len(SNR)):
        want, a = by_hand(engine, sim, index)
        for name, w in want.items():
            assert len(sim.results[name]) == len(SNR)
            same(sim.results[name][index], w)
        stats = sim.results["stream_statistics"][index]
        assert int(stats._value.sum()) == REP == stats.num_updates
        assert np.count_nonzero(stats._value) >= 3                     # the selection really selects
        sent = NSYMBS * a["ns"].sum(axis=1)
        assert sent.min() < sent.max()                                 # num_symbols varies with the selection
        assert sim.results["num_symbols"][index]._value == int(sent.sum())


def test_batch_size_does_not_matter(sims):
    a, b = sims
    names = set(a.results.get_result_names())
    assert names == set(b.results.get_result_names()) and {"ber", "ser", "sum_capacity", "stream_statistics"} <= names
    for name in sorted(names - {"elapsed_time"}):              # (the runner's own wall-clock Result)
        for ra, rb in zip(a.results[name], b.results[name]):
            same(ra, rb)


def test_solver_names():
    from pyphysim_amd.simulators import GeneralIaSimulator
    for solver in ("closed_form", "mmse"):
        with pytest.raises(ValueError, match="'alt_min', 'min_leakage' and 'max_sinr'"):
            GeneralIaSimulator([10.0], solver=solver)
