"""The nine first-generation simulators of pyphysim_amd/simulators.py (AwgnSimulator, FlatFadingSimulator, OfdmTdlSimulator,
MimoOfdmSimulator, MimoSimulator, LargeMimoSimulator, BdSimulator, IaSimulator, MimoOfdmTdlSimulator) held to the oracle chains
(oracle/chains.py) count by count: the cases shared by test_simulator_cases_cpu.py (CPU: the conditions on the inputs) and
test_gpu_simulators_exact.py (GPU: simulate() itself).  TEST INFRASTRUCTURE.

What is under test is the layer between a simulator's constructor and its Engine.run_* call and between the counters and the
Results, so every case states in its own words what that layer has to hand on: the chain's keyword arguments next to the
constructor's (tap delays in samples next to seconds, the default profiles and sizes written out), the noise variance or transmit
power of an SNR point, and the seed of a parameter variation.

Seed rule (stated here on its own): variation i of the unpacked SNR list runs on

    seed_i = (seed + (i + 1) * 0x9E3779B97F4A7C15) mod 2^64

and with common_random_numbers=True every variation runs on `seed` itself.  Realization r of variation i is then
chain(PhiloxRng(seed_i, r), ...) for r = 0 .. rep_max - 1.

Every case: seed 7 (13 for Alamouti, see there), rep_max 37, batch_size 16 -- two full batches and a ragged one of 5, first_rep 0,
16 and 32 -- and two SNR points.  The shapes are the smallest at which this layer can still go wrong: no kernel edge is looked for here (the pipelines'
own tests do that through Engine.run_*)."""
import functools

import numpy as np

SEED, REP_MAX, BATCH = 7, 37, 16
OTHER_BATCHES = (37, 5)          # one batch; seven full batches and a ragged one of 2

_TS_LTE = 1.0 / (15e3 * 1024)
_PATHLOSS = ((1.0, 0.2, 0.05), (0.3, 1.0, 0.1), (0.02, 0.4, 1.0))
# tests/test_gpu_simulators.py::F1_KW with the SNR taken out (the GPU file checks that the two agree)
F1 = dict(mod="qam", M=16, nt=2, nr=2, fft_size=64, cp_size=16, num_used=52, n_ofdm_sym=2, Fd=50.0, Ts=1e-6, L=8,
          tap_powers_dB=(0.0, -4.0, -9.0), tap_delays_samples=(0, 2, 5))
_F1_CTOR = dict(modulator="qam", M=16, Nt=2, Nr=2, fft_size=64, cp_size=16, num_used_subcarriers=52, num_ofdm_symbols=2, Fd=50.0,
                Ts=1e-6, L=8, tap_powers_dB=(0.0, -4.0, -9.0), tap_delays=(0.0, 2e-6, 5e-6))


def variation_seed(seed, index, common_random_numbers=False):
    """The seed of variation `index` (module docstring)."""
    if common_random_numbers:
        return seed
    return (seed + (index + 1) * 0x9E3779B97F4A7C15) % (1 << 64)


def _snr(snr_db):
    return dict(snr_db=snr_db)


def _bd_power(noise_var, path_loss_border):
    """apps/comp_BD/simulate_comp_simple.py: the noise power is fixed, SNR sets the transmit power."""
    return lambda snr_db: dict(iPu=10.0 ** (snr_db / 10.0) * noise_var / path_loss_border, noise_var=noise_var)


def _case(sim, ctor, chain, kw, snr, decided="est", point=_snr, seed=SEED, detailed=True):
    return dict(sim=sim, ctor=ctor, chain=chain, kw=kw, snr=snr, decided=decided, point=point, seed=seed, detailed=detailed)


def _mimo(scheme, nt, nr, seed=SEED):
    return _case("MimoSimulator", dict(scheme=scheme, modulator="psk", M=4, Nt=nt, Nr=nr, NSymbs=50), "chain_mimo_scheme",
                 dict(scheme=scheme, mod="psk", M=4, nt=nt, nr=nr, NSymbs=50, canonical=True), (5.0, 12.0), seed=seed)


# name: simulator class, constructor arguments (next to SNR, seed, rep_max, batch_size, dtype, demod), oracle chain, its
# arguments, the two SNR points, the key of the decided values, what an SNR point becomes in the chain's arguments
CASES = {
    "awgn-qam16": _case("AwgnSimulator", dict(modulator="qam", M=16, NSymbs=1000), "chain_awgn", dict(mod="qam", M=16, N=1000),
                        (6.0, 12.0), "rx"),
    "awgn-psk8": _case("AwgnSimulator", dict(modulator="psk", M=8, NSymbs=1000), "chain_awgn", dict(mod="psk", M=8, N=1000),
                       (6.0, 12.0), "rx"),
    # (BPSK makes no error in 37 000 symbols at 12 dB: 0 and 6 dB)
    "awgn-bpsk": _case("AwgnSimulator", dict(modulator="bpsk", M=2, NSymbs=1000), "chain_awgn", dict(mod="bpsk", M=2, N=1000),
                       (0.0, 6.0), "rx"),
    "flat-jakes": _case("FlatFadingSimulator", dict(modulator="qam", M=64, NSymbs=5000, Fd=100.0, Ts=1e-3, L=8),
                        "chain_flat_jakes", dict(mod="qam", M=64, N=5000, Fd=100.0, Ts=1e-3, L=8), (10.0, 25.0), "eq"),
    "flat-rayleigh": _case("FlatFadingSimulator", dict(modulator="qam", M=16, NSymbs=1000, rayleigh_iid=True),
                           "chain_flat_rayleigh", dict(mod="qam", M=16, N=1000, form="suchannel"), (10.0, 20.0), "eq"),
    # the constructor's defaults, written out on the oracle's side
    "ofdm-tdl-defaults": _case("OfdmTdlSimulator", dict(), "chain_ofdm_tdl",
                               dict(mod="qpsk", M=4, fft_size=1024, cp_size=16, num_used=1024, n_ofdm_sym=1, Fd=10.0, Ts=_TS_LTE,
                                    L=8, tap_powers_dB=(0.0, -3.0, -6.0, -9.0, -12.0), tap_delays_samples=(0, 1, 2, 3, 4)),
                               (10.0, 20.0), "eq"),
    "ofdm-tdl-256": _case("OfdmTdlSimulator",
                          dict(fft_size=256, cp_size=8, num_used_subcarriers=200, num_ofdm_symbols=2,
                               tap_powers_dB=(0.0, -4.0, -9.0), tap_delays=(0.0, 3 * _TS_LTE, 11 * _TS_LTE)), "chain_ofdm_tdl",
                          dict(mod="qpsk", M=4, fft_size=256, cp_size=8, num_used=200, n_ofdm_sym=2, Fd=10.0, Ts=_TS_LTE, L=8,
                               tap_powers_dB=(0.0, -4.0, -9.0), tap_delays_samples=(0, 3, 11)), (10.0, 20.0), "eq"),
    "mimo-ofdm-defaults": _case("MimoOfdmSimulator", dict(), "chain_mimo_ofdm",
                                dict(mod="qam", M=64, nt=4, nr=4, fft_size=1024, cp_size=16, num_used=1024, n_ofdm_sym=1,
                                     mmse=True), (15.0, 25.0)),
    "mimo-ofdm-2x3-zf": _case("MimoOfdmSimulator",
                              dict(modulator="qam", M=16, Nt=2, Nr=3, fft_size=256, mmse=False, num_used_subcarriers=200),
                              "chain_mimo_ofdm",
                              dict(mod="qam", M=16, nt=2, nr=3, fft_size=256, cp_size=16, num_used=200, n_ofdm_sym=1, mmse=False),
                              (10.0, 20.0)),
    "mimo-blast-2x2": _mimo("blast", 2, 2),
    # (diversity 4: with seed 7 the chain makes no error in the 1850 symbols at 12 dB.  Seed 13 is the first after 7 at which it
    # makes one at both points, with and without common random numbers: 38 and 1, 63 and 3)
    "mimo-alamouti-2x2": _mimo("alamouti", 2, 2, seed=13),
    "mimo-mrc-1x2": _mimo("mrc", 1, 2),
    "mimo-mrt-2x1": _mimo("mrt", 2, 1),
    "mimo-svd-2x2": _mimo("svd", 2, 2),
    "mimo-gmd-2x2": _mimo("gmd", 2, 2),
    "mimo-blast-3x4-mmse": _case("MimoSimulator", dict(scheme="blast", modulator="qam", M=16, Nt=3, Nr=4, NSymbs=51, mmse=True),
                                 "chain_mimo_scheme",
                                 dict(scheme="blast", mod="qam", M=16, nt=3, nr=4, NSymbs=51, mmse=True, canonical=True),
                                 (6.0, 14.0)),
    "large-mimo-5x6": _case("LargeMimoSimulator", dict(Nt=5, Nr=6, modulator="qam", M=16, NSymbs=51), "chain_mimo_scheme",
                            dict(scheme="blast", mod="qam", M=16, nt=5, nr=6, NSymbs=51), (8.0, 14.0)),
    "bd": _case("BdSimulator", dict(modulator="psk", M=4, K=3, Nr=2, NSymbs=51, noise_var=1e-3, path_loss_border=1.0,
                                    waterfilling=True), "chain_bd",
                dict(mod="psk", M=4, K=3, nr=2, NSymbs=51, bd_noise_var=1e-50, pathloss=None, waterfill=True, canonical=True),
                (5.0, 15.0), point=_bd_power(1e-3, 1.0)),
    # (a border loss other than 1, so that the division by it shows)
    "bd-pathloss": _case("BdSimulator", dict(modulator="psk", M=4, K=3, Nr=2, NSymbs=51, noise_var=1e-3, path_loss_border=0.5,
                                             pathloss=_PATHLOSS, bd_noise_var=0.5, waterfilling=True), "chain_bd",
                         dict(mod="psk", M=4, K=3, nr=2, NSymbs=51, bd_noise_var=0.5, pathloss=_PATHLOSS, waterfill=True,
                              canonical=True), (5.0, 15.0), point=_bd_power(1e-3, 0.5)),
    "ia-closed-form": _case("IaSimulator", dict(modulator="qam", M=16, NSymbs=51), "chain_ia",
                            dict(mod="qam", M=16, K=3, nr=2, nt=2, Ns=1, NSymbs=51), (10.0, 20.0), detailed=False),
    "ia-max-sinr": _case("IaSimulator", dict(modulator="qam", M=16, NSymbs=51, solver="max_sinr", max_iterations=20,
                                             initialize_with="random"), "chain_ia_iterative",
                         dict(algo="max_sinr", mod="qam", M=16, K=3, nr=2, nt=2, Ns=1, NSymbs=51, max_iterations=20,
                              relative_factor=1e-6, initialize_with="random"), (10.0, 20.0), detailed=False),
    "mimo-ofdm-tdl-auto": _case("MimoOfdmTdlSimulator", dict(_F1_CTOR, fused="auto"), "chain_mimo_ofdm_tdl", F1, (8.0, 14.0)),
    "mimo-ofdm-tdl-staged": _case("MimoOfdmTdlSimulator", dict(_F1_CTOR, fused=False), "chain_mimo_ofdm_tdl", F1, (8.0, 14.0)),
}
NAMES = list(CASES)
QAM = [n for n in NAMES if CASES[n]["kw"]["mod"] == "qam"]            # the cases demod="auto" sends through the slicer
# one case per simulator for the common-random-numbers run
CRN = ["awgn-qam16", "flat-jakes", "ofdm-tdl-256", "mimo-ofdm-2x3-zf", "mimo-svd-2x2", "large-mimo-5x6", "bd-pathloss",
       "ia-max-sinr", "mimo-ofdm-tdl-auto"]
EARLY_STOP = ["flat-jakes", "mimo-blast-2x2"]


def seeds(name, common_random_numbers=False):
    cfg = CASES[name]
    return [variation_seed(cfg["seed"], i, common_random_numbers) for i in range(len(cfg["snr"]))]


@functools.lru_cache(maxsize=None)
def realizations(name, seed, snr_db):
    """The chain of a case on `seed` at one SNR point over realizations 0 .. REP_MAX - 1, computed once and shared read-only:
    se, be [REP_MAX]; cap, its [REP_MAX] where the chain gives them (else None); nsym, nbits; table; decided [REP_MAX, nsym]."""
    from oracle import chains
    cfg = CASES[name]
    fn = getattr(chains, cfg["chain"])
    outs = [fn(chains.PhiloxRng(seed, r), **cfg["kw"], **cfg["point"](snr_db)) for r in range(REP_MAX)]
    ref = dict(se=np.array([o["symbol_errors"] for o in outs], dtype=np.int64),
               be=np.array([o["bit_errors"] for o in outs], dtype=np.int64),
               cap=np.array([o["sum_capacity"] for o in outs]) if "sum_capacity" in outs[0] else None,
               its=np.array([o["runned_iterations"] for o in outs], dtype=np.int64) if "runned_iterations" in outs[0] else None,
               nsym=outs[0]["num_symbols"], nbits=outs[0]["num_bits"], table=np.asarray(outs[0]["table"]),
               decided=np.stack([np.asarray(o[cfg["decided"]]).reshape(-1) for o in outs]))
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def reference(name, common_random_numbers=False):
    """One realizations() per SNR point of a case, on the seeds the simulator has to use."""
    cfg = CASES[name]
    return [realizations(name, s, snr) for s, snr in zip(seeds(name, common_random_numbers), cfg["snr"])]


def sequential_results(ref):
    """The Results of one SNR point as the serial loop builds them: one update per realization."""
    from pyphysim_amd.simulations.results import Result
    out = {"ser": Result("ser", Result.RATIOTYPE), "ber": Result("ber", Result.RATIOTYPE),
           "symbol_errors": Result("symbol_errors", Result.SUMTYPE)}
    for s, b in zip(ref["se"].tolist(), ref["be"].tolist()):
        out["ser"].update(s, ref["nsym"])
        out["ber"].update(b, ref["nbits"])
        out["symbol_errors"].update(s)
    return out


def assert_same_statistics(got, want, rel=1e-12):
    """`got` holds the statistics of `want` (a Result fed one update per realization) to `rel`, relative: value, total and the
    number of updates equal; the running sum and the sum of squares to rel of themselves; the 95 % interval's ends to rel of
    themselves; the variance, sum of squares / n - mean^2, to rel of the mean square it is the small difference of (relative
    to the variance itself two exact ways of summing already differ by more: test_simulator_cases_cpu.py).  A sum of squares
    that is wrong by one realization's square moves all of these by far more.  Returns the variances' difference relative to
    the variance."""
    assert got.get_result() == want.get_result() and got.num_updates == want.num_updates
    a, b = got.to_dict(), want.to_dict()
    assert a["value"] == b["value"] and a["total"] == b["total"] and a["update_type_code"] == b["update_type_code"]
    for key in ("result_sum", "result_squared_sum"):
        assert abs(a[key] - b[key]) <= rel * abs(b[key]), (got.name, key, a[key], b[key])
    mean_square = b["result_squared_sum"] / want.num_updates
    assert abs(got.get_result_var() - want.get_result_var()) <= rel * mean_square, (got.name, got.get_result_var(),
                                                                                    want.get_result_var())
    for x, y in zip(got.get_confidence_interval(95), want.get_confidence_interval(95)):
        assert abs(x - y) <= rel * abs(y), (got.name, x, y)
    var = want.get_result_var()
    return abs(got.get_result_var() - var) / var if var > 0 else 0.0


def stop_prefix(ref, threshold):
    """Realizations the reference's loop runs under 'go on while symbol_errors < threshold': up to and including the first one
    whose running total reaches the threshold (all of them when none does)."""
    total = np.cumsum(ref["se"])
    hit = np.nonzero(total >= threshold)[0]
    return int(hit[0]) + 1 if hit.size else len(total)
