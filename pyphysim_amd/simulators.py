"""Ready-made link simulators on the fused GPU pipelines, shaped like the reference's own template
simulators (apps/awgn_modulators/simulate_psk.py, apps/mimo/simulate_mimo.py,
notebooks/TDL_and_OFDM.ipynb) but advancing by batches: subclasses of BatchedSimulationRunner
whose ``_run_batch`` is one call into libmcle.

    sim = MimoOfdmSimulator(SNR=[15, 20, 25], rep_max=100000)
    sim.simulate()
    sim.results.get_result_values_list('ser')
"""
import numpy as np

from . import _lib
from .channels import discretize_profile
from .engine import get_engine
from .modulators import BPSK, PSK, QAM, QPSK, dB2Linear
from .simulations import BatchedSimulationRunner

_GOLDEN = 0x9E3779B97F4A7C15


def make_modulator(name, M=None, engine=None):
    name = name.lower()
    if name == "qam":
        return QAM(M, engine=engine)
    if name == "psk":
        return PSK(M, engine=engine)
    if name == "qpsk":
        return QPSK(engine=engine)
    if name == "bpsk":
        return BPSK(engine=engine)
    raise ValueError("unknown modulator %r" % (name,))


class _LinkSimulator(BatchedSimulationRunner):
    """Common part: SNR sweep ('SNR' unpacked), modulator, seed handling, engine binding."""

    def __init__(self, SNR, modulator="qam", M=16, rep_max=1000, seed=0, batch_size=4096, dtype="f32",
                 demod="auto", engine=None, common_random_numbers=False, process_group=None,
                 exact_early_stop=False):
        super().__init__(batch_size=batch_size, process_group=process_group, exact_early_stop=exact_early_stop)
        self.rep_max = rep_max
        self.seed = int(seed)
        self.dtype = dtype
        self.common_random_numbers = common_random_numbers
        self._engine = engine
        self.modulator = make_modulator(modulator, M, engine) if isinstance(modulator, str) else modulator
        if demod == "auto":
            demod = "slicer" if isinstance(self.modulator, QAM) else "mindist"
        self.demod_method = _lib.DEMOD_QAM_SLICER if demod == "slicer" else _lib.DEMOD_MINDIST
        self.params.add("SNR", np.atleast_1d(np.asarray(SNR, dtype=float)))
        self.params.set_unpack_parameter("SNR")
        self.params.add("modulator", self.modulator.name)

    @property
    def engine(self):
        if self._engine is None:
            self._engine = get_engine()
        return self._engine

    def _seed_for(self, current_parameters):
        """Independent randomness per parameter variation (the reference keeps drawing from one
        global stream) unless common_random_numbers asks for the same draws at every SNR."""
        if self.common_random_numbers:
            return self.seed
        return (self.seed + (max(current_parameters.unpack_index, 0) + 1) * _GOLDEN) & 0xFFFFFFFFFFFFFFFF

    def _bind(self):
        self.modulator._engine = self.engine
        return self.modulator._bind()

    @staticmethod
    def _noise_var(current_parameters):
        return 1.0 / float(dB2Linear(current_parameters["SNR"]))

    def _launch(self, current_parameters, first_rep, count, per_realization):
        raise NotImplementedError

    def _run_batch(self, current_parameters, first_rep, count):
        return self._launch(current_parameters, first_rep, count, False)

    def _run_batch_detailed(self, current_parameters, first_rep, count):
        return self._launch(current_parameters, first_rep, count, True)[:3]


class AwgnSimulator(_LinkSimulator):
    """Config 1: apps/awgn_modulators/simulate_psk.py:51-115."""

    def __init__(self, SNR, modulator="qam", M=16, NSymbs=10000, **kw):
        super().__init__(SNR, modulator, M, **kw)
        self.params.add("NSymbs", int(NSymbs))

    def _launch(self, current_parameters, first_rep, count, per_realization):
        eng = self._bind()
        return eng.run_awgn(current_parameters["NSymbs"], self._noise_var(current_parameters),
                            self._seed_for(current_parameters), first_rep, count, method=self.demod_method,
                            dtype=self.dtype, per_realization=per_realization)


class FlatFadingSimulator(_LinkSimulator):
    """Config 2: flat fading SuChannel(JakesSampleGenerator(Fd, Ts, L)) (or i.i.d. Rayleigh),
    receiver equalises with the known channel."""

    def __init__(self, SNR, modulator="qam", M=64, NSymbs=100000, Fd=100.0, Ts=1e-3, L=8, rayleigh_iid=False, **kw):
        super().__init__(SNR, modulator, M, **kw)
        for k, v in (("NSymbs", int(NSymbs)), ("Fd", float(Fd)), ("Ts", float(Ts)), ("L", int(L)),
                     ("rayleigh_iid", bool(rayleigh_iid))):
            self.params.add(k, v)

    def _launch(self, current_parameters, first_rep, count, per_realization):
        p = current_parameters
        eng = self._bind()
        return eng.run_flat_fading(p["NSymbs"], self._noise_var(p), self._seed_for(p), first_rep, count, Fd=p["Fd"],
                                   Ts=p["Ts"], L=p["L"], rayleigh_iid=p["rayleigh_iid"], method=self.demod_method,
                                   dtype=self.dtype, per_realization=per_realization)


class OfdmTdlSimulator(_LinkSimulator):
    """Config 3: notebooks/TDL_and_OFDM.ipynb OfdmTdlSimulator (OFDM over a Jakes TDL channel with
    the one-tap equaliser)."""

    def __init__(self, SNR, modulator="qpsk", M=4, fft_size=1024, cp_size=16, num_used_subcarriers=None,
                 num_ofdm_symbols=1, Fd=10.0, Ts=1.0 / (15e3 * 1024), L=8,
                 tap_powers_dB=(0.0, -3.0, -6.0, -9.0, -12.0), tap_delays=None, **kw):
        super().__init__(SNR, modulator, M, **kw)
        if tap_delays is None:
            tap_delays = np.arange(len(tap_powers_dB)) * Ts
        self._tap_power, self._tap_delay = discretize_profile(np.asarray(tap_powers_dB, dtype=float),
                                                               np.asarray(tap_delays, dtype=float), Ts)
        for k, v in (("fft_size", int(fft_size)), ("cp_size", int(cp_size)),
                     ("num_used_subcarriers", int(num_used_subcarriers or fft_size)),
                     ("num_ofdm_symbols", int(num_ofdm_symbols)), ("Fd", float(Fd)), ("Ts", float(Ts)),
                     ("L", int(L))):
            self.params.add(k, v)

    def _launch(self, current_parameters, first_rep, count, per_realization):
        p = current_parameters
        eng = self._bind()
        return eng.run_ofdm_tdl(p["fft_size"], p["cp_size"], p["num_used_subcarriers"], p["num_ofdm_symbols"],
                                self._noise_var(p), self._tap_power, self._tap_delay, self._seed_for(p), first_rep,
                                count, Fd=p["Fd"], Ts=p["Ts"], L=p["L"], method=self.demod_method, dtype=self.dtype,
                                per_realization=per_realization)


class MimoOfdmSimulator(_LinkSimulator):
    """Config 4: apps/mimo/simulate_mimo.py:68-142 (Blast, flat H = randn_c(Nr, Nt) per
    realization) with per-antenna OFDM; MMSE (set_noise_var) or zero forcing."""

    def __init__(self, SNR, modulator="qam", M=64, Nt=4, Nr=4, fft_size=1024, cp_size=16,
                 num_used_subcarriers=None, num_ofdm_symbols=1, mmse=True, **kw):
        super().__init__(SNR, modulator, M, **kw)
        for k, v in (("Nt", int(Nt)), ("Nr", int(Nr)), ("fft_size", int(fft_size)), ("cp_size", int(cp_size)),
                     ("num_used_subcarriers", int(num_used_subcarriers or fft_size)),
                     ("num_ofdm_symbols", int(num_ofdm_symbols)), ("mmse", bool(mmse))):
            self.params.add(k, v)

    def _launch(self, current_parameters, first_rep, count, per_realization):
        p = current_parameters
        eng = self._bind()
        return eng.run_mimo_ofdm(p["Nt"], p["Nr"], p["fft_size"], p["cp_size"], p["num_used_subcarriers"],
                                 p["num_ofdm_symbols"], self._noise_var(p), self._seed_for(p), first_rep, count,
                                 mmse=p["mmse"], method=self.demod_method, dtype=self.dtype,
                                 per_realization=per_realization)


class MimoSimulator(_LinkSimulator):
    """apps/mimo/simulate_mimo.py:22-142 (MIMOSimulationRunner and its Alamouti / Blast / MRC / MRT / SVDMimo /
    GMDMimo subclasses): flat channel per realization, NSymbs symbols per layer, single carrier.  `mmse=True`
    is Blast.set_noise_var(noise_var) (the app itself runs zero forcing)."""

    def __init__(self, SNR, scheme="blast", modulator="qam", M=16, Nt=2, Nr=2, NSymbs=200, mmse=False, **kw):
        super().__init__(SNR, modulator, M, **kw)
        if scheme not in _lib.MIMO_SCHEMES:
            raise ValueError("unknown MIMO scheme %r" % (scheme,))
        for k, v in (("scheme", scheme), ("Nt", int(Nt)), ("Nr", int(Nr)), ("NSymbs", int(NSymbs)),
                     ("mmse", bool(mmse))):
            self.params.add(k, v)

    def _launch(self, current_parameters, first_rep, count, per_realization):
        p = current_parameters
        eng = self._bind()
        return eng.run_mimo_flat(p["scheme"], p["Nt"], p["Nr"], p["NSymbs"], self._noise_var(p), self._seed_for(p),
                                 first_rep, count, mmse=p["mmse"], method=self.demod_method, dtype=self.dtype,
                                 per_realization=per_realization)


class LargeMimoSimulator(_LinkSimulator):
    """MimoSimulator's 'blast' (apps/mimo/simulate_mimo.py with mimo.Blast; Nt = 1: mimo.MRC) for arrays beyond 4 x 4:
    1 <= Nt <= 8, Nt <= Nr <= 16, on the matrix-core link (Engine.run_mimo_large).  Same draws as MimoSimulator, so up to
    4 x 4 the two give the same counts in complex128.  `mmse=True` is Blast.set_noise_var(noise_var)."""

    def __init__(self, SNR, Nt=8, Nr=8, NSymbs=200, modulator="qam", M=16, mmse=False, **kw):
        super().__init__(SNR, modulator, M, **kw)
        if not (1 <= int(Nt) <= 8 and int(Nt) <= int(Nr) <= 16):
            raise ValueError("LargeMimoSimulator needs 1 <= Nt <= 8 and Nt <= Nr <= 16 (got Nt %d, Nr %d)" % (Nt, Nr))
        for k, v in (("Nt", int(Nt)), ("Nr", int(Nr)), ("NSymbs", int(NSymbs)), ("mmse", bool(mmse))):
            self.params.add(k, v)

    def _launch(self, current_parameters, first_rep, count, per_realization):
        p = current_parameters
        eng = self._bind()
        return eng.run_mimo_large(p["Nt"], p["Nr"], p["NSymbs"], self._noise_var(p), self._seed_for(p), first_rep, count,
                                  mmse=p["mmse"], method=self.demod_method, dtype=self.dtype,
                                  per_realization=per_realization)


class BdSimulator(_LinkSimulator):
    """apps/comp_BD/simulate_comp_simple.py:22-140 (no external interference source): K cells with Nr x Nr antennas
    each transmit jointly through a block-diagonalising precoder (water-filling normalised to the strongest cell,
    BlockDiagonalizer.block_diagonalize) and every user zero-forces with pinv(newH).  As in the app the noise
    power is fixed and SNR sets the transmit power: iPu = dB2Linear(SNR) * noise_var / path_loss_border."""

    def __init__(self, SNR, modulator="psk", M=4, K=3, Nr=2, NSymbs=500, noise_var=None, path_loss_border=1.0,
                 pathloss=None, bd_noise_var=1e-50, waterfilling=True, **kw):
        super().__init__(SNR, modulator, M, **kw)
        for k, v in (("K", int(K)), ("Nr", int(Nr)), ("NSymbs", int(NSymbs)), ("waterfilling", bool(waterfilling))):
            self.params.add(k, v)
        # conversion.dBm2Linear(-116.4): the app's N0 (simulate_comp_simple.py:42,62)
        self.noise_var = float(noise_var) if noise_var is not None else 10.0 ** ((-116.4 - 30.0) / 10.0)
        self.path_loss_border = float(path_loss_border)
        self.pathloss = None if pathloss is None else np.asarray(pathloss, dtype=float)
        self.bd_noise_var = float(bd_noise_var)

    def _launch(self, current_parameters, first_rep, count, per_realization):
        p = current_parameters
        eng = self._bind()
        iPu = float(dB2Linear(p["SNR"])) * self.noise_var / self.path_loss_border
        return eng.run_bd(p["K"], p["Nr"], p["NSymbs"], iPu, self.noise_var, self._seed_for(p), first_rep, count,
                          bd_noise_var=self.bd_noise_var, pathloss=self.pathloss, waterfilling=p["waterfilling"],
                          method=self.demod_method, dtype=self.dtype, per_realization=per_realization)


class MimoOfdmTdlSimulator(_LinkSimulator):
    """spatial multiplexing over a frequency-selective MIMO TDL channel
    (TdlMimoChannel fading.py:1290-1333, MIMO branch of corrupt_data :1107-1117), per-antenna OFDM and one
    MMSE/ZF receive filter per used subcarrier from the per-symbol mean frequency response (:513-536).

    Unlike configs 1-5 this chain is STAGED: a batch of realizations flows through the batched operator
    kernels with every intermediate resident in HBM (symbols -> modulate -> Blast -> OFDM -> Jakes taps ->
    TDL -> AWGN -> OFDM^-1 -> mean response -> filters -> decode -> demod+count); nothing but the counters
    returns to the host.  Draw layout: the mcle-philox-v1 streams of realization r (DATA symbols, PHASE
    (L, S, Nr, Nt) phi then psi, NOISE [Nr, n + max delay])."""

    def __init__(self, SNR, modulator="qam", M=16, Nt=2, Nr=2, fft_size=64, cp_size=16, num_used_subcarriers=None,
                 num_ofdm_symbols=2, Fd=50.0, Ts=1e-6, L=8, tap_powers_dB=(0.0, -4.0, -9.0), tap_delays=None,
                 mmse=True, fused="auto", **kw):
        self.fused = fused                    # "auto": fused kernel when it supports the configuration
        kw.setdefault("batch_size", 4096 if fused else 256)
        super().__init__(SNR, modulator, M, **kw)
        if tap_delays is None:
            tap_delays = np.asarray((0, 2, 5)[:len(tap_powers_dB)], dtype=float) * Ts
        self._tap_power, self._tap_delay = discretize_profile(np.asarray(tap_powers_dB, dtype=float),
                                                               np.asarray(tap_delays, dtype=float), Ts)
        for k, v in (("Nt", int(Nt)), ("Nr", int(Nr)), ("fft_size", int(fft_size)), ("cp_size", int(cp_size)),
                     ("num_used_subcarriers", int(num_used_subcarriers or fft_size)),
                     ("num_ofdm_symbols", int(num_ofdm_symbols)), ("Fd", float(Fd)), ("Ts", float(Ts)),
                     ("L", int(L)), ("mmse", bool(mmse))):
            self.params.add(k, v)

    _FUSED_FFT = (64, 128, 256, 512, 1024, 2048)

    def _launch(self, current_parameters, first_rep, count, per_realization):
        p = current_parameters
        # fused kernels: every 1 <= Nt <= Nr <= 4 at fft_size 256 .. 2048 with delays <= min(256, fft_size / 2) (one receive antenna per
        # wavefront, round 5; delays beyond the prefix since round 6), Nt = Nr in {2, 4} at 64 .. 2048 otherwise; the C ABI reports anything else as unsupported
        if self.fused and 1 <= p["Nt"] <= p["Nr"] <= 4 and p["fft_size"] in self._FUSED_FFT:
            try:
                eng = self._bind()
                return eng.run_mimo_ofdm_tdl(
                    p["Nt"], p["Nr"], p["fft_size"], p["cp_size"], p["num_used_subcarriers"], p["num_ofdm_symbols"],
                    self._noise_var(p), self._tap_power, self._tap_delay, self._seed_for(p), first_rep, count,
                    Fd=p["Fd"], Ts=p["Ts"], L=p["L"], mmse=p["mmse"], method=self.demod_method, dtype=self.dtype,
                    per_realization=per_realization)
            except _lib.McleUnsupported:
                if self.fused is True:
                    raise
        elif self.fused is True:
            raise ValueError("the fused pipeline supports 1 <= Nt <= Nr <= 4 and fft_size in {64, 128, ..., 2048}")
        return self._launch_staged(p, first_rep, count, per_realization)

    def _launch_staged(self, p, first_rep, count, per_realization):
        eng = self._bind()
        dt = self.dtype
        nt, nr, fft, cp, used = p["Nt"], p["Nr"], p["fft_size"], p["cp_size"], p["num_used_subcarriers"]
        n_sym, L, Ts = p["num_ofdm_symbols"], p["L"], p["Ts"]
        noise_var, seed = self._noise_var(p), self._seed_for(p)
        ns = used * n_sym                      # data symbols per antenna
        n = n_sym * (fft + cp)                 # time samples per antenna
        delays = np.asarray(self._tap_delay, dtype=np.int32)
        S = delays.size
        if count == 0:
            c = eng.read_counters(eng.new_counters())
            return (c, None, None) if per_realization else c
        idx = eng.rand_symbols_batch(nt * ns, self.modulator.M, seed, first_rep, count)
        X = eng.blast_encode(eng.modulate(idx, dtype=dt), nt, batch=count, dtype=dt)           # [count, nt, ns]
        T = eng.ofdm_modulate(X, fft, cp, used, batch=count * nt, dtype=dt).reshape(count, nt, n)
        # Jakes time axis of a fresh generator (fading_generators.py:459-467): t_k = Ts + k*delta
        step = Ts * 1.0000000001
        delta = float(np.float64(Ts + step) - np.float64(Ts))
        amp = np.repeat(np.sqrt(np.asarray(self._tap_power, dtype=float)), nr * nt) * np.sqrt(1.0 / L)
        taps = eng.jakes_taps_philox(seed, first_rep, count, L, p["Fd"], Ts, delta, amp, n, dtype=dt)
        taps5 = taps.reshape(count, S, nr, nt, n)
        faded = eng.tdl_apply_mimo(T, taps5, delays, dtype=dt)                                  # [count, nr, n+dmax]
        R = eng.awgn_philox(faded, seed, first_rep, count, noise_var, dtype=dt)
        Rn = eng.slice_rows(R, n) if R.shape[-1] != n else R
        Y = eng.ofdm_demodulate(Rn, fft, cp, used, batch=count * nr, dtype=dt).reshape(count, nr, ns)
        Hm = eng.tdl_mean_freq_response(taps5, delays, n_sym, fft, cp, used, dtype=dt, batch=count)
        # MMSE Gram matrices are positive definite: the singular-matrix flags are only read back for ZF
        G, skipped = eng.blast_filter(Hm.reshape(count * ns, nr, nt), noise_var if p["mmse"] else 0.0, dtype=dt,
                                      read_skipped=not p["mmse"])
        est = eng.blast_decode_per_subcarrier(G.reshape(count, ns, nt, nr), Y, dtype=dt)        # [count, ns*nt]
        c, se, be = eng.demod_count(est, idx, n_real=count, method=self.demod_method, dtype=dt)
        if not p["mmse"]:
            c["n_singular_subcarriers"] = int(np.count_nonzero(skipped))
        return (c, se, be) if per_realization else c


class IaSimulator(_LinkSimulator):
    """Config 5: apps/ia/simulate_ia.py:94-245 with ClosedFormIASolver(use_best_init=True) on a
    3-user 2x2 interference channel, one stream per user.  Adds the 'sum_capacity' RATIO(x, 1)
    Result of the reference app next to the error-rate Results."""

    def __init__(self, SNR, modulator="qam", M=16, NSymbs=200, solver="closed_form", max_iterations=60,
                 relative_factor=1e-6, initialize_with="random", **kw):
        """solver: 'closed_form' (ClosedFormIASolver, use_best_init) or 'alt_min' / 'min_leakage' / 'max_sinr'
        (AlternatingMinIASolver / MinLeakageIASolver / MaxSinrIASolver with initialize_with='random';
        max_iterations defaults to the app's 60, apps/ia/simulate_ia.py:330)."""
        super().__init__(SNR, modulator, M, **kw)
        if solver not in _lib.IA_SOLVERS:
            raise ValueError("unknown IA solver %r" % (solver,))
        for k, v in (("NSymbs", int(NSymbs)), ("K", 3), ("Nr", 2), ("Nt", 2), ("Ns", 1), ("solver", solver)):
            self.params.add(k, v)
        if solver != "closed_form":
            if initialize_with not in ("random", "closed_form", "alt_min", "svd"):
                raise ValueError("initialize_with must be 'random', 'closed_form', 'alt_min' or 'svd'")
            self.params.add("max_iterations", int(max_iterations))
            self.params.add("initialize_with", initialize_with)
        self.relative_factor = float(relative_factor)
        if self.exact_early_stop:
            raise ValueError("IaSimulator carries per-batch capacity / iteration sums and does not replay single "
                             "realizations: exact_early_stop is not supported")

    # per-batch sums carried next to the integer counters: added over batches, all-reduced over ranks and kept in
    # the partial-results state, so 'sum_capacity' / 'ia_runned_iterations' are right under sharding and resume
    EXTRA_KEYS = ("sum_capacity", "sum_capacity_sq", "ia_runned_iterations", "ia_runned_iterations_sq")
    EXTRA_INT_KEYS = ("ia_runned_iterations", "ia_runned_iterations_sq")

    def _run_batch(self, current_parameters, first_rep, count):
        eng = self._bind()
        p = current_parameters
        return eng.run_ia(p["NSymbs"], self._noise_var(p), self._seed_for(p), first_rep, count,
                          method=self.demod_method, dtype=self.dtype, solver=p["solver"],
                          max_iterations=p["max_iterations"] if p["solver"] != "closed_form" else 1,
                          relative_factor=self.relative_factor,
                          initialize_with=p["initialize_with"] if p["solver"] != "closed_form" else "random")

    def _results_from_counters(self, current_parameters, c):
        from .simulations import Result
        res = super()._results_from_counters(current_parameters, c)
        n = max(int(c["n_realizations"]), 1)
        cap, cap_sq = float(c.get("sum_capacity", 0.0)), float(c.get("sum_capacity_sq", 0.0))
        res.add_result(Result.from_batch("sum_capacity", Result.RATIOTYPE, cap, n, cap, cap_sq, n))
        if current_parameters["solver"] != "closed_form":
            its, its_sq = int(c.get("ia_runned_iterations", 0)), int(c.get("ia_runned_iterations_sq", 0))
            res.add_result(Result.from_batch("ia_runned_iterations", Result.RATIOTYPE, its, n, its, its_sq, n))
        return res


class QuantizedIaSimulator(IaSimulator):
    """Limited-feedback IA: apps/ia/simple_maxsinr_quantized.py:170-273 as a simulator.  Every link of the 3-user 2x2
    interference channel is fed back as the index of the nearest word of ``codebook`` [C, 4]; the solver (the app's
    MaxSinrIASolver with 120 iterations by default) sees only the quantized channel, the precoded data cross the true one, and
    'ber', 'ser' and 'sum_capacity' are those of the true channel.  Adds 'quant_dist' (RATIO: the sum of the chosen distances over
    the links).  On the draws of IaSimulator for the same seed (common random numbers with the perfect-CSI run).

    codebook: None draws ``codebook_size`` random unit-norm words (quantization.gen_codebook, seeded by ``seed``); a codebook
    from CodebookFinder in G(4, 1), reshaped to [C, 4], is taken as is -- metric='chordal' is the one that matches it."""

    def __init__(self, SNR, codebook=None, codebook_size=512, metric="euclidean", solver="max_sinr", max_iterations=120,
                 modulator="bpsk", M=2, NSymbs=50, **kw):
        super().__init__(SNR, modulator, M, NSymbs=NSymbs, solver=solver, max_iterations=max_iterations, **kw)
        if metric not in _lib.QUANT_METRICS:
            raise ValueError("metric must be 'euclidean' or 'chordal' (got %r)" % (metric,))
        if codebook is None:
            from .quantization import gen_codebook
            codebook = gen_codebook(int(codebook_size), 4, seed=self.seed, engine=self.engine)
        self.codebook = np.ascontiguousarray(np.asarray(codebook).reshape(-1, 4), dtype=np.complex128)
        self.params.add("metric", metric)
        self.params.add("codebook_size", int(self.codebook.shape[0]))

    EXTRA_KEYS = IaSimulator.EXTRA_KEYS + ("quant_dist", "quant_dist_sq")

    def _run_batch(self, current_parameters, first_rep, count):
        eng = self._bind()
        p = current_parameters
        return eng.run_ia_quantized(p["NSymbs"], self._noise_var(p), self._seed_for(p), first_rep, count, self.codebook,
                                    metric=p["metric"], method=self.demod_method, dtype=self.dtype, solver=p["solver"],
                                    max_iterations=p["max_iterations"] if p["solver"] != "closed_form" else 1,
                                    relative_factor=self.relative_factor,
                                    initialize_with=p["initialize_with"] if p["solver"] != "closed_form" else "random")

    def _results_from_counters(self, current_parameters, c):
        from .simulations import Result
        res = super()._results_from_counters(current_parameters, c)
        n = max(int(c["n_realizations"]), 1)
        d, d_sq = float(c.get("quant_dist", 0.0)), float(c.get("quant_dist_sq", 0.0))
        # one update per realization: RATIO(sum of its nine distances, 9 links)
        res.add_result(Result.from_batch("quant_dist", Result.RATIOTYPE, d, 9 * n, d / 9.0, d_sq / 81.0, n))
        return res


class ChannelEstimationSimulator(BatchedSimulationRunner):
    """Estimation-error Monte Carlo of the CAZAC-based channel estimator (the experiment of the reference's
    apps/simple_precoded_srs.py): `n_users` users send the SRS sequences of one root (cyclic shifts `shifts`) on the
    same comb of `Ne` positions, every (user, receive antenna) link is a block-static tapped delay line with the given
    profile (integer delays on the size_multiplier * Ne subcarrier grid), and every user is estimated with
    `num_taps_to_keep`.  One call into libmcle per batch (Engine.run_chanest).
    Results: 'nmse_user{u}' = RATIO(sum |H^ - H|^2, sum |H|^2), 'elapsed_time'.

    The app's interference-cancellation rules at the receiver of `direct_user`: interference_cancellation='direct' estimates
    that user first and subtracts its contribution before the others are estimated, 'sic' then goes on through the others
    in descending order of their first estimates' norm; `pathloss` is a linear power gain per user (the app's unequal path
    losses are what makes the rules matter), `root_indexes` one root per user as the app has it (the shifts may then
    coincide).  A rule other than 'none' or a pathloss routes the batches through Engine.run_chanest_ic; otherwise run_chanest."""

    def __init__(self, SNR, n_users=3, shifts=None, Ne=150, size_multiplier=2, num_taps_to_keep=15, Nr=4, root_index=25,
                 tap_powers_dB=(0.0, -3.0, -6.0, -9.0), tap_delays=(0, 1, 2, 4), rep_max=1000, seed=0, batch_size=4096,
                 dtype="f32", engine=None, common_random_numbers=False, process_group=None,
                 interference_cancellation="none", direct_user=0, pathloss=None, root_indexes=None):
        super().__init__(batch_size=batch_size, process_group=process_group)
        from .reference_signals import RootSequence, SrsUeSequence
        self.rep_max = rep_max
        self.seed = int(seed)
        self.dtype = dtype
        self.common_random_numbers = common_random_numbers
        self._engine = engine
        shifts = tuple(range(n_users)) if shifts is None else tuple(int(s) for s in shifts)
        if root_indexes is None:
            if len(shifts) != n_users or len(set(shifts)) != n_users:
                raise ValueError("shifts must name one distinct cyclic shift per user")
            root = RootSequence(root_index=int(root_index), size=int(Ne))
            self.ref_seqs = np.stack([SrsUeSequence(root, s).seq_array() for s in shifts])
        else:
            roots = tuple(int(u) for u in root_indexes)
            if len(roots) != n_users or len(shifts) != n_users or len(set(zip(roots, shifts))) != n_users:
                raise ValueError("root_indexes and shifts must name one distinct (root, cyclic shift) pair per user")
            self.ref_seqs = np.stack([SrsUeSequence(RootSequence(root_index=u, size=int(Ne)), s).seq_array()
                                      for u, s in zip(roots, shifts)])
        if interference_cancellation not in _lib.CHANEST_IC_MODES:
            raise ValueError("interference_cancellation must be 'none', 'direct' or 'sic'")
        if not 0 <= int(direct_user) < n_users:
            raise ValueError("direct_user must be one of the %d users" % n_users)
        self._link_gain = None if pathloss is None else np.asarray(pathloss, dtype=float).reshape(-1)
        if self._link_gain is not None and self._link_gain.size != n_users:
            raise ValueError("pathloss must hold one linear gain per user")
        self._ic_mode, self._direct_user = interference_cancellation, int(direct_user)
        self._plain = interference_cancellation == "none" and pathloss is None
        self._tap_power = 10.0 ** (np.asarray(tap_powers_dB, dtype=float) / 10.0)
        self._tap_power = self._tap_power / self._tap_power.sum()
        self._tap_delay = [int(d) for d in tap_delays]
        self.EXTRA_KEYS = tuple("%s_user%d" % (k, u) for u in range(n_users) for k in ("err", "pow", "nmse", "nmse_sq"))
        self.params.add("SNR", np.atleast_1d(np.asarray(SNR, dtype=float)))
        self.params.set_unpack_parameter("SNR")
        for k, v in (("n_users", int(n_users)), ("shifts", shifts), ("Ne", int(Ne)), ("size_multiplier", int(size_multiplier)),
                     ("num_taps_to_keep", int(num_taps_to_keep)), ("Nr", int(Nr)), ("root_index", int(root_index))):
            self.params.add(k, v)

    engine = _LinkSimulator.engine
    _seed_for = _LinkSimulator._seed_for

    def _run_batch(self, current_parameters, first_rep, count):
        p = current_parameters
        args = (self.ref_seqs, p["Nr"], p["num_taps_to_keep"], p["size_multiplier"], 1.0 / float(dB2Linear(p["SNR"])),
                self._tap_power, self._tap_delay, self._seed_for(p), first_rep, count)
        if self._plain:
            res, err, pw = self.engine.run_chanest(*args, dtype=self.dtype, per_realization=True)
        else:
            res, err, pw = self.engine.run_chanest_ic(*args, self._ic_mode, direct_user=self._direct_user,
                                                      link_gain=self._link_gain, dtype=self.dtype, per_realization=True)
        c = {k: 0 for k in self.COUNTER_KEYS + ("n_symbols", "n_bits")}
        c["n_realizations"] = int(count)
        ratio = np.cumsum(err / pw, axis=0)[-1] if count else np.zeros(p["n_users"])
        ratio_sq = np.cumsum(np.square(err / pw), axis=0)[-1] if count else np.zeros(p["n_users"])
        for u in range(p["n_users"]):
            c["err_user%d" % u], c["pow_user%d" % u] = float(res["err"][u]), float(res["pow"][u])
            c["nmse_user%d" % u], c["nmse_sq_user%d" % u] = float(ratio[u]), float(ratio_sq[u])
        return c

    def _results_from_counters(self, current_parameters, c):
        from .simulations import Result, SimulationResults
        n = max(int(c["n_realizations"]), 1)
        res = SimulationResults()
        for u in range(current_parameters["n_users"]):
            res.add_result(Result.from_batch("nmse_user%d" % u, Result.RATIOTYPE, float(c.get("err_user%d" % u, 0.0)),
                                             float(c.get("pow_user%d" % u, 0.0)), float(c.get("nmse_user%d" % u, 0.0)),
                                             float(c.get("nmse_sq_user%d" % u, 0.0)), n))
        return res


def _exact_limbs(values):
    """Three integer-valued float64 sums whose weighted total (2^-8, 2^-34, 2^-60) is sum(values) to 2^-60 per value.  Each is
    a sum of integers below 2^26 (for values below 2^18), exact in float64 up to 2^27 values -- so the totals a simulator
    adds up over batches and ranks do not depend on how the realizations were grouped, which a float sum would."""
    x = np.asarray(values, dtype=np.float64)
    t1 = np.floor(x * 2.0 ** 8)
    r1 = x - t1 * 2.0 ** -8
    t2 = np.floor(r1 * 2.0 ** 34)
    r2 = r1 - t2 * 2.0 ** -34
    t3 = np.floor(r2 * 2.0 ** 60)
    return tuple(float(t.sum()) for t in (t1, t2, t3))       # (integers: any order gives the same sum)


def _from_limbs(c, key):
    return (float(c.get(key + "_l0", 0.0)) * 2.0 ** -8 + float(c.get(key + "_l1", 0.0)) * 2.0 ** -34) \
        + float(c.get(key + "_l2", 0.0)) * 2.0 ** -60


class PilotEstimationSimulator(BatchedSimulationRunner):
    """Estimation-error Monte Carlo of the LS and MMSE block-pilot estimators (the experiment of the reference's
    tests/channel_estimation_package_test.py:246-325; Fodor et al. 2014): per realization `Nt` x `num_pilots` pilots of power
    `pilot_power` (random phases when random_pilots, else the first rows of a DFT matrix), a channel h = alpha L w with w
    `Nr` x `Nt` of CN(0, 1), Y = h s + noise of power 1 / SNR, and both estimates from the same Y.  With a covariance `C`
    (`Nr` x `Nr`, Nt = 1) L = cholesky(C) and the MMSE estimator is handed alpha^2 C; without one L = I and only the LS
    estimator runs.  One call into libmcle per batch (Engine.run_pilot_mse).

    Results: 'mse_ls' = RATIO(sum |h^_LS - h|^2, alpha^2 n), the reference test's normalisation; 'mse_mmse' =
    RATIO(sum |h^_MMSE - h|^2, n), only with C; 'channel_power' = RATIO(sum |h|^2, n); 'elapsed_time'.  The sums are kept as
    exact integer limbs, so the results do not depend on batch_size or on the number of ranks."""

    _SUMS = ("err_ls", "err_mmse", "pow")
    # (the sums of squares only feed the confidence intervals and stay plain float sums)
    EXTRA_KEYS = tuple("%s_l%d" % (k, i) for k in _SUMS for i in range(3)) + tuple(k + "_sq" for k in _SUMS)

    def __init__(self, SNR, Nr=64, Nt=1, num_pilots=10, pilot_power=1.0, alpha=1.0, C=None, random_pilots=True,
                 rep_max=5000, seed=0, batch_size=4096, dtype="f64", engine=None, common_random_numbers=False,
                 process_group=None):
        super().__init__(batch_size=batch_size, process_group=process_group)
        self.rep_max = rep_max
        self.seed = int(seed)
        self.dtype = dtype
        self.common_random_numbers = common_random_numbers
        self._engine = engine
        self._L = self._cov = None
        if C is not None:
            C = np.asarray(C, dtype=np.complex128)
            if C.shape != (int(Nr), int(Nr)) or int(Nt) != 1:
                raise ValueError("C must be [Nr, Nr] = [%d, %d] and needs Nt = 1 (the MMSE estimator is SIMO)" % (Nr, Nr))
            self._L, self._cov = np.linalg.cholesky(C), float(alpha) ** 2 * C
        self._pilots = None
        if not random_pilots:
            t, p = np.arange(int(Nt))[:, None], np.arange(int(num_pilots))[None, :]
            self._pilots = np.sqrt(float(pilot_power)) * np.exp(-2j * np.pi * t * p / int(num_pilots))
        self.params.add("SNR", np.atleast_1d(np.asarray(SNR, dtype=float)))
        self.params.set_unpack_parameter("SNR")
        for k, v in (("Nr", int(Nr)), ("Nt", int(Nt)), ("num_pilots", int(num_pilots)), ("pilot_power", float(pilot_power)),
                     ("alpha", float(alpha)), ("random_pilots", bool(random_pilots))):
            self.params.add(k, v)

    engine = _LinkSimulator.engine
    _seed_for = _LinkSimulator._seed_for

    def _run_batch(self, current_parameters, first_rep, count):
        p = current_parameters
        res, e_ls, e_mm, pw = self.engine.run_pilot_mse(
            p["Nr"], p["Nt"], p["num_pilots"], 1.0 / float(dB2Linear(p["SNR"])), self._seed_for(p), first_rep, count,
            pilot_power=p["pilot_power"], alpha=p["alpha"], pilots=self._pilots, chan_factor=self._L, cov=self._cov,
            dtype=self.dtype, per_realization=True)
        c = {k: 0 for k in self.COUNTER_KEYS + ("n_symbols", "n_bits")}
        c["n_realizations"] = int(count)
        for key, arr in zip(self._SUMS, (e_ls, e_mm, pw)):
            limbs = _exact_limbs(arr) if arr is not None else (0.0, 0.0, 0.0)
            for i, v in enumerate(limbs):
                c["%s_l%d" % (key, i)] = v
            c[key + "_sq"] = float(np.square(arr).sum()) if arr is not None else 0.0
        return c

    def _results_from_counters(self, current_parameters, c):
        from .simulations import Result, SimulationResults
        n = max(int(c["n_realizations"]), 1)
        a2 = current_parameters["alpha"] ** 2
        res = SimulationResults()
        e_ls, pw = _from_limbs(c, "err_ls"), _from_limbs(c, "pow")
        res.add_result(Result.from_batch("mse_ls", Result.RATIOTYPE, e_ls, a2 * n, e_ls / a2, float(c.get("err_ls_sq", 0.0)) / a2 ** 2, n))
        if self._cov is not None:
            e_mm = _from_limbs(c, "err_mmse")
            res.add_result(Result.from_batch("mse_mmse", Result.RATIOTYPE, e_mm, float(n), e_mm, float(c.get("err_mmse_sq", 0.0)), n))
        res.add_result(Result.from_batch("channel_power", Result.RATIOTYPE, pw, float(n), pw, float(c.get("pow_sq", 0.0)), n))
        return res


class PilotMimoSimulator(_LinkSimulator):
    """What imperfect channel state costs the flat Blast link (MimoSimulator's 'blast'; the estimators of
    channel_estimation/estimators.py, Fodor et al. 2014, in front of mimo.Blast): per realization a channel h = alpha L w, a block
    of `num_pilots` pilots of power `pilot_power` (random phases when random_pilots, else the first rows of a DFT matrix), the LS
    estimate -- or with estimator='mmse' and a covariance `C` (`Nr` x `Nr`, Nt = 1: L = cholesky(C), the estimator is handed
    alpha^2 C) the MMSE one --, and `NSymbs` symbols per layer decoded with the Blast filter of the estimate and with that of the
    true channel, on the same data and the same noise.  Pilots and data see the same noise power 1 / SNR; `mmse=True` is
    Blast.set_noise_var.  One call into libmcle per batch (Engine.run_mimo_pilot_link).

    Results: 'ber', 'ser' (and the counts behind them) with estimated CSI; 'ber_perfect_csi', 'ser_perfect_csi' with the true
    channel; 'mse' = RATIO(sum |h^ - h|^2, alpha^2 n) for LS and RATIO(sum |h^ - h|^2, n) for MMSE, PilotEstimationSimulator's
    'mse_ls' / 'mse_mmse'; 'channel_power' = RATIO(sum |h|^2, n); 'elapsed_time'.  The sums of the errors are kept as exact integer
    limbs, so the results do not depend on batch_size or on the number of ranks."""

    _SUMS = ("err", "pow")
    _PERFECT = ("sym_errors_perfect", "sym_errors_sq_perfect", "bit_errors_perfect", "bit_errors_sq_perfect")
    EXTRA_INT_KEYS = _PERFECT
    EXTRA_KEYS = _PERFECT + tuple("%s_l%d" % (k, i) for k in _SUMS for i in range(3)) + tuple(k + "_sq" for k in _SUMS)

    def __init__(self, SNR, Nr=2, Nt=2, num_pilots=4, NSymbs=200, modulator="qam", M=16, pilot_power=1.0, alpha=1.0, C=None,
                 estimator="ls", random_pilots=True, mmse=False, **kw):
        kw.setdefault("dtype", "f64")
        super().__init__(SNR, modulator, M, **kw)
        if estimator not in _lib.PILOT_ESTIMATORS:
            raise ValueError("estimator must be 'ls' or 'mmse' (got %r)" % (estimator,))
        self._L = self._cov = None
        if C is not None:
            C = np.asarray(C, dtype=np.complex128)
            if C.shape != (int(Nr), int(Nr)):
                raise ValueError("C must be [Nr, Nr] = [%d, %d]" % (Nr, Nr))
            self._L, self._cov = np.linalg.cholesky(C), float(alpha) ** 2 * C
        if estimator == "mmse":
            if int(Nt) != 1:
                raise ValueError("the MMSE estimator needs Nt = 1 (it is SIMO)")
            if C is None:
                raise ValueError("the MMSE estimator needs a covariance C")
        self._pilots = None
        if not random_pilots:
            t, p = np.arange(int(Nt))[:, None], np.arange(int(num_pilots))[None, :]
            self._pilots = np.sqrt(float(pilot_power)) * np.exp(-2j * np.pi * t * p / int(num_pilots))
        for k, v in (("Nr", int(Nr)), ("Nt", int(Nt)), ("num_pilots", int(num_pilots)), ("NSymbs", int(NSymbs)),
                     ("pilot_power", float(pilot_power)), ("alpha", float(alpha)), ("estimator", estimator),
                     ("random_pilots", bool(random_pilots)), ("mmse", bool(mmse))):
            self.params.add(k, v)

    @staticmethod
    def _entry(eng):
        return eng.run_mimo_pilot_link

    def _launch(self, current_parameters, first_rep, count, per_realization):
        p = current_parameters
        eng = self._bind()
        c_est, c_perf, se, be, err, pw = self._entry(eng)(
            p["Nt"], p["Nr"], p["num_pilots"], p["NSymbs"], self._noise_var(p), self._seed_for(p), first_rep, count,
            pilot_power=p["pilot_power"], alpha=p["alpha"], pilots=self._pilots, chan_factor=self._L,
            cov=self._cov if p["estimator"] == "mmse" else None, estimator=p["estimator"], mmse=p["mmse"],
            method=self.demod_method, dtype=self.dtype, per_realization=True)
        c = dict(c_est)
        for k in ("sym_errors", "sym_errors_sq", "bit_errors", "bit_errors_sq"):
            c[k + "_perfect"] = c_perf[k]
        good = se[0] != 0xFFFFFFFF                   # (a skipped realization's err / pow are unspecified)
        for key, arr in zip(self._SUMS, (err[good], pw[good])):
            for i, v in enumerate(_exact_limbs(arr)):
                c["%s_l%d" % (key, i)] = v
            c[key + "_sq"] = float(np.square(arr).sum())
        return c, se[0], be[0]

    def _run_batch(self, current_parameters, first_rep, count):
        return self._launch(current_parameters, first_rep, count, False)[0]

    def _results_from_counters(self, current_parameters, c):
        from .simulations import Result
        res = super()._results_from_counters(current_parameters, c)
        n = c["n_realizations"]
        res.add_result(Result.from_counters("ber_perfect_csi", Result.RATIOTYPE, int(c.get("bit_errors_perfect", 0)),
                                            int(c.get("bit_errors_sq_perfect", 0)), c["n_bits"], n))
        res.add_result(Result.from_counters("ser_perfect_csi", Result.RATIOTYPE, int(c.get("sym_errors_perfect", 0)),
                                            int(c.get("sym_errors_sq_perfect", 0)), c["n_symbols"], n))
        m = max(int(n), 1)
        norm = 1.0 if current_parameters["estimator"] == "mmse" else current_parameters["alpha"] ** 2
        err, pw = _from_limbs(c, "err"), _from_limbs(c, "pow")
        res.add_result(Result.from_batch("mse", Result.RATIOTYPE, err, norm * m, err / norm, float(c.get("err_sq", 0.0)) / norm ** 2, m))
        res.add_result(Result.from_batch("channel_power", Result.RATIOTYPE, pw, float(m), pw, float(c.get("pow_sq", 0.0)), m))
        return res


class LargePilotMimoSimulator(PilotMimoSimulator):
    """PilotMimoSimulator for large arrays: 1 <= Nt <= 8, Nt <= Nr <= 16 (the envelope of LargeMimoSimulator), one call of
    Engine.run_mimo_large_pilot_link per batch -- how many pilots a large receive array needs before the estimate stops costing
    symbol errors.  Same constructor, same results ('ber', 'ser', 'ber_perfect_csi', 'ser_perfect_csi', 'mse', 'channel_power'
    and the limb sums), same draws: up to 4 x 4 the counts of PilotMimoSimulator, and without a covariance and with alpha = 1
    'ser_perfect_csi' is LargeMimoSimulator's 'ser' on the same seed."""

    def __init__(self, SNR, Nr=16, Nt=4, num_pilots=8, **kw):
        if not (1 <= int(Nt) <= 8 and int(Nt) <= int(Nr) <= 16):
            raise ValueError("LargePilotMimoSimulator needs 1 <= Nt <= 8 and Nt <= Nr <= 16 (got Nt %d, Nr %d)" % (Nt, Nr))
        super().__init__(SNR, Nr=Nr, Nt=Nt, num_pilots=num_pilots, **kw)

    @staticmethod
    def _entry(eng):
        return eng.run_mimo_large_pilot_link


class CompSimulator(BatchedSimulationRunner):
    """CoMP with an external interferer and stream reduction (the reference's apps/comp_BD/simulate_comp.py and its script
    form simulate_comp_with_ext_int_simple.py): `K` cells of `Nr` x `Nr` antennas precode jointly by block diagonalisation
    while an interferer of rank `ext_int_rank` and power `Pe_dBm` disturbs every user; each of the `variants` ('None',
    'naive', 'fixed', 'capacity', 'effec_throughput': EnhancedBD with that metric; 'Whitening': WhiteningBD) is run on the
    same realizations -- one Engine.run_comp per variant and batch on the same seed, so the variants share channel, data,
    interferer and noise draws (the app draws fresh noise per metric; the statistics are the same).  'SNR' and 'Pe_dBm' are
    unpacked.  The transmit power follows the app's rule (pathloss.transmit_power_for_border_loss): SNR at the cell border,
    whose loss is `path_loss_border` (default: PathLoss3GPP1 at 1 km when a path loss is given, else 1).

    `pathloss` [K, K] (rx user, tx cell) and `pathloss_ext` [K, ext_int_rank]: arrays, or `pathloss` a callable
    (first, count) -> [count, K, K + ext_int_rank] for per-drop scenarios of the user's own.

    `user_positioning_method` (the app's parameter; not together with `pathloss`) takes the path loss from the hexagonal
    cluster of `K` cells of `cell_radius` km instead (pyphysim_amd.cell, PathLoss3GPP1 with the small-distance clamp, the
    interferer at external_radius - distance to the cluster centre): 'Random' drops one user per cell anew in EVERY
    repetition -- one Engine.run_hex_drops per batch on the variation's seed, whose resident records every variant's
    run_comp reads, no host round trip; 'Symmetric Far Away' (K = 3) places the users once at 70 % of the way to the far
    vertex of each cell and runs the fixed-matrix path.  `path_loss_border` then defaults to the model at `cell_radius`.

    Results per variant v, formed per realization and per stream as simulate_comp.py:556-621 does: 'ber_v', 'ser_v',
    'per_v' (per = 1 - (1 - ber_stream)^packet_length, errors = per x packages, summed over the streams), 'spec_effic_v'
    (sum (1 - per) Kb, RATIO against 1), 'sinr_v' (calc_JP_SINR with unit interferer power -- the app's call -- one update
    per stream).  Sums and sums of squares travel through EXTRA_KEYS, so sharding and resume keep them."""

    VARIANTS = ("None", "naive", "fixed", "capacity", "effec_throughput", "Whitening")
    _RATIOS = ("ber", "ser", "per", "spec_effic")

    def __init__(self, SNR, Pe_dBm, modulator="psk", M=4, K=3, Nr=2, ext_int_rank=1, NSymbs=500, packet_length=60,
                 N0_dBm=-116.4, variants=VARIANTS, num_streams=1, pathloss=None, pathloss_ext=None, path_loss_border=None,
                 rep_max=1000, seed=0, batch_size=4096, dtype="f64", demod="auto", engine=None,
                 common_random_numbers=False, process_group=None, user_positioning_method=None, cell_radius=1.0):
        super().__init__(batch_size=batch_size, process_group=process_group)
        from .pathloss import PathLoss3GPP1
        if user_positioning_method not in (None, "Random", "Symmetric Far Away"):
            raise ValueError("user_positioning_method must be None, 'Random' or 'Symmetric Far Away' (got %r)"
                             % (user_positioning_method,))
        if user_positioning_method is not None:
            if pathloss is not None or pathloss_ext is not None:
                raise ValueError("give user_positioning_method or pathloss, not both")
            if not (np.isfinite(cell_radius) and cell_radius > 0):
                raise ValueError("cell_radius must be positive (got %r)" % (cell_radius,))
            if user_positioning_method == "Symmetric Far Away" and int(K) != 3:
                raise ValueError("'Symmetric Far Away' needs K = 3 (got %d)" % int(K))
        self.user_positioning_method = user_positioning_method
        self.cell_radius = float(cell_radius)
        self.rep_max = rep_max
        self.seed = int(seed)
        self.dtype = dtype
        self.common_random_numbers = common_random_numbers
        self._engine = engine
        self.modulator = make_modulator(modulator, M, engine) if isinstance(modulator, str) else modulator
        if demod == "auto":
            demod = "slicer" if isinstance(self.modulator, QAM) else "mindist"
        self.demod_method = _lib.DEMOD_QAM_SLICER if demod == "slicer" else _lib.DEMOD_MINDIST
        self.variants = tuple(variants)
        for v in self.variants:
            if v not in self.VARIANTS:
                raise ValueError("unknown variant %r (known: %s)" % (v, ", ".join(self.VARIANTS)))
        self._pl_call = pathloss if callable(pathloss) else None
        self._pl = self._ple = None
        if pathloss is not None and self._pl_call is None:
            self._pl = np.asarray(pathloss, dtype=float)
            self._ple = np.zeros((int(K), 0)) if pathloss_ext is None else np.asarray(pathloss_ext, dtype=float)
            if self._pl.shape != (int(K), int(K)) or self._ple.shape != (int(K), int(ext_int_rank)):
                raise ValueError("pathloss must be [K, K] and pathloss_ext [K, ext_int_rank]")
        if user_positioning_method == "Symmetric Far Away":
            self._pl, self._ple = self.far_away_pathloss(self.cell_radius, int(ext_int_rank))
        if path_loss_border is None:
            if user_positioning_method is not None:
                path_loss_border = PathLoss3GPP1().calc_path_loss(self.cell_radius)
            else:
                path_loss_border = 1.0 if pathloss is None else PathLoss3GPP1().calc_path_loss(1.0)
        self.path_loss_border = float(path_loss_border)
        keys = []
        for v in self.variants:
            keys += ["%s_%s_%s" % (m, v, s) for m in self._RATIOS for s in ("value", "total", "sum", "sq")]
            keys += ["sinr_%s_sum" % v, "sinr_%s_sq" % v, "sinr_%s_n" % v, "n_%s" % v]
        self.EXTRA_KEYS = tuple(keys)
        self.params.add("SNR", np.atleast_1d(np.asarray(SNR, dtype=float)))
        self.params.add("Pe_dBm", np.atleast_1d(np.asarray(Pe_dBm, dtype=float)))
        self.params.set_unpack_parameter("SNR")
        self.params.set_unpack_parameter("Pe_dBm")
        for k, v in (("modulator", self.modulator.name), ("K", int(K)), ("Nr", int(Nr)), ("ext_int_rank", int(ext_int_rank)),
                     ("NSymbs", int(NSymbs)), ("packet_length", int(packet_length)), ("N0_dBm", float(N0_dBm)),
                     ("num_streams", int(num_streams))):
            self.params.add(k, v)

    engine = _LinkSimulator.engine
    _seed_for = _LinkSimulator._seed_for
    _bind = _LinkSimulator._bind

    @staticmethod
    def far_away_pathloss(cell_radius=1.0, ext_int_rank=1):
        """(pathloss [3, 3], pathloss_ext [3, ext_int_rank]) of the app's 'Symmetric Far Away' users (:172-213)."""
        from .cell import Cluster
        from .pathloss import PathLoss3GPP1
        cluster = Cluster(cell_radius, 3)
        cluster.add_border_users([1, 2, 3], [210, -30, 90], 0.7)
        model = PathLoss3GPP1()
        model.handle_small_distances_bool = True
        to_centre = np.array([cluster.calc_dist(u) for u in cluster.get_all_users()])
        ext = model.calc_path_loss(cluster.external_radius - to_centre)
        return (model.calc_path_loss(cluster.calc_dist_all_users_to_each_cell()),
                np.repeat(ext[:, np.newaxis], int(ext_int_rank), axis=1))

    def drop_records(self, eng, current_parameters, first_rep, count):
        """The resident path-loss records [count, K, K + ext_int_rank] of the 'Random' users of repetitions [first_rep,
        first_rep + count) of this variation."""
        p = current_parameters
        out = eng.run_hex_drops(p["K"], self.cell_radius, 1, self._seed_for(p), first_rep, count, n_ext=p["ext_int_rank"],
                                dtype=self.dtype, records=True)
        if out["flags"].any():
            raise RuntimeError("a user drop ran out of placement attempts (repetition %d)"
                               % (int(first_rep) + int(np.flatnonzero(out["flags"])[0])))
        return out["records"]

    def _run_batch(self, current_parameters, first_rep, count):
        from .pathloss import transmit_power_for_border_loss
        p = current_parameters
        eng = self._bind()
        K, r, E, NS, L = p["K"], p["Nr"], p["ext_int_rank"], p["NSymbs"], p["packet_length"]
        Kb = int(self.modulator.K)
        noise_var = 10.0 ** (p["N0_dBm"] / 10.0) / 1000.0
        pe = 10.0 ** (float(p["Pe_dBm"]) / 10.0) / 1000.0
        iPu = transmit_power_for_border_loss(p["SNR"], p["N0_dBm"], self.path_loss_border)
        per_drop = None
        if self._pl_call is not None and count:
            per_drop = eng.to_device(np.ascontiguousarray(self._pl_call(int(first_rep), int(count)), dtype=np.float64))
        elif self.user_positioning_method == "Random" and count:
            per_drop = self.drop_records(eng, p, first_rep, count)
        c = None
        slot = np.arange(K * r) % r
        for v in self.variants:
            res, a = eng.run_comp(K, r, E, NS, iPu, noise_var, pe, self._seed_for(p), first_rep, count, variant=v,
                                  num_streams=p["num_streams"], packet_length=L, pathloss=self._pl, pathloss_ext=self._ple,
                                  pathloss_per_realization=per_drop, sinr_pe=1.0, method=self.demod_method,
                                  dtype=self.dtype, per_realization=True)
            if c is None:
                c = dict(res)
            ok = a["sym_err"] != 0xFFFFFFFF
            active = (slot[None, :] < np.repeat(a["ns"], r, axis=1)) & ok[:, None]
            n_act = active.sum(axis=1).astype(float)
            sbit = np.where(active, a["stream_bit_err"], 0).astype(float)
            ssym = np.where(active, a["stream_sym_err"], 0).astype(float)
            num_bits = float(NS * Kb)
            per_s = np.where(active, 1.0 - (1.0 - sbit / num_bits) ** L, 0.0)
            packages = num_bits / L
            pairs = dict(ber=(sbit.sum(axis=1), n_act * num_bits), ser=(ssym.sum(axis=1), n_act * float(NS)),
                         per=((per_s * packages).sum(axis=1), n_act * packages),
                         spec_effic=(np.where(active, (1.0 - per_s) * Kb, 0.0).sum(axis=1), np.ones(int(count))))
            for m, (num, den) in pairs.items():
                ratio = num[ok] / den[ok]
                c["%s_%s_value" % (m, v)], c["%s_%s_total" % (m, v)] = float(num[ok].sum()), float(den[ok].sum())
                c["%s_%s_sum" % (m, v)], c["%s_%s_sq" % (m, v)] = float(ratio.sum()), float(np.square(ratio).sum())
            s = a["sinr"][active]
            c["sinr_%s_sum" % v], c["sinr_%s_sq" % v] = float(s.sum()), float(np.square(s).sum())
            c["sinr_%s_n" % v], c["n_%s" % v] = float(s.size), float(ok.sum())
        if c is None:
            c = {k: 0 for k in self.COUNTER_KEYS + ("n_symbols", "n_bits")}
        return c

    def _results_from_counters(self, current_parameters, c):
        from .simulations import Result, SimulationResults
        res = SimulationResults()
        g = lambda k: float(c.get(k, 0.0))
        for v in self.variants:
            n = int(round(g("n_%s" % v)))
            for m in self._RATIOS:
                res.add_result(Result.from_batch("%s_%s" % (m, v), Result.RATIOTYPE, g("%s_%s_value" % (m, v)),
                                                 g("%s_%s_total" % (m, v)), g("%s_%s_sum" % (m, v)), g("%s_%s_sq" % (m, v)), n))
            ns = int(round(g("sinr_%s_n" % v)))
            res.add_result(Result.from_batch("sinr_%s" % v, Result.RATIOTYPE, g("sinr_%s_sum" % v), float(ns),
                                             g("sinr_%s_sum" % v), g("sinr_%s_sq" % v), ns))
        return res


class MetisDropSimulator(BatchedSimulationRunner):
    """Monte Carlo over user drops on one floor of the METIS indoor scenario (the reference's
    apps/metis_scenarios/simulate_metis_scenario2.py runs ONE drop per call): `num_rooms_per_side`^2 square rooms of
    `side_length` metres, APs by `ap_decimation` (1, 2, 4, 9), `num_users` users dropped uniformly, best-channel association on
    METIS PS7 plus `single_wall_loss_dB` per wall, the APs nobody chose switched off (`active_only=False` leaves all on).  A
    repetition is a drop; one Engine.run_indoor_drops per batch.  Any of the scalars may be a list: every combination is one
    parameter variation.

    Results: 'sinr_dB' and 'capacity' (RATIO against users: the mean per user), 'sum_capacity' and 'active_aps' (RATIO against
    drops), 'sinr_histogram' (CHOICE over hist_bins + 2 slots of width hist_step_dB from hist_lo_dB: below, the bins, at or
    above the top).  Sums and the histogram travel through EXTRA_KEYS, so sharding and partial-result resume keep them."""

    _SUMS = ("users", "sinr_dB_sum", "sinr_dB_sq", "capacity_sum", "capacity_sq", "active_aps_sum", "active_aps_sq")
    _SCALARS = ("num_rooms_per_side", "side_length", "single_wall_loss_dB", "ap_decimation", "Pt_dBm", "noise_power_dBm",
                "num_users")

    def __init__(self, num_rooms_per_side=12, side_length=10.0, single_wall_loss_dB=5.0, ap_decimation=1, Pt_dBm=20.0,
                 noise_power_dBm=None, num_users=100, rep_max=1000, fc_MHz=900.0, active_only=True, hist_bins=60,
                 hist_lo_dB=-10.0, hist_step_dB=1.0, seed=0, batch_size=4096, dtype="f32", engine=None,
                 common_random_numbers=False, process_group=None):
        super().__init__(batch_size=batch_size, process_group=process_group)
        if noise_power_dBm is None:
            from .noise import calc_thermal_noise_power_dBm
            noise_power_dBm = calc_thermal_noise_power_dBm(25, 5e6)
        self.rep_max = rep_max
        self.seed = int(seed)
        self.dtype = dtype
        self.common_random_numbers = common_random_numbers
        self._engine = engine
        self.fc_MHz, self.active_only = float(fc_MHz), bool(active_only)
        self.hist_bins, self.hist_lo_dB, self.hist_step_dB = int(hist_bins), float(hist_lo_dB), float(hist_step_dB)
        self.EXTRA_KEYS = self._SUMS + tuple("sinr_h%d" % i for i in range(self.hist_bins + 2))
        self.EXTRA_INT_KEYS = ("users", "active_aps_sum", "active_aps_sq") + self.EXTRA_KEYS[len(self._SUMS):]
        values = dict(zip(self._SCALARS, (num_rooms_per_side, side_length, single_wall_loss_dB, ap_decimation, Pt_dBm,
                                          noise_power_dBm, num_users)))
        for k, v in values.items():
            if np.ndim(v) > 0:
                self.params.add(k, np.asarray(v))
                self.params.set_unpack_parameter(k)
            else:
                self.params.add(k, v)

    engine = _LinkSimulator.engine
    _seed_for = _LinkSimulator._seed_for

    def drop_args(self, current_parameters):
        """The variation as keyword arguments of Engine.run_indoor_drops."""
        from .util import dBm2Linear
        p = current_parameters
        return dict(rooms_per_side=int(p["num_rooms_per_side"]), side_length=float(p["side_length"]),
                    ap_decimation=int(p["ap_decimation"]), n_users=int(p["num_users"]), model="metis_ps7",
                    assoc="best_channel", active=self.active_only, wall_loss_dB=float(p["single_wall_loss_dB"]),
                    tx_power=float(dBm2Linear(p["Pt_dBm"])), noise_power=float(dBm2Linear(p["noise_power_dBm"])),
                    fc_MHz=self.fc_MHz, hist_bins=self.hist_bins, hist_lo_dB=self.hist_lo_dB, hist_step_dB=self.hist_step_dB,
                    dtype=self.dtype)

    def _run_batch(self, current_parameters, first_rep, count):
        out = self.engine.run_indoor_drops(seed=self._seed_for(current_parameters), first=first_rep, count=count,
                                           **self.drop_args(current_parameters))
        c = {k: 0 for k in self.COUNTER_KEYS + ("n_symbols", "n_bits")}
        c["n_realizations"] = int(count)
        U = int(current_parameters["num_users"])
        mean_db, mean_cap = out["sum_sinr_dB"] / U, out["sum_capacity"] / U        # one RATIO update per drop
        act = out["active_aps"].astype(np.int64)
        c.update(users=int(count) * U, sinr_dB_sum=float(mean_db.sum()), sinr_dB_sq=float(np.square(mean_db).sum()),
                 capacity_sum=float(out["sum_capacity"].sum()), capacity_sq=float(np.square(out["sum_capacity"]).sum()),
                 active_aps_sum=int(act.sum()), active_aps_sq=int(np.square(act).sum()))
        for i, h in enumerate(out["hist"].tolist()):
            c["sinr_h%d" % i] = int(h)
        return c

    def _results_from_counters(self, current_parameters, c):
        from .simulations import Result, SimulationResults
        res = SimulationResults()
        n = int(c["n_realizations"])
        gf = lambda k: float(c.get(k, 0.0))
        users, U = int(round(gf("users"))), int(current_parameters["num_users"])
        cap, cap_sq = gf("capacity_sum"), gf("capacity_sq")
        res.add_result(Result.from_batch("sinr_dB", Result.RATIOTYPE, gf("sinr_dB_sum") * U, users, gf("sinr_dB_sum"),
                                         gf("sinr_dB_sq"), n))
        res.add_result(Result.from_batch("capacity", Result.RATIOTYPE, cap, users, cap / U, cap_sq / (U * U), n))
        res.add_result(Result.from_batch("sum_capacity", Result.RATIOTYPE, cap, n, cap, cap_sq, n))
        act, act_sq = int(round(gf("active_aps_sum"))), int(round(gf("active_aps_sq")))
        res.add_result(Result.from_batch("active_aps", Result.RATIOTYPE, act, n, float(act), float(act_sq), n))
        hist = [int(round(gf("sinr_h%d" % i))) for i in range(self.hist_bins + 2)]
        res.add_result(Result.from_histogram("sinr_histogram", hist))
        return res


class HexDropSimulator(BatchedSimulationRunner):
    """Monte Carlo over user drops in a cluster of hexagonal cells -- the system-level experiment the reference's cell.Cluster
    exists for: `num_cells` (1 .. 19) cells of `cell_radius` km, `users_per_cell` users dropped uniformly in every cell at
    least `min_dist_ratio` radii from its base station, each served by its own cell while every other cell interferes;
    PathLoss3GPP1 with the small-distance clamp; optionally an external interferer of `ext_power_dBm` at the cluster's
    external radius and wrap around (19 cells).  A repetition is a drop; one Engine.run_hex_drops per batch.  Any of the
    scalars may be a list: every combination is one parameter variation.

    Results: 'sinr_dB' and 'capacity' (RATIO against users: the mean per user), 'sum_capacity' and 'min_sinr_dB' (RATIO
    against drops), 'sinr_histogram' (CHOICE over hist_bins + 2 slots of width hist_step_dB from hist_lo_dB: below, the bins,
    at or above the top).  Sums and the histogram travel through EXTRA_KEYS, so sharding and partial-result resume keep
    them.  A drop the device flags (a user out of placement attempts: probability below 1e-17 per user) is left out."""

    _SUMS = ("users", "drops", "sinr_dB_sum", "sinr_dB_sq", "capacity_sum", "capacity_sq", "min_sinr_dB_sum", "min_sinr_dB_sq")
    _SCALARS = ("num_cells", "cell_radius", "users_per_cell", "Pt_dBm", "noise_power_dBm", "min_dist_ratio", "ext_power_dBm")

    def __init__(self, num_cells=19, cell_radius=1.0, users_per_cell=10, Pt_dBm=46.0, noise_power_dBm=-104.0,
                 min_dist_ratio=0.0, ext_power_dBm=None, wrap_around=False, rep_max=1000, hist_bins=60, hist_lo_dB=-10.0,
                 hist_step_dB=1.0, seed=0, batch_size=4096, dtype="f32", engine=None, common_random_numbers=False,
                 process_group=None):
        super().__init__(batch_size=batch_size, process_group=process_group)
        self.rep_max = rep_max
        self.seed = int(seed)
        self.dtype = dtype
        self.common_random_numbers = common_random_numbers
        self._engine = engine
        self.wrap_around = bool(wrap_around)
        self.hist_bins, self.hist_lo_dB, self.hist_step_dB = int(hist_bins), float(hist_lo_dB), float(hist_step_dB)
        self.EXTRA_KEYS = self._SUMS + tuple("sinr_h%d" % i for i in range(self.hist_bins + 2))
        self.EXTRA_INT_KEYS = ("users", "drops") + self.EXTRA_KEYS[len(self._SUMS):]
        values = dict(zip(self._SCALARS, (num_cells, cell_radius, users_per_cell, Pt_dBm, noise_power_dBm, min_dist_ratio,
                                          -np.inf if ext_power_dBm is None else ext_power_dBm)))
        for k, v in values.items():
            if np.ndim(v) > 0:
                self.params.add(k, np.asarray(v))
                self.params.set_unpack_parameter(k)
            else:
                self.params.add(k, v)

    engine = _LinkSimulator.engine
    _seed_for = _LinkSimulator._seed_for

    def drop_args(self, current_parameters):
        """The variation as keyword arguments of Engine.run_hex_drops."""
        from .util import dBm2Linear
        p = current_parameters
        pe = float(p["ext_power_dBm"])
        return dict(num_cells=int(p["num_cells"]), cell_radius=float(p["cell_radius"]), users_per_cell=int(p["users_per_cell"]),
                    model="general", wrap_around=self.wrap_around, min_dist_ratio=float(p["min_dist_ratio"]),
                    tx_power=float(dBm2Linear(p["Pt_dBm"])), noise_power=float(dBm2Linear(p["noise_power_dBm"])),
                    ext_power=float(dBm2Linear(pe)) if np.isfinite(pe) else 0.0, hist_bins=self.hist_bins,
                    hist_lo_dB=self.hist_lo_dB, hist_step_dB=self.hist_step_dB, dtype=self.dtype)

    def _run_batch(self, current_parameters, first_rep, count):
        out = self.engine.run_hex_drops(seed=self._seed_for(current_parameters), first=first_rep, count=count, per_user=True,
                                        **self.drop_args(current_parameters))
        c = {k: 0 for k in self.COUNTER_KEYS + ("n_symbols", "n_bits")}
        c["n_realizations"] = int(count)
        KU = int(current_parameters["num_cells"]) * int(current_parameters["users_per_cell"])
        ok = out["flags"] == 0
        mean_db = out["sinr_dB"][ok].sum(axis=1) / KU                               # one RATIO update per drop
        cap, low = out["sum_capacity"][ok], out["min_sinr_dB"][ok]
        c.update(users=int(ok.sum()) * KU, drops=int(ok.sum()), sinr_dB_sum=float(mean_db.sum()),
                 sinr_dB_sq=float(np.square(mean_db).sum()), capacity_sum=float(cap.sum()), capacity_sq=float(np.square(cap).sum()),
                 min_sinr_dB_sum=float(low.sum()), min_sinr_dB_sq=float(np.square(low).sum()))
        for i, h in enumerate(out["hist"].tolist()):
            c["sinr_h%d" % i] = int(h)
        return c

    def _results_from_counters(self, current_parameters, c):
        from .simulations import Result, SimulationResults
        res = SimulationResults()
        gf = lambda k: float(c.get(k, 0.0))
        users, n = int(round(gf("users"))), int(round(gf("drops")))
        KU = int(current_parameters["num_cells"]) * int(current_parameters["users_per_cell"])
        cap, cap_sq = gf("capacity_sum"), gf("capacity_sq")
        res.add_result(Result.from_batch("sinr_dB", Result.RATIOTYPE, gf("sinr_dB_sum") * KU, users, gf("sinr_dB_sum"),
                                         gf("sinr_dB_sq"), n))
        res.add_result(Result.from_batch("capacity", Result.RATIOTYPE, cap, users, cap / KU, cap_sq / (KU * KU), n))
        res.add_result(Result.from_batch("sum_capacity", Result.RATIOTYPE, cap, n, cap, cap_sq, n))
        res.add_result(Result.from_batch("min_sinr_dB", Result.RATIOTYPE, gf("min_sinr_dB_sum"), n, gf("min_sinr_dB_sum"),
                                         gf("min_sinr_dB_sq"), n))
        hist = [int(round(gf("sinr_h%d" % i))) for i in range(self.hist_bins + 2)]
        res.add_result(Result.from_histogram("sinr_histogram", hist))
        return res


class GeneralIaSimulator(BatchedSimulationRunner):
    """The IA link on any geometry the general solver covers (the reference's apps/ia/simulate_ia.py with Nr, Nt, Ns as
    parameters -- apps/ia/IA_Results_NrxNt(Ns).py runs K = 3, Nr = 5, Nt = 3, Ns = 2 -- and apps/ia/simulate_greedy_ia.py,
    3 x 3 with Ns = 3 under a stream-selection wrapper): `K` <= 4 users of `Nr` x `Nt` <= 6 x 6 antennas, `Ns` configured
    streams per user (a scalar or one value per user), `solver` 'alt_min' / 'min_leakage' / 'max_sinr' from a 'random' or
    'svd' start, `stream_selection` None / 'greedy' (GreedStreamIASolver) / 'brute' (BruteForceStreamIASolver, always from
    'svd').  One Engine.run_ia_general per batch: channel and start drawn on the device, the solver of
    Engine.ia_solve_general, NSymbs symbols per KEPT stream.  'SNR' is unpacked.

    Results, formed per realization with that realization's own totals as the two apps form them: 'symbol_errors',
    'num_symbols', 'bit_errors', 'num_bits' (SUM); 'ber', 'ser' (RATIO against the bits / symbols actually sent);
    'sum_capacity', 'ia_runned_iterations' (RATIO against 1); with a stream selection 'stream_statistics' (CHOICE: index
    ravel_multi_index(Ns_final - 1, Ns_configured) of prod(Ns_configured) choices, simulate_greedy_ia.py:417-426).  A
    realization the solver flags is left out of every Result.  Sums travel through EXTRA_KEYS (the histogram as one key per
    choice), so sharding and resume keep them.

    Not covered: the closed-form and MMSE solvers, which exist on the 3-user 2 x 2 one-stream geometry only (IaSimulator);
    the apps' 'ia_cost' Result; a transmit power other than 1 and path loss -- the greedy app's 'NoPathLoss' scenario is this
    link in the normalisation of simulate_ia.py: P = 1, noise_var = 1 / SNR."""

    SOLVERS = ("alt_min", "min_leakage", "max_sinr")
    _SUMS = ("sent_symbols", "sent_symbols_sq", "ber_sum", "ber_sq", "ser_sum", "ser_sq", "sum_capacity", "sum_capacity_sq",
             "ia_runned_iterations", "ia_runned_iterations_sq")
    EXTRA_INT_KEYS = ("sent_symbols", "sent_symbols_sq", "ia_runned_iterations", "ia_runned_iterations_sq")

    def __init__(self, SNR, K=3, Nr=3, Nt=3, Ns=2, solver="max_sinr", stream_selection=None, initialize_with="random",
                 max_iterations=60, relative_factor=1e-6, modulator="qam", M=16, NSymbs=200, rep_max=1000, seed=0,
                 batch_size=4096, dtype="f64", demod="auto", engine=None, common_random_numbers=False, process_group=None):
        super().__init__(batch_size=batch_size, process_group=process_group)
        if solver not in self.SOLVERS:
            raise ValueError("the general-geometry solvers are 'alt_min', 'min_leakage' and 'max_sinr' (got %r); the closed "
                             "form and MMSE exist for K = 3, 2 x 2, Ns = 1 only: IaSimulator" % (solver,))
        if stream_selection not in (None, "greedy", "brute"):
            raise ValueError("stream_selection must be None, 'greedy' or 'brute'")
        if initialize_with not in ("random", "svd"):
            raise ValueError("initialize_with must be 'random' or 'svd'")
        K = int(K)
        ns = [int(Ns)] * K if np.isscalar(Ns) else [int(n) for n in Ns]
        if len(ns) != K or min(ns, default=0) < 1:
            raise ValueError("Ns must be a positive int or one per user")
        self.rep_max = rep_max
        self.seed = int(seed)
        self.dtype = dtype
        self.common_random_numbers = common_random_numbers
        self._engine = engine
        self.modulator = make_modulator(modulator, M, engine) if isinstance(modulator, str) else modulator
        if demod == "auto":
            demod = "slicer" if isinstance(self.modulator, QAM) else "mindist"
        self.demod_method = _lib.DEMOD_QAM_SLICER if demod == "slicer" else _lib.DEMOD_MINDIST
        self.Ns = tuple(ns)
        self.stream_selection = stream_selection
        self.relative_factor = float(relative_factor)
        self.num_choices = int(np.prod(ns)) if stream_selection else 0
        self.EXTRA_KEYS = self._SUMS + tuple("streams_c%d" % c for c in range(self.num_choices))
        self.EXTRA_INT_KEYS = GeneralIaSimulator.EXTRA_INT_KEYS + self.EXTRA_KEYS[len(self._SUMS):]
        self.params.add("SNR", np.atleast_1d(np.asarray(SNR, dtype=float)))
        self.params.set_unpack_parameter("SNR")
        for k, v in (("modulator", self.modulator.name), ("K", K), ("Nr", int(Nr)), ("Nt", int(Nt)),
                     ("Ns", "x".join(str(n) for n in ns)), ("NSymbs", int(NSymbs)), ("solver", solver),
                     ("stream_selection", str(stream_selection)), ("initialize_with", initialize_with),
                     ("max_iterations", int(max_iterations))):
            self.params.add(k, v)

    engine = _LinkSimulator.engine
    _seed_for = _LinkSimulator._seed_for
    _bind = _LinkSimulator._bind
    _noise_var = staticmethod(_LinkSimulator._noise_var)

    def _run_batch(self, current_parameters, first_rep, count):
        p = current_parameters
        eng = self._bind()
        res, a = eng.run_ia_general(p["K"], p["Nr"], p["Nt"], self.Ns, p["NSymbs"], self._noise_var(p), self._seed_for(p),
                                    first_rep, count, solver=p["solver"], select=self.stream_selection,
                                    initialize_with=p["initialize_with"], max_iterations=p["max_iterations"],
                                    relative_factor=self.relative_factor, method=self.demod_method, dtype=self.dtype,
                                    per_realization=True)
        c = dict(res)
        ok = a["sym_err"] != 0xFFFFFFFF
        ns = a["ns"][ok].astype(np.int64)
        sent = int(p["NSymbs"]) * ns.sum(axis=1)                       # symbols the realization actually sent
        Kb = int(self.modulator.K)
        ser = a["sym_err"][ok].astype(np.float64) / sent
        ber = a["bit_err"][ok].astype(np.float64) / (sent * Kb)
        c["sent_symbols"], c["sent_symbols_sq"] = int(sent.sum()), int(np.square(sent).sum())
        c["ser_sum"], c["ser_sq"] = float(ser.sum()), float(np.square(ser).sum())
        c["ber_sum"], c["ber_sq"] = float(ber.sum()), float(np.square(ber).sum())
        if self.num_choices:
            index = np.ravel_multi_index(tuple((ns - 1).T), self.Ns) if ns.size else np.zeros(0, dtype=np.int64)
            hist = np.bincount(index, minlength=self.num_choices)
            for ch in range(self.num_choices):
                c["streams_c%d" % ch] = int(hist[ch])
        return c

    def _results_from_counters(self, current_parameters, c):
        from .simulations import Result, SimulationResults
        res = SimulationResults()
        n = int(c["n_realizations"])
        Kb = int(self.modulator.K)
        gi = lambda k: int(round(c.get(k, 0)))
        gf = lambda k: float(c.get(k, 0.0))
        sent, sent_sq = gi("sent_symbols"), gi("sent_symbols_sq")
        res.add_result(Result.from_counters("symbol_errors", Result.SUMTYPE, c["sym_errors"], c["sym_errors_sq"], 1, n))
        res.add_result(Result.from_batch("num_symbols", Result.SUMTYPE, sent, 0, float(sent), float(sent_sq), n))
        res.add_result(Result.from_counters("bit_errors", Result.SUMTYPE, c["bit_errors"], c["bit_errors_sq"], 1, n))
        res.add_result(Result.from_batch("num_bits", Result.SUMTYPE, sent * Kb, 0, float(sent * Kb), float(sent_sq * Kb * Kb), n))
        res.add_result(Result.from_batch("ber", Result.RATIOTYPE, int(c["bit_errors"]), sent * Kb, gf("ber_sum"), gf("ber_sq"), n))
        res.add_result(Result.from_batch("ser", Result.RATIOTYPE, int(c["sym_errors"]), sent, gf("ser_sum"), gf("ser_sq"), n))
        cap, cap_sq = gf("sum_capacity"), gf("sum_capacity_sq")
        res.add_result(Result.from_batch("sum_capacity", Result.RATIOTYPE, cap, n, cap, cap_sq, n))
        its, its_sq = gi("ia_runned_iterations"), gi("ia_runned_iterations_sq")
        res.add_result(Result.from_batch("ia_runned_iterations", Result.RATIOTYPE, its, n, float(its), float(its_sq), n))
        if self.num_choices:
            res.add_result(Result.from_histogram("stream_statistics", [gi("streams_c%d" % ch) for ch in range(self.num_choices)]))
        return res
