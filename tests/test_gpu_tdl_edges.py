"""GPU: the kernel-selection edges of config 3 (mcle_run_ofdm_tdl) and f1 (mcle_run_mimo_ofdm_tdl), each walked on BOTH of its
sides, in both arithmetics, against the oracle chains (oracle/chains.py::chain_ofdm_tdl / chain_mimo_ofdm_tdl) under the same Philox
keying.

Each call falls through a chain of kernels, every one of which declines what is outside its envelope:
  config 3: the two-wavefront kernel at 2048 points (siso_hw: every delay inside the prefix, orders 2 .. 5) -> the one-wavefront kernel
            (siso_wave: 256 .. 2048, <= 8 taps reaching <= min(256, N / 2) back, orders 2 .. 5, 2 .. 8 at 1024) -> complex64 at 1024 the
            matrix-core kernel (siso_mfma: delays inside the prefix) -> the batched kernels (siso_batched: orders <= 12, delays < N) ->
            the one-realization-per-workgroup kernel (siso_single);
  f1:       the parked-coefficient kernels (mimo_wave_parked: order 5 in complex128, 2 in complex64) -> the run-time-order wavefront
            kernels (mimo_wave_rt) -> the cooperative kernel (mimo_coop: Nt = Nr in {2, 4}) -> McleUnsupported.
Every case names the kernel it expects (Engine.last_kernel(), tag and polynomial order K), so the tables below read as the envelope's
boundaries; Fd is chosen through a host replay of the order rule so that K lands where a case needs it.  Per case: the tag; per-
realization symbol and bit counts against the oracle (complex128 exact; complex64 |dSER| <= 1e-4, ties only, <= 3 per realization);
the counts bit-identical under a split of the realization range."""
import math

import numpy as np
import pytest

from oracle import chains, modem as omodem
from pyphysim_amd import _lib

pytestmark = pytest.mark.gpu
SEED = 16180339
TS = 1.0 / (15e3 * 1024)
FIRST, COUNT, SPLIT = (1 << 33) + 1237, 9, 4          # a count that is not a multiple of 4 (nor of a workgroup's realizations)
TOL = {"f64": 1e-17, "f32": 1e-8}
MAX_ORDER = 12                                        # kSisoMaxOrder (siso_tdl.hpp) = kMaxOrder (mimo_tdl.hpp)


def _dt(Ts):
    """numpy.arange(Ts, ..., Ts * 1.0000000001)'s step: fl(fl(Ts + step) - Ts), as the dispatchers compute it."""
    step = Ts * 1.0000000001
    return (Ts + step) - Ts


def tdl_order(fft, cp, dmax, Fd, dtype, Ts=TS):
    """Host replay of the polynomial-order rule of both dispatchers (pipeline_siso_tdl.hip: run_ofdm_tdl_batched,
    pipeline_mimo_tdl.hip: mcle_run_mimo_ofdm_tdl): the smallest K >= 2 with z^(K+1) / (K+1)! <= tol, z the largest Doppler phase
    across half a symbol plus the reach; MAX_ORDER + 1 = beyond the tap model."""
    xc = 0.5 * (fft + cp - 1)
    z = 2.0 * 3.14159265358979323846 * abs(Fd) * _dt(Ts) * (xc + dmax)
    K, term = 1, z * z / 2.0
    while term > TOL[dtype] and K < MAX_ORDER + 1:
        K += 1
        term *= z / (K + 1)
    return max(K, 2)


def fd_for_order(K, fft, cp, dmax, dtype, Ts=TS):
    """A Doppler (Hz) in the middle (geometrically) of the interval where the order rule gives exactly K."""
    tol = TOL[dtype]
    hi = (tol * math.factorial(K + 1)) ** (1.0 / (K + 1))                 # order K suffices up to here
    lo = (tol * math.factorial(K)) ** (1.0 / K) if K > 2 else hi / 4      # order K - 1 suffices up to here
    Fd = math.sqrt(lo * hi) / (2.0 * math.pi * _dt(Ts) * (0.5 * (fft + cp - 1) + dmax))
    assert tdl_order(fft, cp, dmax, Fd, dtype, Ts) == K
    return Fd


def quarter_turn_fd(fft, cp, n_ofdm_sym, reach, Ts=TS):
    """The Doppler below which complex64 evaluates the rays' frequencies in float: the largest Doppler phase of the run, Fd x (Ts +
    dt x ((n_ofdm_sym + 1) x (N + cp) + reach)), below a quarter turn -- reach 256 in config 3 (siso_tdl.hpp), dmax in f1 (mimo_tdl.hpp)."""
    return 0.25 / (Ts + _dt(Ts) * ((n_ofdm_sym + 1) * (fft + cp) + reach))


def _profile(delays, powers_dB, Ts=TS):
    from pyphysim_amd.channels import discretize_profile
    return discretize_profile(np.asarray(powers_dB, dtype=float), np.asarray(delays, dtype=float) * Ts, Ts)


def _powers(n):
    return tuple(-1.5 * i for i in range(n))


def _set(engine, mod, M):
    engine.set_constellation(chains.constellation(mod, M), _lib.CONST_QAM if mod == "qam" else _lib.CONST_GENERIC)


def _check_counts(dtype, se, be, want_se, want_be, nsym, nbits, what):
    se, be = se.astype(np.int64), be.astype(np.int64)
    if dtype == "f64":
        assert np.array_equal(se, want_se) and np.array_equal(be, want_be), (what, se.tolist(), want_se.tolist(), be.tolist(),
                                                                            want_be.tolist())
    else:
        n = len(se)
        assert abs(int(se.sum()) - int(want_se.sum())) <= 1e-4 * n * nsym + 2, (what, se.tolist(), want_se.tolist())
        assert abs(int(be.sum()) - int(want_be.sum())) <= 1e-4 * n * nbits + 2, (what, be.tolist(), want_be.tolist())
        assert np.max(np.abs(se - want_se)) <= 3, (what, se.tolist(), want_se.tolist())          # boundary ties only


# ---- config 3 ---------------------------------------------------------------------------------------------------------------------
_ORACLE_C3 = {}


def _c3_oracle(mod, M, fft, cp, used, n_sym, snr_db, Fd, delays, powers):
    key = (mod, M, fft, cp, used, n_sym, snr_db, Fd, delays, powers)
    if key not in _ORACLE_C3:
        okw = dict(mod=mod, M=M, fft_size=fft, cp_size=cp, num_used=used, n_ofdm_sym=n_sym, snr_db=snr_db, Fd=Fd, Ts=TS, L=8,
                   tap_powers_dB=powers, tap_delays_samples=delays, linear_mean=True)
        out = [chains.chain_ofdm_tdl(chains.PhiloxRng(SEED, r), **okw) for r in range(FIRST, FIRST + COUNT)]
        _ORACLE_C3[key] = (np.array([o["symbol_errors"] for o in out], dtype=np.int64),
                           np.array([o["bit_errors"] for o in out], dtype=np.int64), out[0]["num_symbols"], out[0]["num_bits"])
    return _ORACLE_C3[key]


def _c3_walk(engine, dtype, want_tag, fft, cp, delays, Fd, n_sym=1, used=None, mod="qam", M=16, snr_db=22.0, powers=None):
    """One config-3 case: the kernel's tag, per-realization counts against the oracle, counts under a split of the range."""
    powers = tuple(powers) if powers is not None else _powers(len(delays))
    delays = tuple(delays)
    used = used or fft
    _set(engine, mod, M)
    want_se, want_be, nsym, nbits = _c3_oracle(mod, M, fft, cp, used, n_sym, snr_db, Fd, delays, powers)
    p_lin, d_idx = _profile(delays, powers)
    nv = 1.0 / omodem.dB2Linear(snr_db)

    def run(first, count):
        return engine.run_ofdm_tdl(fft, cp, used, n_sym, nv, p_lin, d_idx, SEED, first, count, Fd=Fd, Ts=TS, L=8, dtype=dtype,
                                   per_realization=True)

    res, se, be = run(FIRST, COUNT)
    tag = engine.last_kernel()
    assert res["n_symbols"] == nsym and res["n_bits"] == nbits and res["n_realizations"] == COUNT
    _check_counts(dtype, se, be, want_se, want_be, nsym, nbits, (tag, Fd))
    assert tag == want_tag, (tag, want_tag, Fd)
    a = run(FIRST, SPLIT)
    b = run(FIRST + SPLIT, COUNT - SPLIT)
    assert np.array_equal(np.concatenate([a[1], b[1]]), se) and np.array_equal(np.concatenate([a[2], b[2]]), be)
    return tag


D5 = (0, 1, 2, 3, 4)                                  # the benchmark's five taps
D8, D9 = (0, 1, 7, 33, 64, 65, 130, 200), (0, 1, 7, 33, 64, 65, 130, 200, 201)


def _both(tag):
    return {"f64": tag, "f32": tag}


# (name, dict(fft, cp, delays, K = the target polynomial order [, n_sym]), expected tag per arithmetic)
C3_ORDER = [
    # 1024: the one-wavefront kernel at every order 2 .. 8; order 9 -> complex64 the matrix-core kernel, complex128 the batched one
    *[("order1024_K%d" % k, dict(fft=1024, cp=16, delays=D5, K=k), _both("siso_wave N=1024 K=%d" % k)) for k in range(2, 9)],
    ("order1024_K9", dict(fft=1024, cp=16, delays=D5, K=9), {"f64": "siso_batched K=9", "f32": "siso_mfma"}),
    # orders 12 (the batched kernels' last: five taps x 14 coefficients are too many for the matrix-core kernel's pass) and 13
    ("order1024_K12", dict(fft=1024, cp=16, delays=D5, K=12), _both("siso_batched K=12")),
    ("order1024_K13", dict(fft=1024, cp=16, delays=D5, K=13), _both("siso_single")),
    # 256 / 512: the one-wavefront kernel up to order 5; 2048: the two-wavefront kernel up to order 5 -- then the batched kernels
    *[("order%d_K%d" % (n, k), dict(fft=n, cp=16, delays=D5, K=k),
       _both(("siso_hw K=%d" % k if n == 2048 else "siso_wave N=%d K=%d" % (n, k)) if k == 5 else "siso_batched K=%d" % k))
      for n in (256, 512, 2048) for k in (5, 6)],
]
C3_REACH = [
    # every delay inside the prefix at 2048 (the two-wavefront kernel) / one sample beyond it (the one-wavefront kernel)
    ("prefix2048_in", dict(fft=2048, cp=64, delays=(0, 5, 30, 64), K=3, n_sym=3), _both("siso_hw K=3")),
    ("prefix2048_out", dict(fft=2048, cp=64, delays=(0, 5, 30, 65), K=3, n_sym=3), _both("siso_wave N=2048 K=3")),
    # the wavefront kernels' reach: 256 samples (and N / 2)
    ("reach512_256", dict(fft=512, cp=256, delays=(0, 9, 256), K=3), _both("siso_wave N=512 K=3")),
    ("reach512_257", dict(fft=512, cp=257, delays=(0, 9, 257), K=3), _both("siso_batched K=3")),
    ("reach1024_256", dict(fft=1024, cp=256, delays=(0, 9, 256), K=3), _both("siso_wave N=1024 K=3")),
    ("reach1024_257", dict(fft=1024, cp=257, delays=(0, 9, 257), K=3), {"f64": "siso_batched K=3", "f32": "siso_mfma"}),
    # (complex128: the two-wavefront kernel's planes for a 256-sample reach leave one workgroup per CU -- it declines)
    ("reach2048_256", dict(fft=2048, cp=256, delays=(0, 9, 256), K=3), {"f64": "siso_wave N=2048 K=3", "f32": "siso_hw K=3"}),
    ("reach2048_257", dict(fft=2048, cp=257, delays=(0, 9, 257), K=3), _both("siso_batched K=3")),
    ("reach256_128", dict(fft=256, cp=128, delays=(0, 9, 128), K=3), _both("siso_wave N=256 K=3")),
    ("reach256_129", dict(fft=256, cp=129, delays=(0, 9, 129), K=3), _both("siso_batched K=3")),
    # a delay of a whole symbol with no prefix: the entry point accepts it, the batched kernels do not (delays < N)
    ("reach256_fft", dict(fft=256, cp=0, delays=(0, 255), K=3), _both("siso_batched K=3")),
    ("reach256_fft_plus", dict(fft=256, cp=0, delays=(0, 256), K=3), _both("siso_single")),
    # eight taps (kWaveMaxTaps) / nine
    ("taps8", dict(fft=1024, cp=208, delays=D8, K=3), _both("siso_wave N=1024 K=3")),
    ("taps9", dict(fft=1024, cp=208, delays=D9, K=3), {"f64": "siso_batched K=3", "f32": "siso_mfma"}),
]
# the Doppler's sign: Fd = 0, and negative Fd at the orders above (1024) and at the two-wavefront kernel's last order (2048)
C3_SIGN = [("fd0", dict(fft=1024, cp=16, delays=D5, Fd=0.0), _both("siso_wave N=1024 K=2"))] + [
    ("neg_" + name, dict(kw, sign=-1), tags) for name, kw, tags in C3_ORDER if kw["fft"] == 1024 or name == "order2048_K5"]
C3_CASES = C3_ORDER + C3_REACH + C3_SIGN


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", [c[0] for c in C3_CASES])
def test_config3_edge(engine, name, dtype):
    _, kw, tags = next(c for c in C3_CASES if c[0] == name)
    kw = dict(kw)
    fft, cp, delays = kw["fft"], kw["cp"], kw["delays"]
    if "K" in kw:
        K = kw["K"]
        Fd = kw.get("sign", 1) * fd_for_order(K, fft, cp, max(delays), dtype)
    else:
        Fd = kw["Fd"]
    _c3_walk(engine, dtype, tags[dtype], fft, cp, delays, Fd, n_sym=kw.get("n_sym", 1), used=kw.get("used"))


@pytest.mark.parametrize("fft,n_sym", [(1024, 1), (2048, 2)])
@pytest.mark.parametrize("side", [-1, 1])
def test_config3_quarter_turn_complex64(engine, fft, n_sym, side):
    """complex64 one part in 1e3 below / above the quarter-turn Doppler (v_cos_f32 ray frequencies below it, f64 above): the same
    kernel and order on both sides (the choice is inside the record kernel); counts against the oracle on both."""
    thr = quarter_turn_fd(fft, 16, n_sym, 256)
    Fd = thr * (1.0 + side * 1e-3)
    K = tdl_order(fft, 16, 4, Fd, "f32")
    tag = "siso_wave N=1024 K=%d" % K if fft == 1024 else "siso_batched K=%d" % K
    _c3_walk(engine, "f32", tag, fft, 16, D5, Fd, n_sym=n_sym, snr_db=24.0)


@pytest.mark.parametrize("n_sym", [1, 3])
def test_config3_quarter_turn_crossed_by_the_number_of_symbols(engine, n_sym):
    """One Doppler below the quarter turn over one symbol and above it over three: complex64 counts follow the oracle on both."""
    lo, hi = quarter_turn_fd(1024, 16, 3, 256), quarter_turn_fd(1024, 16, 1, 256)
    Fd = math.sqrt(lo * hi)
    assert quarter_turn_fd(1024, 16, 3, 256) < Fd < quarter_turn_fd(1024, 16, 1, 256)
    K = tdl_order(1024, 16, 4, Fd, "f32")
    _c3_walk(engine, "f32", "siso_wave N=1024 K=%d" % K, 1024, 16, D5, Fd, n_sym=n_sym, snr_db=24.0)


@pytest.mark.parametrize("case", range(5))
def test_a_delay_beyond_the_prefix_in_complex64(engine, case):
    """tests/test_gpu_tdl_wave.py::ISI_CASES (a tap delay beyond the cyclic prefix) in complex64 against the oracle, with the split."""
    from test_gpu_tdl_wave import ISI_CASES
    kw = dict(ISI_CASES[case])
    fft, cp, delays = kw["fft"], kw["cp_size"], kw["tap_delays_samples"]
    K = tdl_order(fft, cp, max(delays), 10.0, "f32")
    _c3_walk(engine, "f32", "siso_wave N=%d K=%d" % (fft, K), fft, cp, delays, 10.0, n_sym=kw["n_ofdm_sym"], used=kw.get("num_used"),
             mod=kw["mod"], M=kw["M"], snr_db=kw["snr_db"], powers=kw.get("tap_powers_dB", (0.0, -3.0, -6.0, -9.0, -12.0)))


def test_last_kernel_is_empty_before_and_after_a_refused_call():
    from pyphysim_amd.engine import Engine
    eng = Engine(0, "f64")
    try:
        assert eng.last_kernel() == ""
        _set(eng, "qpsk", 4)
        p_lin, d_idx = _profile(D5, _powers(5))
        eng.run_ofdm_tdl(1024, 16, 1024, 1, 0.01, p_lin, d_idx, SEED, 0, 3, Fd=10.0, Ts=TS)
        assert eng.last_kernel().startswith("siso_wave N=1024 K=")
        with pytest.raises(_lib.McleError):
            eng.run_ofdm_tdl(1024, 16, 1024, 1, 0.01, p_lin, d_idx, SEED, 0, 3, Fd=float("nan"), Ts=TS)
        assert eng.last_kernel() == ""
    finally:
        eng.close()


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_config2_and_config3_refuse_a_doppler_that_is_not_finite(engine, bad):
    _set(engine, "qpsk", 4)
    p_lin, d_idx = _profile(D5, _powers(5))
    with pytest.raises(_lib.McleError, match="Fd"):
        engine.run_ofdm_tdl(1024, 16, 1024, 1, 0.01, p_lin, d_idx, SEED, 0, 3, Fd=bad, Ts=TS)
    with pytest.raises(_lib.McleError, match="Fd"):
        engine.run_flat_fading(1000, 0.01, SEED, 0, 3, Fd=bad, Ts=1e-3)


# ---- f1 -------------------------------------------------------------------------------------------------------------------------
def _f1_walk(engine, dtype, want_tag, fft, cp, delays, Fd, nt=4, nr=4, n_sym=1, mod="qam", M=16, snr_db=24.0):
    powers = _powers(len(delays))
    _set(engine, mod, M)
    okw = dict(mod=mod, M=M, nt=nt, nr=nr, fft_size=fft, cp_size=cp, num_used=None, n_ofdm_sym=n_sym, snr_db=snr_db, Fd=Fd, Ts=TS,
               L=8, tap_powers_dB=powers, tap_delays_samples=tuple(delays), mmse=True, linear_mean=True)
    out = [chains.chain_mimo_ofdm_tdl(chains.PhiloxRng(SEED, r), **okw) for r in range(FIRST, FIRST + COUNT)]
    want_se = np.array([o["symbol_errors"] for o in out], dtype=np.int64)
    want_be = np.array([o["bit_errors"] for o in out], dtype=np.int64)
    nsym, nbits = out[0]["num_symbols"], out[0]["num_bits"]
    p_lin, d_idx = _profile(delays, powers)
    nv = 1.0 / omodem.dB2Linear(snr_db)

    def run(first, count):
        return engine.run_mimo_ofdm_tdl(nt, nr, fft, cp, fft, n_sym, nv, p_lin, d_idx, SEED, first, count, Fd=Fd, Ts=TS, L=8,
                                        dtype=dtype, per_realization=True)

    res, se, be = run(FIRST, COUNT)
    tag = engine.last_kernel()
    assert res["n_symbols"] == nsym and res["n_bits"] == nbits and res["n_realizations"] == COUNT
    _check_counts(dtype, se, be, want_se, want_be, nsym, nbits, (tag, Fd))
    assert tag == want_tag, (tag, want_tag, Fd)
    a = run(FIRST, SPLIT)
    b = run(FIRST + SPLIT, COUNT - SPLIT)
    assert np.array_equal(np.concatenate([a[1], b[1]]), se) and np.array_equal(np.concatenate([a[2], b[2]]), be)


# the parked-coefficient kernels' order (5 in complex128, 2 in complex64) and the next one (the run-time-order kernels)
F1_ORDER = [(dtype, fft, K, ("mimo_wave_parked K=%d" if K == parked else "mimo_wave_rt K=%d") % K)
            for dtype, parked in (("f64", 5), ("f32", 2)) for fft in (1024, 512) for K in (parked, parked + 1)]


@pytest.mark.parametrize("dtype,fft,K,tag", F1_ORDER)
def test_f1_order_edge(engine, dtype, fft, K, tag):
    _f1_walk(engine, dtype, tag, fft, 16, D5, fd_for_order(K, fft, 16, 4, dtype))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_f1_beyond_the_largest_order_is_unsupported(engine, dtype):
    Fd = fd_for_order(MAX_ORDER + 1, 1024, 16, 4, dtype)
    _set(engine, "qam", 16)
    p_lin, d_idx = _profile(D5, _powers(5))
    with pytest.raises(_lib.McleUnsupported):
        engine.run_mimo_ofdm_tdl(4, 4, 1024, 16, 1024, 1, 0.01, p_lin, d_idx, SEED, FIRST, COUNT, Fd=Fd, Ts=TS, dtype=dtype)
    assert engine.last_kernel() == ""
    # the order below it still runs (on the run-time-order kernels)
    Fd = fd_for_order(MAX_ORDER, 1024, 16, 4, dtype)
    engine.run_mimo_ofdm_tdl(4, 4, 1024, 16, 1024, 1, 0.01, p_lin, d_idx, SEED, FIRST, 3, Fd=Fd, Ts=TS, dtype=dtype)
    assert engine.last_kernel() == "mimo_wave_rt K=%d" % MAX_ORDER


@pytest.mark.parametrize("side", [-1, 1])
def test_f1_quarter_turn_complex64(engine, side):
    Fd = quarter_turn_fd(1024, 16, 1, 4) * (1.0 + side * 1e-3)
    K = tdl_order(1024, 16, 4, Fd, "f32")
    _f1_walk(engine, "f32", "mimo_wave_rt K=%d" % K, 1024, 16, D5, Fd, snr_db=26.0)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("dmax", [256, 257])
def test_f1_reach_edge(engine, dtype, dmax):
    """4 x 4: the wavefront kernels up to 256 samples back, the cooperative kernel beyond; 2 x 3 (no cooperative kernel): refused."""
    K = {"f64": 5, "f32": 2}[dtype]
    delays = (0, 9, dmax)
    Fd = fd_for_order(K, 1024, dmax, dmax, dtype)
    _f1_walk(engine, dtype, "mimo_wave_parked K=%d" % K if dmax <= 256 else "mimo_coop", 1024, dmax, delays, Fd)
    if dmax <= 256:
        _f1_walk(engine, dtype, "mimo_wave_parked K=%d" % K, 1024, dmax, delays, Fd, nt=2, nr=3)
    else:
        p_lin, d_idx = _profile(delays, _powers(3))
        with pytest.raises(_lib.McleUnsupported):
            engine.run_mimo_ofdm_tdl(2, 3, 1024, dmax, 1024, 1, 0.01, p_lin, d_idx, SEED, FIRST, COUNT, Fd=Fd, Ts=TS, dtype=dtype)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_f1_refuses_a_negative_doppler(engine, dtype):
    _set(engine, "qam", 16)
    p_lin, d_idx = _profile(D5, _powers(5))
    with pytest.raises(_lib.McleError, match="Fd"):
        engine.run_mimo_ofdm_tdl(4, 4, 1024, 16, 1024, 1, 0.01, p_lin, d_idx, SEED, FIRST, COUNT, Fd=-10.0, Ts=TS, dtype=dtype)


# ---- config 2: the sign of the Doppler does not matter to the flat-fading pipeline either ------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_config2_negative_doppler(engine, dtype):
    kw = dict(mod="qam", M=16, N=5000, snr_db=18.0, Fd=-100.0, Ts=1e-3, L=8)
    _set(engine, "qam", 16)
    out = [chains.chain_flat_jakes(chains.PhiloxRng(SEED, r), **kw) for r in range(FIRST, FIRST + COUNT)]
    want_se = np.array([o["symbol_errors"] for o in out], dtype=np.int64)
    want_be = np.array([o["bit_errors"] for o in out], dtype=np.int64)
    nv = 1.0 / omodem.dB2Linear(18.0)

    def run(first, count):
        return engine.run_flat_fading(5000, nv, SEED, first, count, Fd=-100.0, Ts=1e-3, L=8, dtype=dtype, per_realization=True)

    res, se, be = run(FIRST, COUNT)
    assert res["n_realizations"] == COUNT
    _check_counts(dtype, se, be, want_se, want_be, out[0]["num_symbols"], out[0]["num_bits"], "config 2")
    a = run(FIRST, SPLIT)
    b = run(FIRST + SPLIT, COUNT - SPLIT)
    assert np.array_equal(np.concatenate([a[1], b[1]]), se) and np.array_equal(np.concatenate([a[2], b[2]]), be)
