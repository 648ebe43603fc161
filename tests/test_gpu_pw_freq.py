"""The part-wave complex128 kernel of config 4's link (csrc/pipeline_mimo_pw.hip, fft_size 512 / 1024 / 2048 = NW 2 / 4 / 8 wavefronts per
realization) in its round-7 form: the channel is flat, so  fft(H T + sigma n) = H X (tx_scale N) + fft(sigma n)  and only the noise is
transformed; the signal joins the noise spectrum on v_mfma_f64_4x4x4 in front of the decode.  The default
(f64_threads = 0, at 1024 also 263 / 264); f64_threads = 265 = the time-domain form of round 6, the second witness.

GPU: per-realization symbol AND bit error counts equal to the oracle chain's (oracle/chains.py::chain_mimo_ofdm) for BOTH forms at
every size, both demodulators, MMSE and ZF, one and three OFDM symbols, prefix 0 and 16, QPSK / 16- / 64- / 256-QAM, 40 dB and 5 dB;
requests outside the envelope (odd prefix, partial band) served by the planar kernel with the oracle's counts and ITS tag; the
new form against the time-domain form over 4 096 realizations per size with the tag (mcle_ctx_last_kernel) naming the form that ran,
totals invariant under a split of the range, runs bit-identical.
CPU: a NumPy replay of the new form's lane maps for NW = 2, 4, 8 -- the label byte a lane supplies as B operand in register q + NW uu
is the symbol of the bin whose noise spectrum that register holds, and the scaled identity reproduces the oracle's Y to 1e-12.
Reference: apps/mimo/simulate_mimo.py:68-142, mimo/mimo.py:609-660, modulators/ofdm.py:52-94, :394-466."""
import math

import numpy as np
import pytest

from oracle import chains, modem as omodem
from pyphysim_amd import _lib

gpu = pytest.mark.gpu
SEED = 29979245

# inside the envelope (4 x 4, full band, even prefix, certificate or slicer)
CASES = [dict(mod="qam", M=64, snr_db=25.0),                                               # BASELINE config 4: MMSE, prefix 16
         dict(mod="qam", M=16, snr_db=18.0, cp_size=0, mmse=False, n_ofdm_sym=3),          # ZF, three symbols, no prefix
         dict(mod="qam", M=256, snr_db=40.0),                                              # 40 dB
         dict(mod="qpsk", M=4, snr_db=5.0, cp_size=0),                                     # 5 dB, quadrant certificate
         dict(mod="qam", M=256, snr_db=32.0, cp_size=0, n_ofdm_sym=3),
         dict(mod="qam", M=4, snr_db=8.0, mmse=False, n_ofdm_sym=3)]
# outside: odd prefix, partial band -> the planar kernel answers
OUTSIDE = [dict(mod="qam", M=16, snr_db=18.0, cp_size=7),
           dict(mod="qam", M=64, snr_db=25.0, num_used_frac=0.75, n_ofdm_sym=2)]
DEPTH = {512: 2048, 1024: 1024, 2048: 512}                     # realizations per case against the oracle
FREQ = {512: (0,), 1024: (0, 263, 264), 2048: (0,)}            # f64_threads values that select the new form
TIME = 265


def _set(engine, kw):
    engine.set_constellation(chains.constellation(kw["mod"], kw["M"]), _lib.CONST_QAM if kw["mod"] == "qam" else _lib.CONST_GENERIC)


def _used(kw, fft):
    return int(fft * kw["num_used_frac"]) if "num_used_frac" in kw else fft


def _run(engine, kw, fft, first, count, method, threads):
    nv = 1.0 / omodem.dB2Linear(kw["snr_db"])
    with engine.options(f64_threads=threads):
        out = engine.run_mimo_ofdm(4, 4, fft, kw.get("cp_size", 16), _used(kw, fft), kw.get("n_ofdm_sym", 1), nv, SEED, first, count,
                                   mmse=kw.get("mmse", True), method=method, dtype="f64", per_realization=True)
        return out + (engine.last_kernel(),)


def _oracle(kw, fft, first, count):
    okw = dict(mod=kw["mod"], M=kw["M"], nt=4, nr=4, fft_size=fft, cp_size=kw.get("cp_size", 16), num_used=_used(kw, fft),
               n_ofdm_sym=kw.get("n_ofdm_sym", 1), snr_db=kw["snr_db"], mmse=kw.get("mmse", True))
    want = [chains.chain_mimo_ofdm(chains.PhiloxRng(SEED, r), **okw) for r in range(first, first + count)]
    return np.array([w["symbol_errors"] for w in want]), np.array([w["bit_errors"] for w in want])


def _methods(kw):
    return [_lib.DEMOD_MINDIST] + ([_lib.DEMOD_QAM_SLICER] if kw["mod"] == "qam" else [])


def _tag(fft, form):
    return "mimo_ofdm_pw<%d>/%s" % (fft // 256, form)


@gpu
@pytest.mark.parametrize("fft", [512, 1024, 2048])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_both_forms_equal_the_oracle(engine, case, fft):
    """Every per-realization count of DEPTH[fft] consecutive realizations, both demodulators, the new form under each option value
    that selects it and the time-domain form."""
    kw = CASES[case]
    _set(engine, kw)
    first, count = (1 << 33) + 4711 * case, DEPTH[fft]
    want_se, want_be = _oracle(kw, fft, first, count)
    if kw["snr_db"] < 30.0:
        assert want_se.sum() > 100                                  # (the high-SNR cases mostly count nothing: equality is the point)
    for method in _methods(kw):
        for threads in FREQ[fft] + (TIME,):
            res, se, be, tag = _run(engine, kw, fft, first, count, method, threads)
            print("case %d fft %d method %d f64_threads %d: %s, symbol errors %d (oracle %d), realizations that differ %d" %
                  (case, fft, method, threads, tag, int(se.sum()), int(want_se.sum()), int(np.count_nonzero(se != want_se))))
            assert tag == _tag(fft, "time" if threads == TIME else "freq") + ("/w2" if threads == 264 else "")     # (264: the two-wavefront bound)
            assert np.array_equal(se, want_se), (threads, method, np.flatnonzero(se != want_se)[:5])
            assert np.array_equal(be, want_be), (threads, method, np.flatnonzero(be != want_be)[:5])
            assert res["n_realizations"] == count and res["n_skipped"] == 0
            assert res["sym_errors"] == int(want_se.sum()) and res["bit_errors"] == int(want_be.sum())


def _planar_tag(fft):
    """(fft, 4 x 4) complex128 outside the part-wave envelope, f64_threads in FREQ[fft] + (TIME,): 512 radix-4 with two antennas per
    thread, 1024 the fused radix-16 form, 2048 four antennas per thread (the grammar: include/mcle.h at mcle_ctx_last_kernel)."""
    return "mimo_ofdm_planar<%d,4,4> f64 %s" % (fft, {512: "ah2 w3 v0", 1024: "ah4 w2 v12", 2048: "ah4 w2 v0"}[fft])


@gpu
@pytest.mark.parametrize("fft", [512, 1024, 2048])
@pytest.mark.parametrize("case", range(len(OUTSIDE)))
def test_outside_the_envelope_the_planar_kernel_answers(engine, case, fft):
    kw = OUTSIDE[case]
    _set(engine, kw)
    first, count = 31337, 24 if fft < 2048 else 8
    want_se, want_be = _oracle(kw, fft, first, count)
    for method in _methods(kw):
        for threads in FREQ[fft] + (TIME,):
            res, se, be, tag = _run(engine, kw, fft, first, count, method, threads)
            assert tag == _planar_tag(fft), tag                     # no part-wave kernel ran: the planar form of the shape
            assert np.array_equal(se, want_se) and np.array_equal(be, want_be), (threads, method, se, want_se)
            assert res["n_realizations"] == count and res["n_skipped"] == 0


@gpu
@pytest.mark.parametrize("fft", [512, 1024, 2048])
@pytest.mark.parametrize("case", [0, 1])
def test_new_form_against_the_time_domain_form(engine, case, fft):
    """Same seed and range: equal per-realization counts over 4 096 realizations, the tag names the form that served each call, totals
    are those of any split of the range, and a second run is bit-identical."""
    kw = CASES[case]
    _set(engine, kw)
    first, n, k = 123456789, 4096, 1365
    for method in _methods(kw):
        res, se, be, tag = _run(engine, kw, fft, first, n, method, 0)
        res_t, se_t, be_t, tag_t = _run(engine, kw, fft, first, n, method, TIME)
        assert tag == _tag(fft, "freq") and tag_t == _tag(fft, "time")           # the default IS the new form
        print("fft %d case %d method %d: symbol errors %d / %d, realizations that differ %d" %
              (fft, case, method, int(se.sum()), int(se_t.sum()), int(np.count_nonzero(se != se_t))))
        assert se.sum() > 1000
        assert np.array_equal(se, se_t) and np.array_equal(be, be_t)
        assert res["n_realizations"] == res_t["n_realizations"] == n and res["n_skipped"] == res_t["n_skipped"] == 0
        a = _run(engine, kw, fft, first, k, method, 0)[0]
        b = _run(engine, kw, fft, first + k, n - k, method, 0)[0]
        for key in ("sym_errors", "sym_errors_sq", "bit_errors", "bit_errors_sq", "n_realizations", "n_skipped"):
            assert res[key] == a[key] + b[key], key
        again = _run(engine, kw, fft, first, n, method, 0)
        assert np.array_equal(again[1], se) and np.array_equal(again[2], be) and again[0] == res


# ---- CPU: the lane maps of the new form ----
def pw_mtime(h, c):
    return (c & 3) * 64 + (c >> 2) * 16 + (h & 3) * 4 + (h >> 2)


def _last_stage(Yj, NW, kp):
    """Y[k' + 256 q], q = 0 .. NW - 1, from the NW partial transforms at k' (forward), as the reading lane forms them"""
    N = 256 * NW
    x = [Yj[jj] * np.exp(-2j * np.pi * jj * kp / N) for jj in range(NW)]
    if NW == 2:
        return [x[0] + x[1], x[0] - x[1]]
    f4 = lambda u: [u[0] + u[1] + u[2] + u[3], (u[0] - u[2]) - 1j * (u[1] - u[3]), (u[0] + u[2]) - (u[1] + u[3]), (u[0] - u[2]) + 1j * (u[1] - u[3])]
    if NW == 4:
        return f4(x)
    E, O = f4([x[0], x[2], x[4], x[6]]), f4([x[1], x[3], x[5], x[7]])
    h = 0.70710678118654752440
    t = [O[0], h * (1 - 1j) * O[1], -1j * O[2], h * (-1 - 1j) * O[3]]
    return [E[q] + t[q] for q in range(4)] + [E[q] - t[q] for q in range(4)]


@pytest.mark.parametrize("NW", [2, 4, 8])
def test_lane_maps_of_the_frequency_domain_form(NW):
    """One realization of the oracle chain, two OFDM symbols, replayed the way the kernel distributes it: S0a's label bytes, the noise
    sample NW pw_mtime(h, c) + j in register c of lane (r, h) of wavefront j, a 256-point forward transform per wavefront, the last
    radix-NW stage in lane (r, g) of wavefront jw (register q + NW uu = bin k' + 256 q, k' = g + 16 (UU jw + uu)), the B operand of
    lane (a, g) = byte 16 jw + q + NW uu of its label row, and v_mfma_f64_4x4x4's lane maps (A_b[i][k] <- lane 4 b + i + 16 k,
    B_b[k][j] <- lane 4 b + j + 16 k, C / D_b[i][j] <-> lane 4 b + j + 16 i) with lane (a, h) supplying H[h mod 4][a]."""
    N, NT, cp, n_sym, M = 256 * NW, 4, 16, 2, 64
    UU, stride = 16 // NW, 16 * NW + 16
    out = chains.chain_mimo_ofdm(chains.PhiloxRng(SEED, 5), mod="qam", M=M, nt=NT, nr=4, fft_size=N, cp_size=cp, num_used=None,
                                 n_ofdm_sym=n_sym, snr_db=25.0, mmse=True)
    H, idx, noise, table = out["H"], np.asarray(out["idx"]).reshape(-1), out["noise"], out["table"]
    sigma = math.sqrt(out["noise_var"])
    tx_scale = 1.0 / math.sqrt(NT) / math.sqrt(N + cp)
    txtab = table * (tx_scale * N)                                       # s_txtab of the new form
    rx_scale = math.sqrt(N + cp) / N                                     # what the record kernel folds into G
    per_sym = N * NT
    Y = np.zeros((4, n_sym, N), complex)                                 # [r][symbol][data subcarrier d], the oracle's units
    for os_ in range(n_sym):
        # S0a: thread t draws DATA block t of the symbol: word s = subcarrier d = 4 t + s, byte a = antenna a
        lab = np.full((64, stride), -1, int)
        for t in range(64 * NW):
            q, u = (t >> 6) ^ (NW // 2), (t & 63) >> 2
            for s in range(4):
                g = 4 * (t & 3) + s
                for a in range(4):
                    lab[a * 16 + g, NW * u + q] = idx[os_ * per_sym + 16 * t + 4 * s + a]
        # the noise alone through the receive transform: per wavefront its 256 samples, lane (r, h), register c
        Yj = np.zeros((NW, 4, 256), complex)
        for j in range(NW):
            for r in range(4):
                v = np.zeros(256, complex)
                for h in range(16):
                    for c in range(16):
                        m = pw_mtime(h, c)
                        v[m] = sigma * noise[r, os_ * (N + cp) + cp + NW * m + j]
                Yj[j, r] = np.fft.fft(v)                                 # element k' = g + 16 u in lane (r, g), register u
        want_spec = np.fft.fft(sigma * noise[:, os_ * (N + cp) + cp:(os_ + 1) * (N + cp)], axis=1)
        seen = np.zeros(N, int)
        for jw in range(NW):
            C = np.zeros((64, 16), complex)                              # [lane][register]: the noise spectrum
            B = np.zeros((64, 16), complex)                              # the lane's symbols
            A = np.zeros(64, complex)
            bins = np.zeros((16, 16), int)                               # [g][register] -> bin
            for ln in range(64):
                r, g = ln >> 4, ln & 15                                  # (= (a, g) for the B operand)
                A[ln] = H[ln & 3, ln >> 4]
                for uu in range(UU):
                    kp = g + 16 * (UU * jw + uu)
                    spec = _last_stage([Yj[jj, r, kp] for jj in range(NW)], NW, kp)
                    for q in range(NW):
                        reg, k = q + NW * uu, kp + 256 * q
                        C[ln, reg] = spec[q]
                        bins[g, reg] = k
                        label = lab[ln, 16 * jw + reg]
                        d = k ^ (N // 2)                                 # full band: data subcarrier d rides bin d ^ (N / 2)
                        assert label == idx[os_ * per_sym + 4 * d + r], (NW, jw, ln, reg)   # the symbol of THAT bin, stream a = r
                        B[ln, reg] = txtab[label]
            for b in range(4):                                           # D_b[i][j] = C_b[i][j] + sum_k A_b[i][k] B_b[k][j]
                for i in range(4):
                    for jj in range(4):
                        lane_d = 4 * b + jj + 16 * i
                        for reg in range(16):
                            acc = C[lane_d, reg] + sum(A[4 * b + i + 16 * k] * B[4 * b + jj + 16 * k, reg] for k in range(4))
                            k_bin = bins[lane_d & 15, reg]
                            assert abs(C[lane_d, reg] - want_spec[i, k_bin]) < 1e-9
                            Y[i, os_, k_bin ^ (N // 2)] = acc * rx_scale
                            seen[k_bin] += i == 0
        assert np.all(seen == 1)                                         # every bin by exactly one (wavefront, lane, register)
    want = np.asarray(out["Y"]).reshape(4, n_sym, N)
    assert np.max(np.abs(Y - want)) < 1e-12, np.max(np.abs(Y - want))
    # and the estimates: the oracle's G on that Y
    est = (out["G"] @ Y.reshape(4, -1)).reshape(-1, order="F")
    assert np.max(np.abs(est - out["est"])) < 1e-11
