"""Config 4 (mcle_run_mimo_ofdm): every kernel-selection edge walked on BOTH of its sides, in both arithmetics, with the kernel that
served each call named (Engine.last_kernel(), grammar at mcle_ctx_last_kernel in include/mcle.h) and its per-realization counts
against the oracle chain (oracle/chains.py::chain_mimo_ofdm) under the same Philox keying.

The selection is a tree (csrc/c4_select.hpp::c4_select, called by csrc/pipelines.hip::mcle_run_mimo_ofdm):
  complex64 with f32_mfma = 1 (and no_mfma = 0) at (1024, 4 x 4)                      -> mimo_ofdm_mfma v<variant>
  Nt = Nr in {2, 4} with f64_generic = 1, or complex64 with no_mfma = 1               -> mimo_ofdm_generic<N,NA> (64 .. 2048)
  (256, 2 x 2): f64_threads in {0, 260, 262} inside the wave envelope                 -> mimo_ofdm_fw<2>, else the generic kernel
  (256, 4 x 4): the same                                                              -> mimo_ofdm_fw<4>, else the planar kernel
  complex128 (512 / 2048, 4 x 4): f64_threads in {0, 260, 262, 265 .. 268} inside the envelope -> mimo_ofdm_pw<2 / 8>, else planar
  complex128 (1024, 4 x 4): {0, 263, 264, 265 .. 268} -> mimo_ofdm_pw<4>; {0, 260, 262} inside the quarter-wave envelope -> mimo_ofdm_qw;
                            258 / 256 / 512 / 257 / anything else -> five planar forms (complex64: 256 / 512 / 259 / 257 / else)
  every 1 <= Nt <= Nr <= 4 with Nr >= 2 at 256 .. 2048                                -> the planar geometry table
  Nt = Nr in {2, 4} at 64 / 128 (and what fell through above)                         -> the generic kernel;  anything else: refused.
The wave envelope: full band, even cyclic prefix, decisions by the slicer or a certificate (square QAM, one point per quadrant, four
points on the axes); the quarter-wave kernel has no on-axis certificate.  demod_nocert = 1 takes the certificates away, so
min-distance calls leave the wave kernels.

c4_tag() below replays that tree on the host as an INDEPENDENT statement of it (it never calls the library, and
tests/test_c4_select_cpu.py holds the C++ selection against it over the whole cross product); every row of ROWS names the
tag it expects, a CPU test proves that the rows cover every tag the replay can produce over the whole cross product of shapes,
arithmetics and options and that every row agrees with the replay, and one GPU walker per row asserts the tag, the counts against the
oracle (complex128 exact; complex64 by the criteria of test_gpu_planar_f32.py::_close), and the counts bit-identical under splits of
the range.  test_later_passes then runs, for every distinct tag, a range long enough that some workgroup handles more than one unit
of its persistent loop, against the same range in pieces that leave every workgroup one unit."""
import itertools

import numpy as np
import pytest

from oracle import chains, modem as omodem
from pyphysim_amd import _lib

gpu = pytest.mark.gpu
SEED = 27182818
# COUNT: not a multiple of 4 (nor of a workgroup's realizations).  The oracle costs 26 ms per realization at (2048, 4 x 4) and 2 - 6 ms
# below 1024 points (measured on the CPU): ~300 rows x 9 realizations stay under a minute, so the 2048-point rows keep COUNT = 9 too.
FIRST, COUNT, SPLIT = (1 << 33) + 1237, 9, 4
SKIPPED = 0xFFFFFFFF                                  # a skipped realization's entry in the per-realization arrays
REFUSED = "refused"
SIZES = (64, 128, 256, 512, 1024, 2048)
PAIRS = tuple((nt, nr) for nr in range(1, 5) for nt in range(1, nr + 1))             # the Nt <= Nr <= 4 triangle: 10 pairs
THREADS = (0, 256, 257, 258, 259, 260, 261, 262, 263, 264, 265, 266, 267, 268, 512, 1024)      # every value mcle_ctx_set_option accepts
COUNTERS = ("sym_errors", "sym_errors_sq", "bit_errors", "bit_errors_sq", "n_realizations", "n_skipped")

# ---- link cases: (constellation, SNR, prefix, band, demodulator).  "used": None = full band, an int = that many FEWER subcarriers,
# a float = that fraction of the band.  Every case has noise and counts errors (checked per row from the oracle alone) ----
LINKS = {
    "in": dict(mod="qam", M=64, snr_db=25.0),                                          # inside: QAM certificate, prefix 16, full band
    "slicer": dict(mod="qam", M=64, snr_db=25.0, method="slicer"),                     # inside: the slicer
    "cp0": dict(mod="qam", M=16, snr_db=18.0, cp=0),                                   # inside: no prefix
    "cp15": dict(mod="qam", M=16, snr_db=18.0, cp=15),                                 # OUTSIDE: odd prefix
    "band": dict(mod="qam", M=16, snr_db=18.0, used=2, n_sym=2),                       # OUTSIDE: two subcarriers short of the band
    "psk8": dict(mod="psk", M=8, snr_db=13.0, n_sym=2),                                # OUTSIDE: no certificate for 8-PSK
    "nocert": dict(mod="qam", M=64, snr_db=25.0, nocert=1),                            # OUTSIDE: the certificate switched off
    "psk4": dict(mod="psk", M=4, snr_db=8.0, cp=18),                                   # inside (on-axis certificate) -- but not for qw
    "qpsk": dict(mod="qpsk", M=4, snr_db=8.0, cp=32, mmse=False),                      # inside: quadrant certificate, ZF
    "low": dict(mod="qam", M=64, snr_db=12.0),                                         # one transmit antenna: diversity Nr, so 12 dB
    "low15": dict(mod="qam", M=64, snr_db=12.0, cp=15),
    # tests/test_gpu_f64_kernel.py::SHAPE_CASES, in its order
    "s0": dict(mod="qam", M=64, snr_db=25.0),
    "s1": dict(mod="qam", M=16, snr_db=17.0, used=0.6, n_sym=2, cp=7, mmse=False),
    "s2": dict(mod="psk", M=8, snr_db=13.0, n_sym=2, cp=33),
}
SHAPE_LINKS = ("s0", "s1", "s2")
# The rows that count NOTHING (the oracle's nine realizations have no symbol error): one transmit antenna under a SHAPE_CASES link of
# 17 / 25 dB -- receive diversity Nr makes these high-SNR rows.  Their kernels count errors in the "low" rows of the same shapes.
QUIET = {((256, 1, 2), "s1"), ((256, 1, 3), "s0"), ((256, 1, 4), "s0"), ((1024, 1, 3), "s1"), ((1024, 1, 4), "s1"),
         ((2048, 1, 3), "s0"), ((2048, 1, 4), "s0")}


def _cp(link):
    return link.get("cp", 16)


def _used(link, fft):
    u = link.get("used")
    if u is None:
        return fft
    return fft - u if isinstance(u, int) else 2 * int(u * fft / 2)


# ---- the tags (include/mcle.h, at mcle_ctx_last_kernel) ----
def PL(n, nt, nr, dt, ah, w, v=0):
    return "mimo_ofdm_planar<%d,%d,%d> %s ah%d w%d v%d" % (n, nt, nr, dt, ah, w, v)


def FW(na, dt, w):
    return "mimo_ofdm_fw<%d> %s w%d" % (na, dt, w)


def PW(nw, form, two=False, sfx=""):
    return "mimo_ofdm_pw<%d>/%s%s%s" % (nw, form, "/w2" if two else "", sfx)


def QW(w):
    return "mimo_ofdm_qw w%d" % w


def MF(v):
    return "mimo_ofdm_mfma v%d" % v


def GE(n, na, dt):
    return "mimo_ofdm_generic<%d,%d> %s" % (n, na, dt)


# ---- host replay of the selection ----
DEC_GENERIC, DEC_SLICER, DEC_QAM, DEC_QUAD, DEC_AXIS4 = range(5)


def dec_kind(link):
    """walk_f64.hpp::walk_dec_kind (+ modem.hpp::modem_cert): the decision form a wave kernel compiles to; DEC_GENERIC = none."""
    if link.get("method") == "slicer":
        return DEC_SLICER                              # (check_pipe: the slicer needs kind QAM)
    if link.get("nocert"):
        return DEC_GENERIC
    if link["mod"] == "qam":
        return DEC_QAM                                 # modem_cert 1: square Gray QAM, 2 <= L <= 256
    if link["mod"] == "qpsk":
        return DEC_QUAD                                # modem_cert 2: one point per quadrant
    if link["mod"] == "psk" and link["M"] == 4:
        return DEC_AXIS4                               # not in modem_cert: walk_dec_kind's own on-axis form
    return DEC_GENERIC


def wave_envelope(link, fft):
    """The wave kernels (full-wave, part-wave): full band, even prefix, M <= 256, a decision form."""
    return _used(link, fft) == fft and _cp(link) % 2 == 0 and link["M"] <= 256 and dec_kind(link) != DEC_GENERIC


def qw_envelope(link, fft):
    """The quarter-wave kernel: as above, but only the slicer or a modem_cert certificate (no on-axis form)."""
    return _used(link, fft) == fft and _cp(link) % 2 == 0 and link["M"] <= 256 and dec_kind(link) in (DEC_SLICER, DEC_QAM, DEC_QUAD)


def planar_wps(dt, n, nt, nr, w64):
    """c4_select.hpp::planar_wps: complex64 takes two more wavefronts per SIMD at 256 points (not 4 x 4) and (512, Nr = 2)."""
    if dt == "f32" and w64 <= 3 and ((n == 256 and not (nt == 4 and nr == 4)) or (n == 512 and nr == 2)):
        return w64 + 2
    return w64


def _geom(dt, n, nt, nr, w2, w4):
    """The planar radix-4 geometry table: Nr = 2 / 4 two antennas per thread, Nr = 3 three (one group)."""
    if nr == 2:
        return PL(n, nt, nr, dt, 2, planar_wps(dt, n, nt, nr, w2))
    if nr == 3:
        return PL(n, nt, nr, dt, 3, planar_wps(dt, n, nt, nr, 2))
    if nr == 4:
        return PL(n, nt, nr, dt, 2, planar_wps(dt, n, nt, nr, w4))
    return None


def fw_tag(dt, na, thr):
    two = thr == 262
    return FW(na, dt, (3 if two else 2) if dt == "f32" else (2 if two else 3))


PW_SUFFIX = {266: "/a", 267: "/x", 268: "/h"}


def pw_tag(n, thr):
    td, two = thr == 265, thr in (262, 264)
    sfx = PW_SUFFIX.get(thr, "")                       # 266 / 267 / 268: the default form with another map or exchange, asked for by value
    if n == 2048:
        return PW(8, "time" if td else "freq", sfx=sfx)
    return PW(n // 256, "time") if td else PW(n // 256, "freq", two, sfx)


def planar_family(dt, n, nt, nr, link, thr):
    """The wave kernels at 4 x 4 and the planar family (c4_select_planar); None = no kernel of this shape here."""
    f64 = dt == "f64"
    if n == 256 and nt == 4 and nr == 4 and thr in (0, 260, 262) and wave_envelope(link, n):
        return fw_tag(dt, 4, thr)
    if n in (512, 2048) and nt == 4 and nr == 4 and f64 and thr in (0, 260, 262, 265, 266, 267, 268) and wave_envelope(link, n):
        return pw_tag(n, thr)
    if n == 1024 and nt == 4 and nr == 4:
        if f64:
            if thr in (0, 263, 264, 265, 266, 267, 268) and wave_envelope(link, n):
                return pw_tag(n, thr)
            if thr in (0, 260, 262) and qw_envelope(link, n):
                return QW(2 if thr == 262 else 3)
            if thr == 258:
                return PL(1024, 4, 4, dt, 4, 2, 28)
        if thr == 256:
            return PL(1024, 4, 4, dt, 4, 2)
        if thr == 512:
            return PL(1024, 4, 4, dt, 2, 4)
        if not f64:
            return PL(1024, 4, 4, dt, 4, 4, 12) if thr == 259 else PL(1024, 4, 4, dt, 4, 3, 4) if thr == 257 else PL(1024, 4, 4, dt, 4, 4, 4)
        return PL(1024, 4, 4, dt, 4, 2, 4) if thr == 257 else PL(1024, 4, 4, dt, 4, 2, 12)
    if n == 256:
        return None if (nt, nr) == (2, 2) else PL(256, 4, 4, dt, 2, 3) if (nt, nr) == (4, 4) else _geom(dt, n, nt, nr, 2, 3)
    if n == 512:
        return PL(512, 4, 4, dt, 2, 3) if (nt, nr) == (4, 4) else _geom(dt, n, nt, nr, 3, 3)
    if n == 1024:
        if nr == 4 and thr == 0:
            return PL(1024, nt, 4, dt, 4, 2 if f64 else 4, 12 if f64 else 4)
        return _geom(dt, n, nt, nr, 3, 4)
    if n == 2048:
        if nr == 4 and (thr == 512 or (thr != 1024 and (nt == 4 or not f64))):
            return PL(2048, nt, 4, dt, 4, 2)
        return PL(2048, 4, 4, dt, 2, 4) if (nt, nr) == (4, 4) else _geom(dt, n, nt, nr, 4, 4)
    return None


def generic_lds(dt, n, na, used, G):
    """run_mimo_impl's dynamic LDS (bytes); G = the candidate grid's side, 0 .. 32."""
    cx = 16 if dt == "f64" else 8
    return (na * n + n + 256 + 2 * na * na) * cx + 256 * 16 + 16 * 4 + G * G * 8 + na * used


def c4_tag(n, nt, nr, dt, link, thr=0, f64_generic=0, no_mfma=0, f32_mfma=0, mfma_variant=0):
    """mcle_run_mimo_ofdm's selection: the tag of the kernel that serves the call, or REFUSED (a host-side MCLE_REQUIRE in front of
    every launch)."""
    f32 = dt == "f32"
    if f32 and f32_mfma and not no_mfma and (n, nt, nr) == (1024, 4, 4):
        return MF(mfma_variant or 36)
    has = nt == nr and nt in (2, 4)
    want_generic = has and bool(f64_generic or (f32 and no_mfma))
    small = (n, nt, nr) == (256, 2, 2)                 # generic_is_faster: the planar family has no kernel of this shape
    if small and not want_generic and thr in (0, 260, 262) and wave_envelope(link, n):
        return fw_tag(dt, 2, thr)
    if not want_generic and not small:
        tag = planar_family(dt, n, nt, nr, link, thr)
        if tag is not None:
            return tag
    if not has:
        return REFUSED
    lo, hi = generic_lds(dt, n, nt, _used(link, n), 0), generic_lds(dt, n, nt, _used(link, n), 32)
    assert (lo <= 160 * 1024) == (hi <= 160 * 1024), (n, nt, dt)          # the grid's size never decides
    return GE(n, nt, dt) if hi <= 160 * 1024 else REFUSED


# ---- the rows: (shape, arithmetic, link case, options, expected tag) ----
ROWS = []


def row(n, nt, nr, dt, link, tag, **opts):
    ROWS.append(((n, nt, nr), dt, link, opts, tag))


BOTH = ("f64", "f32")
# size: 64 and 128 points have the generic kernel only (2 x 2, 4 x 4); 3 x 3 and 2 x 4 are refused there; 256 is the first planar size
for n_, dt_ in itertools.product((64, 128), BOTH):
    for na_ in (2, 4):
        row(n_, na_, na_, dt_, "cp0", GE(n_, na_, dt_))
for dt_ in BOTH:
    row(128, 3, 3, dt_, "cp0", REFUSED)
    row(128, 2, 4, dt_, "cp0", REFUSED)
    row(256, 3, 3, dt_, "cp0", PL(256, 3, 3, dt_, 3, 2 if dt_ == "f64" else 4))
    row(256, 2, 4, dt_, "cp0", PL(256, 2, 4, dt_, 2, 3 if dt_ == "f64" else 5))

# 256 points, 2 x 2 and 4 x 4: the full-wave kernel inside its envelope; outside 4 x 4 -> planar, 2 x 2 -> GENERIC (the planar family
# has no (256, 2 x 2) kernel: f64_threads = 261 there is the generic kernel, whatever earlier documents said)
for dt_, na_ in itertools.product(BOTH, (2, 4)):
    far = GE(256, 2, dt_) if na_ == 2 else PL(256, 4, 4, dt_, 2, 3)
    w_def, w_alt = (3, 2) if dt_ == "f64" else (2, 3)
    row(256, na_, na_, dt_, "in", FW(na_, dt_, w_def))
    row(256, na_, na_, dt_, "in", FW(na_, dt_, w_def), f64_threads=260)
    row(256, na_, na_, dt_, "in", FW(na_, dt_, w_alt), f64_threads=262)
    row(256, na_, na_, dt_, "in", far, f64_threads=261)
    for lk_ in ("cp0", "slicer", "psk4", "qpsk"):                     # prefix 0 / slicer / on-axis / quadrant certificate: inside
        row(256, na_, na_, dt_, lk_, FW(na_, dt_, w_def))
    for lk_ in ("cp15", "band", "psk8", "nocert"):                    # prefix 15 / 254 subcarriers / 8-PSK / demod_nocert = 1: outside
        row(256, na_, na_, dt_, lk_, far)
    if dt_ == "f32":
        row(256, na_, na_, dt_, "in", GE(256, na_, dt_), no_mfma=1)

# (512, 4 x 4) and (2048, 4 x 4)
for n_ in (512, 2048):
    nw_ = n_ // 256
    far = PL(512, 4, 4, "f64", 2, 3) if n_ == 512 else PL(2048, 4, 4, "f64", 4, 2)
    row(n_, 4, 4, "f64", "in", PW(nw_, "freq"))
    row(n_, 4, 4, "f64", "in", PW(nw_, "freq"), f64_threads=260)
    row(n_, 4, 4, "f64", "in", PW(nw_, "freq", two=n_ == 512), f64_threads=262)      # (2048: one register bound only)
    row(n_, 4, 4, "f64", "in", PW(nw_, "time"), f64_threads=265)
    row(n_, 4, 4, "f64", "in", far, f64_threads=261)
    row(n_, 4, 4, "f64", "in", far, f64_threads=264)                                 # (264 selects the part-wave kernel at 1024 only)
    row(n_, 4, 4, "f64", "in", far, f64_threads=512)
    for lk_ in ("cp0", "slicer", "psk4", "qpsk"):
        row(n_, 4, 4, "f64", lk_, PW(nw_, "freq"))
    for lk_ in ("cp15", "band", "psk8", "nocert"):
        row(n_, 4, 4, "f64", lk_, far)
    far32 = PL(512, 4, 4, "f32", 2, 3) if n_ == 512 else PL(2048, 4, 4, "f32", 4, 2)
    for thr_ in (0, 260, 261, 265, 512):                               # complex64: planar whatever f64_threads says ...
        row(n_, 4, 4, "f32", "in", far32, f64_threads=thr_)
row(2048, 4, 4, "f64", "in", PL(2048, 4, 4, "f64", 2, 4), f64_threads=1024)
row(2048, 4, 4, "f32", "in", PL(2048, 4, 4, "f32", 2, 4), f64_threads=1024)          # ... except 1024 at 2048
row(512, 4, 4, "f64", "in", PL(512, 4, 4, "f64", 2, 3), f64_threads=1024)

# (1024, 4 x 4)
P16 = PL(1024, 4, 4, "f64", 4, 2, 12)                                   # planar, fused radix-16: where complex128 lands outside every envelope
for thr_, tag_ in ((0, PW(4, "freq")), (263, PW(4, "freq")), (264, PW(4, "freq", True)), (265, PW(4, "time")), (260, QW(3)), (262, QW(2)),
                   (261, P16), (259, P16), (257, PL(1024, 4, 4, "f64", 4, 2, 4)), (258, PL(1024, 4, 4, "f64", 4, 2, 28)),
                   (256, PL(1024, 4, 4, "f64", 4, 2)), (512, PL(1024, 4, 4, "f64", 2, 4))):
    row(1024, 4, 4, "f64", "in", tag_, f64_threads=thr_)
for lk_ in ("cp0", "slicer", "psk4", "qpsk"):
    row(1024, 4, 4, "f64", lk_, PW(4, "freq"))
for lk_ in ("cp15", "band", "psk8", "nocert"):                         # default outside: through part-wave AND quarter-wave to planar
    row(1024, 4, 4, "f64", lk_, P16)
    row(1024, 4, 4, "f64", lk_, P16, f64_threads=260)
for lk_ in ("cp0", "slicer", "qpsk"):
    row(1024, 4, 4, "f64", lk_, QW(3), f64_threads=260)
row(1024, 4, 4, "f64", "psk4", P16, f64_threads=260)                   # the quarter-wave kernel has no on-axis certificate
row(1024, 4, 4, "f64", "psk4", PW(4, "freq", True), f64_threads=264)
for thr_, tag_ in ((0, PL(1024, 4, 4, "f32", 4, 4, 4)), (259, PL(1024, 4, 4, "f32", 4, 4, 12)), (257, PL(1024, 4, 4, "f32", 4, 3, 4)),
                   (256, PL(1024, 4, 4, "f32", 4, 2)), (512, PL(1024, 4, 4, "f32", 2, 4)), (261, PL(1024, 4, 4, "f32", 4, 4, 4)),
                   (265, PL(1024, 4, 4, "f32", 4, 4, 4))):
    row(1024, 4, 4, "f32", "in", tag_, f64_threads=thr_)
for var_ in (0, 36, 32, 30, 21):
    row(1024, 4, 4, "f32", "in", MF(var_ or 36), f32_mfma=1, mfma_variant=var_)
row(1024, 4, 4, "f32", "cp15", MF(36), f32_mfma=1)                      # (the matrix-core kernel has no prefix / band condition)
row(1024, 4, 4, "f32", "in", GE(1024, 4, "f32"), f32_mfma=1, no_mfma=1)
row(1024, 4, 4, "f32", "in", GE(1024, 4, "f32"), no_mfma=1)
row(1024, 4, 4, "f64", "in", PW(4, "freq"), no_mfma=1)                  # (no_mfma moves complex64 only)
row(512, 4, 4, "f32", "in", PL(512, 4, 4, "f32", 2, 3), f32_mfma=1)     # f32_mfma outside (1024, 4 x 4): the planar family

# (1024, Nt < 4, Nr = 4): f64_threads = 0 -> the radix-16 form, any other value -> the radix-4 form
for dt_, nt_ in itertools.product(BOTH, (1, 2, 3)):
    row(1024, nt_, 4, dt_, "low", PL(1024, nt_, 4, dt_, 4, 2 if dt_ == "f64" else 4, 12 if dt_ == "f64" else 4))
    for thr_ in (261, 512):
        row(1024, nt_, 4, dt_, "low", PL(1024, nt_, 4, dt_, 2, 4), f64_threads=thr_)

# (2048, Nt <= 4, Nr = 4): complex128 4 x 4 four antennas per thread, Nt < 4 the 1 024-thread form; complex64 four antennas at every
# Nt; 512 / 1024 force either in both arithmetics (cp 15 keeps 4 x 4 complex128 off the part-wave kernel)
for dt_, nt_ in itertools.product(BOTH, (1, 2, 3, 4)):
    four = PL(2048, nt_, 4, dt_, 4, 2)
    row(2048, nt_, 4, dt_, "low15", four if (nt_ == 4 or dt_ == "f32") else PL(2048, nt_, 4, dt_, 2, 4))
    row(2048, nt_, 4, dt_, "low15", four, f64_threads=512)
    row(2048, nt_, 4, dt_, "low15", PL(2048, nt_, 4, dt_, 2, 4), f64_threads=1024)

# the complete Nt <= Nr <= 4 triangle at 256 .. 2048, both arithmetics, default options: 80 rows GENERATED from the replay, the link
# case round-robin over test_gpu_f64_kernel.py::SHAPE_CASES.  (1 x 1 is in the triangle and not in the geometry table: its eight rows
# pin the host-side refusal.)
TRIANGLE = []
for i_, (n_, (nt_, nr_), dt_) in enumerate(itertools.product((256, 512, 1024, 2048), PAIRS, BOTH)):
    lk_ = SHAPE_LINKS[(i_ // 2 + i_ // 20) % 3]            # (both arithmetics of a shape share the case, i.e. the oracle batch)
    TRIANGLE.append(len(ROWS))
    row(n_, nt_, nr_, dt_, lk_, c4_tag(n_, nt_, nr_, dt_, LINKS[lk_]))
assert len(TRIANGLE) == 80
# one transmit antenna at a low SNR, every size and arithmetic: the rows in which the Nt = 1 kernels count errors (see QUIET)
for n_, nr_, dt_ in itertools.product((256, 512, 1024, 2048), (2, 3, 4), BOTH):
    row(n_, 1, nr_, dt_, "low", c4_tag(n_, 1, nr_, dt_, LINKS["low"]))

# f64_generic = 1: the generic kernel where it exists (2 x 2 / 4 x 4 at 64 .. 2048) -- inside the wave kernels' envelope too -- and the
# planar family where it does not (Nt < Nr, 3 x 3): the option selects a kernel, it does not shrink the envelope.  (2048, 4 x 4)
# complex128 needs 168 KiB of LDS: run_mimo_impl's MCLE_REQUIRE refuses it on the host, before its launch.
for n_, na_, dt_ in itertools.product(SIZES, (2, 4), BOTH):
    row(n_, na_, na_, dt_, "in", REFUSED if (n_, na_, dt_) == (2048, 4, "f64") else GE(n_, na_, dt_), f64_generic=1)
for dt_ in BOTH:
    row(256, 1, 2, dt_, "in", PL(256, 1, 2, dt_, 2, 2 if dt_ == "f64" else 4), f64_generic=1)
    row(512, 2, 4, dt_, "in", PL(512, 2, 4, dt_, 2, 3), f64_generic=1)
    row(1024, 3, 3, dt_, "in", PL(1024, 3, 3, dt_, 3, 2), f64_generic=1)
    row(128, 2, 4, dt_, "in", REFUSED, f64_generic=1)
# no_mfma = 1 in complex64 at a shape without a generic kernel: the planar family
row(1024, 2, 4, "f32", "in", PL(1024, 2, 4, "f32", 4, 4, 4), no_mfma=1)
row(512, 3, 3, "f32", "in", PL(512, 3, 3, "f32", 3, 2), no_mfma=1)

# f64_threads = 266 / 267 / 268 (appended: the rows above keep their numbers): the part-wave kernel's default form with the ownership
# map of rounds 6 - 9 ("/a"), with the exchange by re / im planes ("/x") or in complex halves ("/h") asked for, at all three sizes;
# outside the envelope the planar kernel the default lands on; complex64 has no part-wave kernel
for thr_, n_ in itertools.product((266, 267, 268), (512, 1024, 2048)):
    row(n_, 4, 4, "f64", "in", PW(n_ // 256, "freq", sfx=PW_SUFFIX[thr_]), f64_threads=thr_)
    row(n_, 4, 4, "f64", "cp15", {512: PL(512, 4, 4, "f64", 2, 3), 1024: P16, 2048: PL(2048, 4, 4, "f64", 4, 2)}[n_], f64_threads=thr_)
    row(n_, 4, 4, "f32", "in", {512: PL(512, 4, 4, "f32", 2, 3), 1024: PL(1024, 4, 4, "f32", 4, 4, 4), 2048: PL(2048, 4, 4, "f32", 4, 2)}[n_],
        f64_threads=thr_)


def _row_id(i):
    (n, nt, nr), dt, lk, opts, _ = ROWS[i]
    return "%d-%dx%dx%d-%s-%s%s" % (i, n, nt, nr, dt, lk, "".join("-%s%d" % (k.replace("f64_", "").replace("mfma_", "")[:7], v)
                                                                    for k, v in sorted(opts.items())))


def _replay_row(r):
    (n, nt, nr), dt, lk, opts, _ = r
    return c4_tag(n, nt, nr, dt, LINKS[lk], thr=opts.get("f64_threads", 0), f64_generic=opts.get("f64_generic", 0),
                  no_mfma=opts.get("no_mfma", 0), f32_mfma=opts.get("f32_mfma", 0), mfma_variant=opts.get("mfma_variant", 0))


def all_replay_tags():
    """Every tag the replay can produce: 6 sizes x 10 antenna pairs x 2 arithmetics x every f64_threads value x f64_generic, no_mfma,
    f32_mfma in {0, 1} (x the matrix-core variants) x inside / outside the envelope (and the on-axis case the quarter-wave kernel
    declines)."""
    tags = set()
    for n, (nt, nr), dt, thr, gen, nom, mf, lk in itertools.product(SIZES, PAIRS, BOTH, THREADS, (0, 1), (0, 1), (0, 1),
                                                                    ("in", "cp15", "psk4")):
        for var in ((0, 36, 32, 30, 21) if mf else (0,)):
            tags.add(c4_tag(n, nt, nr, dt, LINKS[lk], thr, gen, nom, mf, var))
    tags.discard(REFUSED)
    return tags


ALL_TAGS = sorted(all_replay_tags())


# ---- CPU: the table is complete and agrees with the replay ----
def test_rows_cover_every_tag_of_the_replay_and_agree_with_it():
    for i, r in enumerate(ROWS):
        assert _replay_row(r) == r[4], (_row_id(i), _replay_row(r), r[4])
    row_tags = {r[4] for r in ROWS} - {REFUSED}
    print("replay tags %d, row tags %d, rows %d" % (len(ALL_TAGS), len(row_tags), len(ROWS)))
    assert set(ALL_TAGS) - row_tags == set(), sorted(set(ALL_TAGS) - row_tags)       # a new leaf without a row fails here
    assert row_tags - set(ALL_TAGS) == set(), sorted(row_tags - set(ALL_TAGS))
    assert all(len(t) < 48 for t in ALL_TAGS)                                        # mcle_ctx::last_kernel is 48 bytes
    # the triangle is whole: every pair at every planar size in both arithmetics
    assert {(ROWS[i][0], ROWS[i][1]) for i in TRIANGLE} == {((n, nt, nr), dt) for n in (256, 512, 1024, 2048) for nt, nr in PAIRS for dt in BOTH}
    # every tag has its own kernel: the planar family cannot name a (256, 2 x 2) kernel (removed: nothing reached it)
    assert not any(t.startswith("mimo_ofdm_planar<256,2,2>") for t in ALL_TAGS)


def test_refusals_of_the_replay_are_the_documented_ones():
    """Default options: below 256 points only the generic kernel's shapes (2 x 2, 4 x 4) run, from 256 points on every pair with
    Nr >= 2 (the geometry table has no 1 x 1: refused at every size, by the MCLE_REQUIRE in front of the generic kernels);
    f64_generic = 1 adds one refusal, the generic kernel's LDS at (2048, 4 x 4) in complex128."""
    for n, (nt, nr), dt in itertools.product(SIZES, PAIRS, BOTH):
        refused = c4_tag(n, nt, nr, dt, LINKS["in"]) == REFUSED
        assert refused == (nr == 1 or (n < 256 and not (nt == nr and nt in (2, 4)))), (n, nt, nr, dt)
        forced = c4_tag(n, nt, nr, dt, LINKS["in"], f64_generic=1) == REFUSED
        assert forced == (refused or (n, nt, nr, dt) == (2048, 4, 4, "f64")), (n, nt, nr, dt)


# ---- GPU ----
_ORACLE = {}


def _okw(shape, lk):
    n, nt, nr = shape
    link = LINKS[lk]
    return dict(mod=link["mod"], M=link["M"], nt=nt, nr=nr, fft_size=n, cp_size=_cp(link), num_used=_used(link, n),
                n_ofdm_sym=link.get("n_sym", 1), snr_db=link["snr_db"], mmse=link.get("mmse", True))


def _link_key(lk):
    link = LINKS[lk]
    return (link["mod"], link["M"], link["snr_db"], _cp(link), link.get("used"), link.get("n_sym", 1), link.get("mmse", True))


def _oracle(shape, lk, indices):
    """Per-realization counts of the oracle at these indices, cached per (shape, link): the option values of a shape share them."""
    okw = _okw(shape, lk)
    cache = _ORACLE.setdefault((shape, _link_key(lk)), {})
    for r in indices:
        if r not in cache:
            o = chains.chain_mimo_ofdm(chains.PhiloxRng(SEED, int(r)), **okw)
            cache[r] = (o["symbol_errors"], o["bit_errors"], o["num_symbols"], o["num_bits"])
    out = [cache[r] for r in indices]
    return (np.array([o[0] for o in out], dtype=np.int64), np.array([o[1] for o in out], dtype=np.int64), out[0][2], out[0][3])


def _set(engine, lk):
    link = LINKS[lk]
    engine.set_constellation(chains.constellation(link["mod"], link["M"]), _lib.CONST_QAM if link["mod"] == "qam" else _lib.CONST_GENERIC)


def _call(engine, shape, dt, lk, opts, first, count):
    """-> (counters, se, be, tag)"""
    n, nt, nr = shape
    link = LINKS[lk]
    nv = 1.0 / omodem.dB2Linear(link["snr_db"])
    method = _lib.DEMOD_QAM_SLICER if link.get("method") == "slicer" else _lib.DEMOD_MINDIST
    with engine.options(demod_nocert=link.get("nocert", 0), **opts):
        out = engine.run_mimo_ofdm(nt, nr, n, _cp(link), _used(link, n), link.get("n_sym", 1), nv, SEED, first, count,
                                   mmse=link.get("mmse", True), method=method, dtype=dt, per_realization=True)
        return out + (engine.last_kernel(),)


def _check(dt, res, se, be, want_se, want_be, nsym, nbits, what):
    """complex128: exact.  complex64: test_gpu_planar_f32.py::_close -- sums within 1e-4 n nsym + 2, <= 3 per realization, <= 1 skipped."""
    count = len(want_se)
    assert res["n_symbols"] == nsym and res["n_bits"] == nbits, what
    assert res["n_realizations"] + res["n_skipped"] == count, what
    ok = se != SKIPPED
    assert int(np.count_nonzero(~ok)) == res["n_skipped"], what
    s64, b64 = se.astype(np.int64), be.astype(np.int64)
    assert res["sym_errors"] == int(s64[ok].sum()) and res["bit_errors"] == int(b64[ok].sum()), what        # totals = sums of the arrays
    assert res["sym_errors_sq"] == int((s64[ok] ** 2).sum()) and res["bit_errors_sq"] == int((b64[ok] ** 2).sum()), what
    if dt == "f64":
        assert res["n_skipped"] == 0, what
        assert np.array_equal(s64, want_se) and np.array_equal(b64, want_be), (what, s64.tolist(), want_se.tolist())
    else:
        assert res["n_skipped"] <= 1, what
        n = int(ok.sum())
        assert abs(int(s64[ok].sum()) - int(want_se[ok].sum())) <= 1e-4 * n * nsym + 2, (what, s64.tolist(), want_se.tolist())
        assert abs(int(b64[ok].sum()) - int(want_be[ok].sum())) <= 1e-4 * n * nbits + 2, (what, b64.tolist(), want_be.tolist())
        assert np.max(np.abs(s64[ok] - want_se[ok])) <= 3, (what, s64.tolist(), want_se.tolist())


_WALKED, _SEEN = set(), set()


@gpu
@pytest.mark.parametrize("i", range(len(ROWS)), ids=_row_id)
def test_c4_edge(engine, i):
    shape, dt, lk, opts, want_tag = ROWS[i]
    _set(engine, lk)
    if want_tag == REFUSED:                     # host-side refusals only: the MCLE_REQUIREs of mcle_run_mimo_ofdm / run_mimo_impl, in front of every launch
        with pytest.raises(_lib.McleError):
            _call(engine, shape, dt, lk, opts, FIRST, COUNT)
        assert engine.last_kernel() == ""
        _WALKED.add(i)
        return
    want_se, want_be, nsym, nbits = _oracle(shape, lk, range(FIRST, FIRST + COUNT))
    assert (want_se.sum() > 0) == ((shape, lk) not in QUIET), (shape, lk)       # but for the rows listed in QUIET, equality is never 0 == 0
    res, se, be, tag = _call(engine, shape, dt, lk, opts, FIRST, COUNT)
    print("%s: %s, symbol errors %s (oracle %s)" % (_row_id(i), tag, se.astype(np.int64).tolist(), want_se.tolist()))
    assert tag != "" and tag == want_tag, (tag, want_tag)
    _check(dt, res, se, be, want_se, want_be, nsym, nbits, (_row_id(i), tag))
    splits = [SPLIT]
    if tag.startswith("mimo_ofdm_fw<2>"):       # two realizations per wavefront: an odd boundary, and a run of one realization
        splits.append(3)
        one = _call(engine, shape, dt, lk, opts, FIRST + 2, 1)
        assert one[3] == tag and np.array_equal(one[1], se[2:3]) and np.array_equal(one[2], be[2:3])
    for k in splits:
        a = _call(engine, shape, dt, lk, opts, FIRST, k)
        b = _call(engine, shape, dt, lk, opts, FIRST + k, COUNT - k)
        assert a[3] == tag and b[3] == tag
        assert np.array_equal(np.concatenate([a[1], b[1]]), se) and np.array_equal(np.concatenate([a[2], b[2]]), be), (k, tag)
        for key in COUNTERS:
            assert res[key] == a[0][key] + b[0][key], (key, k, tag)
    _WALKED.add(i)
    _SEEN.add(tag)


# ---- later passes of every persistent loop ----
def _prime_below(n):
    p = n - 1
    while any(p % d == 0 for d in range(2, int(p ** 0.5) + 1)):
        p -= 1
    return p


def _units(tag):
    """Realizations per unit of a launcher's persistent loop: the full-wave kernel hands a workgroup 4 wavefronts x RZ = 4 / NA
    realizations per unit (pipeline_mimo_fw.hip: oversubscribed_grid(ctx, resident, (n + 4 RZ - 1) / (4 RZ), ...)); every other
    launcher one realization (planar / pw / qw / mfma: oversubscribed_grid(ctx, resident, n, ...); generic: grid = min(count, cap))."""
    return 4 if tag.startswith("mimo_ofdm_fw<4>") else 8 if tag.startswith("mimo_ofdm_fw<2>") else 1


@gpu
@pytest.mark.parametrize("tag", ALL_TAGS)
def test_later_passes(engine, tag):
    """n = 32 n_cu r + 7 realizations, r = realizations per unit.  Why some workgroup then handles more than one unit:
      * a CU holds at most 32 wavefronts (8 per SIMD) and a workgroup is at least one, so every launcher's resident = n_cu x per_cu
        <= 32 n_cu; the call has units = ceil(n / r) > 32 n_cu >= resident;
      * oversubscribed_grid (pipe_common.hpp) returns min(units, resident x f), and f > 1 only while units >= resident x f x
        min_units with min_units >= 8: so either grid = resident < units (f = 1), or every workgroup has >= 8 units;
      * the generic kernel: grid = min(count, cap), cap = n_cu x per_cu with per_cu <= 8, so n > 8 n_cu >= cap = grid.
    The same range in calls of p realizations, p the largest prime below n_cu (251 of 256): fewer units than n_cu <= resident (<= cap),
    so grid = units and every workgroup handles exactly one -- the regime test_c4_edge checks against the oracle.  Same kernel, same
    arithmetic per realization: the concatenated arrays are bit-identical in both arithmetics, and the six counters add up."""
    i = next(j for j, r in enumerate(ROWS) if r[4] == tag and (r[0], r[2]) not in QUIET)
    shape, dt, lk, opts, _ = ROWS[i]
    _set(engine, lk)
    r = _units(tag)
    n = 32 * engine.n_cu * r + 7
    piece = _prime_below(engine.n_cu)
    first = FIRST + 100
    whole, se, be, got = _call(engine, shape, dt, lk, opts, first, n)
    assert got == tag
    assert whole["n_realizations"] + whole["n_skipped"] == n
    parts, tot = [], dict.fromkeys(COUNTERS, 0)
    for off in range(0, n, piece):
        p = _call(engine, shape, dt, lk, opts, first + off, min(piece, n - off))
        assert p[3] == tag
        parts.append(p)
        for key in COUNTERS:
            tot[key] += p[0][key]
    se_p, be_p = np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])
    bad = np.flatnonzero((se != se_p) | (be != be_p))
    print("%s: n %d, pieces of %d, symbol errors %d, realizations that differ %d %s" %
          (tag, n, piece, int(se[se != SKIPPED].astype(np.int64).sum()), len(bad), bad[:8].tolist()))
    assert len(bad) == 0, (tag, bad[:16].tolist(), se[bad[:16]].tolist(), se_p[bad[:16]].tolist())
    for key in COUNTERS:
        assert whole[key] == tot[key], (key, tag)
    # the oracle at the first, the last and ten indices spread evenly between them (second and later passes)
    at = np.unique(np.linspace(0, n - 1, 12).round().astype(np.int64))
    assert len(at) == 12 and at[0] == 0 and at[-1] == n - 1
    want_se, want_be, _, _ = _oracle(shape, lk, [first + int(a) for a in at])
    got_se, got_be = se[at].astype(np.int64), be[at].astype(np.int64)
    if dt == "f64":
        assert np.array_equal(got_se, want_se) and np.array_equal(got_be, want_be), (tag, at.tolist(), got_se.tolist(), want_se.tolist())
    else:
        ok = se[at] != SKIPPED
        assert np.count_nonzero(~ok) <= 1 and np.max(np.abs(got_se[ok] - want_se[ok])) <= 3, (tag, at.tolist(), got_se.tolist(), want_se.tolist())
    _SEEN.add(tag)


@gpu
def test_the_tags_seen_are_the_tags_enumerated(engine):
    """After the walkers above (this test runs last in the file): nothing ran that the replay does not know, and -- when the whole
    file ran -- every tag the replay enumerates was seen on the device."""
    print("tags seen on the device %d, tags the replay enumerates %d, rows walked %d of %d" % (len(_SEEN), len(ALL_TAGS), len(_WALKED), len(ROWS)))
    assert _SEEN <= set(ALL_TAGS), sorted(_SEEN - set(ALL_TAGS))
    if len(_WALKED) == len(ROWS):
        assert _SEEN == set(ALL_TAGS), sorted(set(ALL_TAGS) - _SEEN)
