"""GPU: the -ln u of the complex128 Box-Muller with its argument reduction in integer arithmetic (csrc/bm_f64.hpp: bm_neg_log_q, the
form csrc/philox.hpp draws every complex128 noise and channel sample with) against bm_neg_log, the form tests/test_bm_f64_cpu.py
pins to NumPy -- ON THE DEVICE.  The library is compiled with contraction on, so the device's expressions are not the host's, and
an identity shown by the host build (tests/test_bm_logq_cpu.py) is not yet one of the kernels.

1. tests/gpu_src/bm_probe.hip, compiled at test time with the library's flags against the library's headers, evaluates the old
   form and the new one -- from the global table, from an LDS copy read as 16-byte pairs (bm_tables_to_lds_pairs) and from an LDS
   copy read as doubles (bm_tables_to_lds) -- on chosen words in one launch and compares them as 64-bit words in the kernel: zero
   differences; its first 1e5 values equal the host build's.
2. Per-realization symbol and bit error counts of config 4's complex128 link (run_mimo_ofdm, part-wave kernel) equal the oracle
   chain's (oracle/chains.py::chain_mimo_ofdm) at 512 / 1024 / 2048 points: both LDS table copies (f64_threads = 266 is the
   kernel form that reads the non-pair copy), and later passes of the persistent loop.
Reference: util/misc.py:327-355 (randn_c), apps/mimo/simulate_mimo.py:68-142, mimo/mimo.py:609-660, modulators/ofdm.py:52-94."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import bm_words
from oracle import chains, modem as omodem
from pyphysim_amd import _lib

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 299792458


# ---- 1. the two forms on the device -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    out = tmp_path_factory.mktemp("bm_probe") / "libbm_probe.so"
    src = os.path.join(REPO, "tests", "gpu_src", "bm_probe.hip")
    csrc = os.path.join(REPO, "pyphysim_amd", "csrc")
    subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-gpu-rdc", "-fno-hip-fp32-correctly-rounded-divide-sqrt",
                    "-ffp-contract=fast", "-shared", "-I", csrc, "-I", os.path.join(REPO, "include"), src, "-o", str(out)], check=True)
    lib = ctypes.CDLL(str(out))
    P = ctypes.c_void_p
    lib.probe_bm_logq.argtypes = [P, ctypes.c_size_t, P, ctypes.c_size_t, P, P]
    lib.probe_bm_logq.restype = ctypes.c_int
    return lib


def _probe_words():
    """The words of tests/test_bm_logq_cpu.py with the two long ranges thinned to ~1e6 (every fourth word below 2^20 and of the
    complements, every eighth within 2^16 of a power of two), the edges whole (the two ends, the three words at every power of two,
    +-256 around every node boundary of every binade) and 1e6 random words -- in a fixed random order, so that the first 1e5 (the
    ones compared with the host build) are a sample of all of them."""
    low = bm_words.low_and_complement(2 ** 20)
    parts = [low[::4], low[:4096], low[2 ** 20:2 ** 20 + 4096], bm_words.around_powers_of_two(2 ** 16, step=8),
             bm_words.around_node_boundaries(256), bm_words.ends(), bm_words.random_words(1_000_000, 20262)]
    w = np.concatenate(parts)
    return np.ascontiguousarray(w[np.random.RandomState(7).permutation(w.size)])


def test_both_forms_agree_on_the_device(probe, engine, tmp_path):
    words = _probe_words()
    n, n_out = words.size, 100_000
    assert 2_500_000 < n < 4_000_000 and np.isin(np.array([0, 2 ** 32 - 1, 2 ** 31, 2 ** 31 - 1], dtype=np.uint32), words).all()
    out = np.full(n_out, np.nan)
    diffs = np.zeros(3, dtype=np.uint64)
    first = np.zeros(1, dtype=np.uint64)
    rc = probe.probe_bm_logq(words.ctypes.data, n, out.ctypes.data, n_out, diffs.ctypes.data, first.ctypes.data)
    assert rc == 0, rc
    print("%d words: differences global %d, LDS pairs %d, LDS doubles %d" % ((n,) + tuple(int(d) for d in diffs)))
    assert not diffs.any(), (diffs.tolist(), hex(int(words[min(int(first[0]), n - 1)])))
    assert int(first[0]) == n
    # ... and the device's values are the host build's (every operation of this function is a single rounding on both sides)
    host = bm_words.host_library(tmp_path)
    want_old, want_new = np.empty(n_out), np.empty(n_out)
    head = np.ascontiguousarray(words[:n_out])
    host.bm_neg_log_batch(head.ctypes.data, want_old.ctypes.data, n_out)
    host.bm_neg_log_q_batch(head.ctypes.data, want_new.ctypes.data, n_out)
    assert np.array_equal(out.view(np.uint64), want_new.view(np.uint64))
    assert np.array_equal(out.view(np.uint64), want_old.view(np.uint64))
    assert np.unique(out).size > 0.99 * np.unique(head).size       # values, not a constant (the ranges overlap: words repeat)


# ---- 2. link counts -----------------------------------------------------------------------------------------------------------
# every size runs 64-QAM at 25 dB and QPSK at 5 dB, MMSE with the min-distance search and ZF with the slicer, one symbol with prefix
# 16 and three with prefix 0 (the slicer is defined for square QAM only: QPSK under ZF takes the min-distance search)
CASES = [dict(mod="qam", M=64, snr_db=25.0, mmse=True, method=_lib.DEMOD_MINDIST, cp_size=16, n_ofdm_sym=1),
         dict(mod="qam", M=64, snr_db=25.0, mmse=False, method=_lib.DEMOD_QAM_SLICER, cp_size=0, n_ofdm_sym=3),
         dict(mod="qpsk", M=4, snr_db=5.0, mmse=True, method=_lib.DEMOD_MINDIST, cp_size=0, n_ofdm_sym=3),
         dict(mod="qpsk", M=4, snr_db=5.0, mmse=False, method=_lib.DEMOD_MINDIST, cp_size=16, n_ofdm_sym=1)]
DEPTH = {512: 64, 1024: 32, 2048: 16}
PLAIN = 266                                # f64_threads: the kernel form whose LDS tables are the non-pair copy (tag suffix "/a")
PLAIN_CASE = {512: 1, 1024: 0, 2048: 2}


def _set(engine, kw):
    engine.set_constellation(chains.constellation(kw["mod"], kw["M"]), _lib.CONST_QAM if kw["mod"] == "qam" else _lib.CONST_GENERIC)


def _run(engine, kw, fft, first, count, threads=0):
    nv = 1.0 / omodem.dB2Linear(kw["snr_db"])
    with engine.options(f64_threads=threads):
        out = engine.run_mimo_ofdm(4, 4, fft, kw["cp_size"], fft, kw["n_ofdm_sym"], nv, SEED, first, count, mmse=kw["mmse"],
                                   method=kw["method"], dtype="f64", per_realization=True)
        return out + (engine.last_kernel(),)


@functools.lru_cache(maxsize=None)
def _oracle(case, fft, first, count):
    """computed once per (case, size, range) and shared; the arrays are not written to"""
    kw = CASES[case]
    okw = dict(mod=kw["mod"], M=kw["M"], nt=4, nr=4, fft_size=fft, cp_size=kw["cp_size"], num_used=fft, n_ofdm_sym=kw["n_ofdm_sym"],
               snr_db=kw["snr_db"], mmse=kw["mmse"])
    want = [chains.chain_mimo_ofdm(chains.PhiloxRng(SEED, r), **okw) for r in range(first, first + count)]
    se, be = np.array([w["symbol_errors"] for w in want]), np.array([w["bit_errors"] for w in want])
    se.setflags(write=False)
    be.setflags(write=False)
    return se, be


def _tag(fft, plain=False):
    return "mimo_ofdm_pw<%d>/freq%s" % (fft // 256, "/a" if plain else "")


@pytest.mark.parametrize("fft", [512, 1024, 2048])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_link_counts_equal_the_oracle(engine, case, fft):
    kw = CASES[case]
    _set(engine, kw)
    first, count = (1 << 34) + 977 * case + fft, DEPTH[fft]
    want_se, want_be = _oracle(case, fft, first, count)
    assert want_se.sum() > 50                                        # the comparison has something to compare
    forms = [(0, False)] + ([(PLAIN, True)] if PLAIN_CASE[fft] == case else [])
    for threads, plain in forms:
        res, se, be, tag = _run(engine, kw, fft, first, count, threads)
        print("case %d fft %d f64_threads %d: %s, symbol errors %d (oracle %d), realizations that differ %d" %
              (case, fft, threads, tag, int(se.sum()), int(want_se.sum()), int(np.count_nonzero(se != want_se))))
        assert tag == _tag(fft, plain)
        assert np.array_equal(se, want_se), np.flatnonzero(se != want_se)[:5]
        assert np.array_equal(be, want_be), np.flatnonzero(be != want_be)[:5]
        assert res["n_realizations"] == count and res["n_skipped"] == 0
        assert res["sym_errors"] == int(want_se.sum()) and res["bit_errors"] == int(want_be.sum())


def test_later_passes_of_the_persistent_loop(engine):
    """32 n_cu + 7 realizations at 1024 points: every workgroup takes ten or eleven realizations in turn, each drawing its noise from
    the one LDS table copy made before the loop.  The same range in pieces of 251 (every workgroup's first pass only) must give the
    same counts, and both ends of the range the oracle's."""
    fft, case = 1024, 1                                              # three symbols, ZF: most realizations count errors
    kw = CASES[case]
    _set(engine, kw)
    first, n, piece, edge = 602214076, 32 * engine.n_cu + 7, 251, 8
    res, se, be, tag = _run(engine, kw, fft, first, n)
    assert tag == _tag(fft)
    assert se.shape == (n,) and np.count_nonzero(se) > n // 2          # (a few realizations of a good channel have none at 25 dB)
    se_p, be_p = np.empty_like(se), np.empty_like(be)
    for off in range(0, n, piece):
        k = min(piece, n - off)
        _, se_p[off:off + k], be_p[off:off + k], tag_p = _run(engine, kw, fft, first + off, k)
        assert tag_p == _tag(fft)
    print("%d realizations: symbol errors %d whole / %d in pieces, realizations that differ %d" %
          (n, int(se.sum()), int(se_p.sum()), int(np.count_nonzero(se != se_p))))
    assert np.array_equal(se, se_p) and np.array_equal(be, be_p)
    assert res["n_realizations"] == n and res["sym_errors"] == int(se_p.sum()) and res["bit_errors"] == int(be_p.sum())
    for lo in (0, n - edge):
        want_se, want_be = _oracle(case, fft, first + lo, edge)
        assert np.array_equal(se[lo:lo + edge], want_se) and np.array_equal(be[lo:lo + edge], want_be)
