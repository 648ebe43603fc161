"""GPU: the headline complex128 kernel (csrc/pipeline_mimo_pw.hip, default form, ownership by lane row) with its noise draw pipelined
one Philox block deep -- block cc + 1 fetched (Philox, row swaps, integer parts, the six table reads of its two samples) before
block cc is finished (cn_fetch_lds_pairs / cn_finish of csrc/philox.hpp).  Only the order of issue moved: per-realization symbol
and bit error counts must stay the oracle chain's (oracle/chains.py::chain_mimo_ofdm) under common random numbers.

Sixteen realizations exercise every lane row, every register and every wavefront of the maps; 512 / 1024 / 2048 points run
64 / 32 / 16 of them on: 64-QAM at 25 dB and QPSK at 5 dB, MMSE with the min-distance search and ZF with the slicer, one symbol
with prefix 16 and three symbols with prefix 0 (three symbols cross barrier B5 twice: the draw of a later symbol starts behind the
decode of the one before), and 256-QAM (the largest table) once at 1024.  The two-wavefront register bound (f64_threads = 262 at
512, 264 at 1024) is another instantiation of the same loop; the ownership map of rounds 6 - 9 (f64_threads = 266, tag "/a") keeps
the one-phase draw and is the untouched witness: its counts equal the default's.  Later passes of the persistent loop: 32 n_cu + 7
realizations at 1024 points whole against pieces of 251.
Reference: util/misc.py:327-355 (randn_c), apps/mimo/simulate_mimo.py:68-142, mimo/mimo.py:609-660, modulators/ofdm.py:52-94."""
import functools

import numpy as np
import pytest

from oracle import chains, modem as omodem
from pyphysim_amd import _lib

pytestmark = pytest.mark.gpu
SEED = 1618033988
# (the slicer is defined for square QAM only: QPSK under ZF takes the min-distance search)
CASES = [dict(mod="qam", M=64, snr_db=25.0, mmse=True, method=_lib.DEMOD_MINDIST, cp_size=16, n_ofdm_sym=1),
         dict(mod="qam", M=64, snr_db=25.0, mmse=False, method=_lib.DEMOD_QAM_SLICER, cp_size=0, n_ofdm_sym=3),
         dict(mod="qpsk", M=4, snr_db=5.0, mmse=True, method=_lib.DEMOD_MINDIST, cp_size=0, n_ofdm_sym=3),
         dict(mod="qpsk", M=4, snr_db=5.0, mmse=False, method=_lib.DEMOD_MINDIST, cp_size=16, n_ofdm_sym=1),
         dict(mod="qam", M=256, snr_db=25.0, mmse=True, method=_lib.DEMOD_MINDIST, cp_size=16, n_ofdm_sym=1)]
LARGEST_TABLE = 4                           # run once, at 1024 points
DEPTH = {512: 64, 1024: 32, 2048: 16}
TWO = {512: 262, 1024: 264}                 # f64_threads: the two-wavefronts-per-SIMD register bound, tag suffix "/w2"
OLD = 266                                   # f64_threads: the ownership map of rounds 6 - 9 (one-phase draw), tag suffix "/a"


def _set(engine, kw):
    engine.set_constellation(chains.constellation(kw["mod"], kw["M"]), _lib.CONST_QAM if kw["mod"] == "qam" else _lib.CONST_GENERIC)


def _run(engine, kw, fft, first, count, threads=0):
    nv = 1.0 / omodem.dB2Linear(kw["snr_db"])
    with engine.options(f64_threads=threads):
        out = engine.run_mimo_ofdm(4, 4, fft, kw["cp_size"], fft, kw["n_ofdm_sym"], nv, SEED, first, count, mmse=kw["mmse"],
                                   method=kw["method"], dtype="f64", per_realization=True)
        return out + (engine.last_kernel(),)


def _range(case, fft):
    return (1 << 36) + 7919 * case + fft, DEPTH[fft]


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


def _tag(fft, suffix=""):
    return "mimo_ofdm_pw<%d>/freq%s" % (fft // 256, suffix)


def _check(engine, case, fft, threads=0, suffix=""):
    kw = CASES[case]
    _set(engine, kw)
    first, count = _range(case, fft)
    want_se, want_be = _oracle(case, fft, first, count)
    assert want_se.sum() > 50                                        # the comparison has something to compare
    res, se, be, tag = _run(engine, kw, fft, first, count, threads)
    print("case %d fft %d f64_threads %d: %s, symbol errors %d (oracle %d), realizations that differ %d" %
          (case, fft, threads, tag, int(se.sum()), int(want_se.sum()), int(np.count_nonzero(se != want_se))))
    assert tag == _tag(fft, suffix)
    assert np.array_equal(se, want_se), np.flatnonzero(se != want_se)[:5]
    assert np.array_equal(be, want_be), np.flatnonzero(be != want_be)[:5]
    assert res["n_realizations"] == count and res["n_skipped"] == 0
    assert res["sym_errors"] == int(want_se.sum()) and res["bit_errors"] == int(want_be.sum())
    return se, be


@pytest.mark.parametrize("fft", [512, 1024, 2048])
@pytest.mark.parametrize("case", range(4))
def test_counts_equal_the_oracle(engine, case, fft):
    _check(engine, case, fft)


def test_largest_table(engine):
    _check(engine, LARGEST_TABLE, 1024)


@pytest.mark.parametrize("fft,case", [(512, 1), (1024, 0), (1024, 2)])
def test_two_wavefront_bound(engine, fft, case):
    _check(engine, case, fft, TWO[fft], "/w2")


@pytest.mark.parametrize("fft,case", [(512, 2), (1024, 1), (2048, 0)])
def test_one_phase_witness_counts_equal_the_defaults(engine, fft, case):
    se_w, be_w = _check(engine, case, fft, OLD, "/a")
    se_d, be_d = _check(engine, case, fft)
    assert np.array_equal(se_w, se_d) and np.array_equal(be_w, be_d)


def test_later_passes_equal_the_range_in_pieces(engine):
    """32 n_cu + 7 realizations at 1024 points: every workgroup takes ten or eleven realizations in turn, and every pass but the
    first starts its draw behind barrier B5 and the previous realization's decode.  The same range in pieces of 251 (every
    workgroup's first pass only) must give the same counts, and both ends of the range the oracle's."""
    fft, case = 1024, 1                                              # three symbols, ZF: most realizations count errors
    kw = CASES[case]
    _set(engine, kw)
    first, n, piece, edge = 662607015, 32 * engine.n_cu + 7, 251, 8
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
