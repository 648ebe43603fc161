"""GPU: the headline complex128 kernel (csrc/pipeline_mimo_pw.hip, default form, ownership by lane row) with the exchange between the
wavefronts in complex halves (template parameter XCH): the partial spectra cross LDS as 16-byte complex values in
two phases, each lane refilling the slots it has just read, so barrier B3 is not issued (and, in builds with MCLE_PW_LATE_B5 only,
barrier B5 stands in front of the symbol's first store into the planes instead of at the top of the symbol: measured slower, not
in the default build).  Only where a value lies in LDS and when a wavefront waits has changed: per-realization symbol and bit error counts must stay the oracle chain's (oracle/chains.py::chain_mimo_ofdm)
under common random numbers.  The index arithmetic itself is replayed on the CPU in tests/test_pw_exchange_layout.py.

The cases, depths and ranges are those of tests/test_gpu_pw_ahead.py (its oracle is computed once and shared): 512 / 1024 / 2048
points with 64 / 32 / 16 realizations, MMSE with the min-distance search and ZF with the slicer, 64-QAM at 25 dB and QPSK at 5 dB,
one symbol with prefix 16 and three symbols with prefix 0 (three symbols cross barrier B5 twice, so the refilled slots of one
symbol meet the transposition of the next), 256-QAM once at 1024.  The exchange in complex halves is the
default at 1024 and 2048 points; at 512 the default keeps the re / im planes (it was not faster there in every run), so every
size also runs f64_threads = 268, tag suffix "/h": the exchange in complex halves asked for.  f64_threads = 267, tag suffix "/x",
is the exchange by re / im planes with B3: the witness, whose counts must equal the default's and those of 268.  The
two-wavefront register bound (262 at 512, 264 at 1024) is another instantiation of the same loop.  Later passes of the persistent
loop: 32 n_cu + 7 realizations at 1024 points whole against pieces of 251.  The kernel tag is asserted in every case."""
import numpy as np
import pytest

from test_gpu_pw_ahead import CASES, LARGEST_TABLE, TWO, _check, _oracle, _run, _set, _tag

pytestmark = pytest.mark.gpu
WITNESS = 267                               # f64_threads: ownership by lane row, exchange by re / im planes (B3), tag suffix "/x"
HALVES = 268                                # f64_threads: the exchange in complex halves at every size, tag suffix "/h"


@pytest.mark.parametrize("fft", [512, 1024, 2048])
@pytest.mark.parametrize("case", range(4))
def test_counts_equal_the_oracle(engine, case, fft):
    _check(engine, case, fft)


@pytest.mark.parametrize("fft", [512, 1024, 2048])
@pytest.mark.parametrize("case", range(4))
def test_counts_of_the_complex_halves_equal_the_oracle(engine, case, fft):
    _check(engine, case, fft, HALVES, "/h")


def test_largest_table(engine):
    _check(engine, LARGEST_TABLE, 1024)
    _check(engine, LARGEST_TABLE, 1024, HALVES, "/h")


@pytest.mark.parametrize("fft,case", [(512, 1), (1024, 0), (1024, 2)])
def test_two_wavefront_bound(engine, fft, case):
    _check(engine, case, fft, TWO[fft], "/w2")


@pytest.mark.parametrize("fft,case", [(512, 2), (512, 1), (1024, 1), (1024, 0), (2048, 0), (2048, 2)])
def test_plane_exchange_witness_counts_equal_the_defaults(engine, fft, case):
    se_w, be_w = _check(engine, case, fft, WITNESS, "/x")
    se_d, be_d = _check(engine, case, fft)
    se_h, be_h = _check(engine, case, fft, HALVES, "/h")
    assert np.array_equal(se_w, se_d) and np.array_equal(be_w, be_d)
    assert np.array_equal(se_w, se_h) and np.array_equal(be_w, be_h)


def test_later_passes_equal_the_range_in_pieces(engine):
    """32 n_cu + 7 realizations at 1024 points, three symbols each: every workgroup takes ten or eleven realizations in turn and
    crosses B5 three times per realization, the first of them behind the previous realization's decode.  The same range in pieces of 251 (every workgroup's first pass only) must give the same counts, the witness
    the same again, and both ends of the range the oracle's."""
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
    _, se_w, be_w, tag_w = _run(engine, kw, fft, first, n, WITNESS)
    assert tag_w == _tag(fft, "/x")
    print("%d realizations: symbol errors %d whole / %d in pieces / %d witness, realizations that differ %d / %d" %
          (n, int(se.sum()), int(se_p.sum()), int(se_w.sum()), int(np.count_nonzero(se != se_p)), int(np.count_nonzero(se != se_w))))
    assert np.array_equal(se, se_p) and np.array_equal(be, be_p)
    assert np.array_equal(se, se_w) and np.array_equal(be, be_w)
    assert res["n_realizations"] == n and res["sym_errors"] == int(se_p.sum()) and res["bit_errors"] == int(be_p.sum())
    for lo in (0, n - edge):
        want_se, want_be = _oracle(case, fft, first + lo, edge)
        assert np.array_equal(se[lo:lo + edge], want_se) and np.array_equal(be[lo:lo + edge], want_be)
