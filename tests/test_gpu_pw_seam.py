"""GPU: the headline complex128 kernel (csrc/pipeline_mimo_pw.hip, default form, ownership by lane row) at the SEAM between two
realizations (round 22): the per-realization symbol and bit error totals of a wavefront are taken by six DPP adds and
one v_readlane_b32 (walk_wave_total of csrc/walk_f64.hpp) instead of twelve ds_bpermute_b32 round trips, lane 0 writes them into
s_part, and thread 0 accounts them one realization later (account_prev), forming the realization's output addresses there.  No
floating-point operation, draw, lane map, barrier or LDS layout moved: per-realization counts must stay the oracle chain's
(oracle/chains.py::chain_mimo_ofdm) under common random numbers.

The cases, depths, ranges and the shared oracle are those of tests/test_gpu_pw_exchange.py (= tests/test_gpu_pw_ahead.py): 512 /
1024 / 2048 points with 64 / 32 / 16 realizations, MMSE with the min-distance search and ZF with the slicer, 64-QAM at 25 dB and
QPSK at 5 dB, one symbol with prefix 16 and three with prefix 0.  One more case at 40 dB, where most realizations count ZERO errors:
a total that leaked from one realization (or one wavefront) into the next would show there at once.  The ownership map of rounds
6 - 9 (f64_threads = 266, tag suffix "/a") keeps wave_sum_u32 and its loop head as they were: the untouched witness, equal counts
at six (size, case) pairs.  32 n_cu + 7 realizations at 1024 points whole, in pieces of 251 and on the witness exercise
account_prev() for every it > 0 and for the last realization of a workgroup (accounted behind the loop).  The kernel tag is
asserted in every case."""
import functools

import numpy as np
import pytest

from oracle import chains
from pyphysim_amd import _lib
from test_gpu_pw_ahead import CASES, DEPTH, OLD, SEED, _check, _oracle, _run, _set, _tag

pytestmark = pytest.mark.gpu
QUIET = dict(mod="qam", M=64, snr_db=40.0, mmse=True, method=_lib.DEMOD_MINDIST, cp_size=16, n_ofdm_sym=1)


@pytest.mark.parametrize("fft", [512, 1024, 2048])
@pytest.mark.parametrize("case", range(4))
def test_counts_equal_the_oracle(engine, case, fft):
    _check(engine, case, fft)


@functools.lru_cache(maxsize=None)
def _quiet_oracle(fft, first, count):
    okw = dict(mod=QUIET["mod"], M=QUIET["M"], nt=4, nr=4, fft_size=fft, cp_size=QUIET["cp_size"], num_used=fft,
               n_ofdm_sym=QUIET["n_ofdm_sym"], snr_db=QUIET["snr_db"], mmse=QUIET["mmse"])
    want = [chains.chain_mimo_ofdm(chains.PhiloxRng(SEED, r), **okw) for r in range(first, first + count)]
    se, be = np.array([w["symbol_errors"] for w in want]), np.array([w["bit_errors"] for w in want])
    se.setflags(write=False)
    be.setflags(write=False)
    return se, be


def test_mostly_zero_counts_at_40_db(engine):
    """64-QAM at 40 dB: most realizations have no error at all and a few (an ill-conditioned channel) have many -- every zero
    must come out as a zero next to them."""
    fft = 1024
    first, count = (1 << 36) + 7919 * 5 + fft, DEPTH[fft]
    want_se, want_be = _quiet_oracle(fft, first, count)
    assert np.count_nonzero(want_se == 0) > count // 2 and want_se.sum() > 0           # mostly zeros, and something to compare
    _set(engine, QUIET)
    res, se, be, tag = _run(engine, QUIET, fft, first, count)
    print("40 dB fft %d: %s, realizations without an error %d of %d (oracle %d), symbol errors %d (oracle %d)" %
          (fft, tag, int(np.count_nonzero(se == 0)), count, int(np.count_nonzero(want_se == 0)), int(se.sum()), int(want_se.sum())))
    assert tag == _tag(fft)
    assert np.array_equal(se, want_se) and np.array_equal(be, want_be)
    assert res["n_realizations"] == count and res["n_skipped"] == 0
    assert res["sym_errors"] == int(want_se.sum()) and res["bit_errors"] == int(want_be.sum())


@pytest.mark.parametrize("fft,case", [(512, 2), (512, 1), (1024, 1), (1024, 0), (2048, 0), (2048, 2)])
def test_witness_counts_equal_the_defaults(engine, fft, case):
    se_w, be_w = _check(engine, case, fft, OLD, "/a")
    se_d, be_d = _check(engine, case, fft)
    assert np.array_equal(se_w, se_d) and np.array_equal(be_w, be_d)


def test_later_passes_equal_the_range_in_pieces_and_the_witness(engine):
    """32 n_cu + 7 realizations at 1024 points, three symbols each: every workgroup takes ten or eleven realizations in turn, so
    account_prev() runs for every it > 0 and the last realization of every workgroup is accounted behind the loop.  The same range
    in pieces of 251 (every workgroup's first pass only: accounted behind the loop alone) must give the same counts, the witness
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
    _, se_w, be_w, tag_w = _run(engine, kw, fft, first, n, OLD)
    assert tag_w == _tag(fft, "/a")
    print("%d realizations: symbol errors %d whole / %d in pieces / %d witness, realizations that differ %d / %d" %
          (n, int(se.sum()), int(se_p.sum()), int(se_w.sum()), int(np.count_nonzero(se != se_p)), int(np.count_nonzero(se != se_w))))
    assert np.array_equal(se, se_p) and np.array_equal(be, be_p)
    assert np.array_equal(se, se_w) and np.array_equal(be, be_w)
    assert res["n_realizations"] == n and res["sym_errors"] == int(se_p.sum()) and res["bit_errors"] == int(be_p.sum())
    for lo in (0, n - edge):
        want_se, want_be = _oracle(case, fft, first + lo, edge)
        assert np.array_equal(se[lo:lo + edge], want_se) and np.array_equal(be[lo:lo + edge], want_be)
