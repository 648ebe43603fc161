"""The part-wave complex128 kernel of config 4's link (csrc/pipeline_mimo_pw.hip) with its (antenna, time class) partial transforms
dealt BY LANE ROW (round 10): lane row rho of wavefront w owns the pair f = NW antenna + class = 4 w + rho, the two
samples of a Philox noise block sit sixteen lanes apart in one wavefront, their words change rows in registers (no LDS round trip)
and barrier B1 is gone.  The map of rounds 6 - 9 (wavefront = class, row = antenna) stays behind f64_threads = 266, tag suffix "/a".
No floating-point operation or operand changed, so the per-realization symbol AND bit error counts of the two maps must be EQUAL, and
equal to the oracle chain's (oracle/chains.py::chain_mimo_ofdm).

GPU: 512 / 1024 / 2048 points over 256 / 128 / 64 realizations: MMSE and ZF, one and three OFDM symbols, prefix 0 and 16, QPSK and
64-QAM, both demodulators; the kernel tag (mcle_ctx_last_kernel) proves which map served a call; 32 n_cu + 7 realizations (later
passes of the persistent loop: the accounting of the previous realization now sits behind B2) against the same range in pieces of
251; the two-wavefront register bound; a request outside the envelope lands where it did, whatever the option says.
Reference: apps/mimo/simulate_mimo.py:68-142, mimo/mimo.py:609-660, modulators/ofdm.py:52-94, :394-466."""
import functools

import numpy as np
import pytest

from oracle import chains, modem as omodem
from pyphysim_amd import _lib

gpu = pytest.mark.gpu
SEED = 1380649
CASES = [dict(mod="qam", M=64, snr_db=18.0),                                               # MMSE, prefix 16, one symbol
         dict(mod="qam", M=64, snr_db=18.0, cp_size=0, mmse=False, n_ofdm_sym=3),          # ZF, no prefix, three symbols
         dict(mod="qpsk", M=4, snr_db=5.0, cp_size=0, n_ofdm_sym=3),                       # quadrant certificate, MMSE, three symbols
         dict(mod="qpsk", M=4, snr_db=5.0, mmse=False)]                                    # ZF, prefix 16, one symbol
DEPTH = {512: 256, 1024: 128, 2048: 64}
OLD = 266                                  # f64_threads: the default form with the ownership map of rounds 6 - 9
TWO = {512: 262, 1024: 264}                # the two-wavefronts-per-SIMD register bound (2048 has the one bound)


def _set(engine, kw):
    engine.set_constellation(chains.constellation(kw["mod"], kw["M"]), _lib.CONST_QAM if kw["mod"] == "qam" else _lib.CONST_GENERIC)


def _run(engine, kw, fft, first, count, method, threads, cp=None):
    nv = 1.0 / omodem.dB2Linear(kw["snr_db"])
    with engine.options(f64_threads=threads):
        out = engine.run_mimo_ofdm(4, 4, fft, kw.get("cp_size", 16) if cp is None else cp, fft, kw.get("n_ofdm_sym", 1), nv, SEED, first,
                                   count, mmse=kw.get("mmse", True), method=method, dtype="f64", per_realization=True)
        return out + (engine.last_kernel(),)


@functools.lru_cache(maxsize=None)
def _oracle(case, fft, cp=None, count=None):
    """computed once per (case, size) and shared; the arrays are not written to"""
    kw = CASES[case]
    first, count = (1 << 33) + 613 * case, count or DEPTH[fft]
    okw = dict(mod=kw["mod"], M=kw["M"], nt=4, nr=4, fft_size=fft, cp_size=kw.get("cp_size", 16) if cp is None else cp, num_used=fft,
               n_ofdm_sym=kw.get("n_ofdm_sym", 1), snr_db=kw["snr_db"], mmse=kw.get("mmse", True))
    want = [chains.chain_mimo_ofdm(chains.PhiloxRng(SEED, r), **okw) for r in range(first, first + count)]
    se, be = np.array([w["symbol_errors"] for w in want]), np.array([w["bit_errors"] for w in want])
    se.setflags(write=False)
    be.setflags(write=False)
    return first, count, se, be


def _methods(kw):
    return [_lib.DEMOD_MINDIST] + ([_lib.DEMOD_QAM_SLICER] if kw["mod"] == "qam" else [])


def _tag(fft, old=False, two=False):
    return "mimo_ofdm_pw<%d>/freq%s%s" % (fft // 256, "/w2" if two else "", "/a" if old else "")


@gpu
@pytest.mark.parametrize("fft", [512, 1024, 2048])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_both_maps_equal_each_other_and_the_oracle(engine, case, fft):
    kw = CASES[case]
    _set(engine, kw)
    first, count, want_se, want_be = _oracle(case, fft)
    assert want_se.sum() > 100                                       # the comparison has something to compare
    for method in _methods(kw):
        res, se, be, tag = _run(engine, kw, fft, first, count, method, 0)
        res_a, se_a, be_a, tag_a = _run(engine, kw, fft, first, count, method, OLD)
        print("case %d fft %d method %d: %s / %s, symbol errors %d / %d (oracle %d), realizations that differ %d / %d" %
              (case, fft, method, tag, tag_a, int(se.sum()), int(se_a.sum()), int(want_se.sum()),
               int(np.count_nonzero(se != want_se)), int(np.count_nonzero(se_a != want_se))))
        assert tag == _tag(fft) and tag_a == _tag(fft, old=True)
        assert np.array_equal(se, se_a) and np.array_equal(be, be_a)
        assert np.array_equal(se, want_se), (method, np.flatnonzero(se != want_se)[:5])
        assert np.array_equal(be, want_be), (method, np.flatnonzero(be != want_be)[:5])
        assert res["n_realizations"] == count and res["n_skipped"] == 0
        assert res["sym_errors"] == int(want_se.sum()) and res["bit_errors"] == int(want_be.sum())
        assert res_a["sym_errors"] == res["sym_errors"] and res_a["bit_errors"] == res["bit_errors"]


@gpu
@pytest.mark.parametrize("fft", [512, 1024, 2048])
def test_later_passes_of_the_persistent_loop(engine, fft):
    """32 n_cu + 7 realizations: every workgroup takes several realizations in turn (512: six or seven, 1024: ten or eleven, 2048: eight
    or nine), so the double-buffered record, the accounting of the previous realization behind B2 and the reuse of the planes without
    B1 all run.  The same range in pieces of 251 (every workgroup's first pass only) and the other map must give the same counts."""
    kw = CASES[1]                                                   # three symbols: every realization counts errors
    _set(engine, kw)
    first, n, piece = 662607015, 32 * engine.n_cu + 7, 251
    res, se, be, tag = _run(engine, kw, fft, first, n, _lib.DEMOD_MINDIST, 0)
    res_a, se_a, be_a, tag_a = _run(engine, kw, fft, first, n, _lib.DEMOD_MINDIST, OLD)
    assert tag == _tag(fft) and tag_a == _tag(fft, old=True)
    assert se.shape == (n,) and se.min() > 0
    se_p, be_p = np.empty_like(se), np.empty_like(be)
    for off in range(0, n, piece):
        k = min(piece, n - off)
        _, se_p[off:off + k], be_p[off:off + k], _ = _run(engine, kw, fft, first + off, k, _lib.DEMOD_MINDIST, 0)
    print("fft %d: %d realizations, symbol errors %d / %d in pieces / %d other map, realizations that differ %d / %d" %
          (fft, n, int(se.sum()), int(se_p.sum()), int(se_a.sum()), int(np.count_nonzero(se != se_p)), int(np.count_nonzero(se != se_a))))
    assert np.array_equal(se, se_p) and np.array_equal(be, be_p)
    assert np.array_equal(se, se_a) and np.array_equal(be, be_a)
    assert res["n_realizations"] == n and res["sym_errors"] == int(se_p.sum()) and res["bit_errors"] == int(be_p.sum())


@gpu
@pytest.mark.parametrize("fft", [512, 1024])
def test_two_wavefront_bound(engine, fft):
    """f64_threads = TWO[fft]: the new map under the two-wavefronts-per-SIMD register bound, tag "/w2" as before."""
    case = 0 if fft == 1024 else 1
    kw = CASES[case]
    _set(engine, kw)
    first, count, want_se, want_be = _oracle(case, fft)
    for method in _methods(kw):
        res, se, be, tag = _run(engine, kw, fft, first, count, method, TWO[fft])
        assert tag == _tag(fft, two=True)
        assert np.array_equal(se, want_se) and np.array_equal(be, want_be)


@gpu
@pytest.mark.parametrize("fft", [512, 1024, 2048])
def test_outside_the_envelope_lands_where_it_did(engine, fft):
    """An odd cyclic prefix is outside the part-wave envelope: f64_threads = 0 and 266 both end on the planar family's kernel of
    this size, with the oracle's counts."""
    kw = CASES[0]
    _set(engine, kw)
    first, count, want_se, want_be = _oracle(0, fft, cp=15, count=16)
    res, se, be, tag = _run(engine, kw, fft, first, count, _lib.DEMOD_MINDIST, 0, cp=15)
    res_a, se_a, be_a, tag_a = _run(engine, kw, fft, first, count, _lib.DEMOD_MINDIST, OLD, cp=15)
    print("fft %d prefix 15: %s / %s" % (fft, tag, tag_a))
    assert tag.startswith("mimo_ofdm_planar<%d,4,4> f64" % fft) and tag_a.startswith("mimo_ofdm_planar<%d,4,4> f64" % fft)
    assert tag_a == tag
    assert np.array_equal(se, want_se) and np.array_equal(be, want_be)
    assert np.array_equal(se_a, want_se) and np.array_equal(be_a, want_be)
