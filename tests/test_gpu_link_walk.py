"""GPU: what the record-walking link kernels share (csrc/link_walk.hpp, csrc/wave_draws.hpp, csrc/pipe_common.hpp).

* k_ia_link through every decision form: run_ia (closed form, K = 3, 2 x 2) against oracle.chains.chain_ia, realizations 61 .. 69,
  helpers.FORMS x both arithmetics at 126 columns (even and below 128, so k_ia_link serves the call; the last pass has 63 busy lanes),
  51 (odd: one column per lane) and 2.  complex128: equal per-realization counts; complex64: helpers.check(exact=False), the rule of
  test_ia_pipeline.  The oracle itself makes errors in every case at the SNRs of FORMS (at 2 columns x 9 realizations: 4, 4, 3, 2
  and 7 symbol errors), asserted per case.
* The draw-position rule (check_link_draws): rows x n_symbols beyond 2^31 - 1 is refused before anything is launched, the largest
  accepted product still passes the argument checks.
* The Fortran-order symbol pair (fortran_symbol_pair) at every alignment: Blast with three layers -- the one layer count at which a
  column pair straddles two Philox blocks -- at 2, 6, 12 and 130 columns, through run_mimo_flat and run_mimo_pilot_link (P = 7),
  complex128, exact."""
import functools

import numpy as np
import pytest

import pilot_link_oracle as po
from helpers import FLAT_COUNT, FLAT_FIRST, FORMS, SEED, check, flat_reference
from oracle import chains
from oracle import modem as omodem
from pyphysim_amd import _lib
from pyphysim_amd._lib import McleError

pytestmark = pytest.mark.gpu
KIND = {"qam": _lib.CONST_QAM, "bpsk": _lib.CONST_BPSK}
METHOD = {"mindist": _lib.DEMOD_MINDIST, "slicer": _lib.DEMOD_QAM_SLICER}
IA_FIRST, IA_COUNT = 61, 9
IA_COLUMNS = (126, 51, 2)


@functools.lru_cache(maxsize=None)
def ia_reference(mod, M, ns, snr):
    kw = dict(mod=mod, M=M, K=3, nr=2, nt=2, Ns=1, NSymbs=ns, snr_db=snr)
    want = [chains.chain_ia(chains.PhiloxRng(SEED, r), **kw) for r in range(IA_FIRST, IA_FIRST + IA_COUNT)]
    se, be = np.array([w["symbol_errors"] for w in want]), np.array([w["bit_errors"] for w in want])
    se.setflags(write=False)
    be.setflags(write=False)
    return se, be


@pytest.mark.parametrize("dt,exact", [("f64", True), ("f32", False)])
@pytest.mark.parametrize("ns", IA_COLUMNS)
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f[0])
def test_ia_link_through_every_decision_form(engine, form, ns, dt, exact):
    fid, mod, M, method, snr = form
    want_se, want_be = ia_reference(mod, M, ns, snr)
    assert want_se.max() > 0                                   # an all-zero output cannot pass
    engine.set_constellation(chains.constellation(mod, M), KIND.get(mod, _lib.CONST_GENERIC))
    bits = int(np.log2(M))

    def once():
        res, se, be, _, _ = engine.run_ia(ns, 1.0 / omodem.dB2Linear(snr), SEED, IA_FIRST, IA_COUNT, method=METHOD[method], dtype=dt,
                                          per_realization=True)
        se, be = se.astype(np.int64), be.astype(np.int64)
        print("%s columns=%d %s: device %d / oracle %d symbol errors, %d / %d bit errors" %
              (fid, ns, dt, se.sum(), want_se.sum(), be.sum(), want_be.sum()))
        check(res, se, be, want_se, want_be, 3 * ns, 3 * ns * bits, exact)

    once()
    if M == 64:
        with engine.options(demod_nocert=1):
            once()


BIG = 357913942          # 6 x BIG = 2^31 + 4: the first n_symbols the six noise rows of the IA link cannot address


def _refused_untouched(engine, call):
    cnt = engine.new_counters()
    before = engine.read_counters(cnt)
    with pytest.raises(McleError, match="draw positions are 32-bit"):
        call(1, cnt)
    assert engine.read_counters(cnt) == before


def test_draw_positions_beyond_32_bits_are_refused(engine):
    """flat, IA, IA-quantized and BD refuse rows x n_symbols > 2^31 - 1 (their kernels form the position in 32 bits); nothing is
    launched and the counters stay as they were.  The largest accepted product passes every argument check (count = 0 returns
    before a launch)."""
    engine.set_constellation(chains.constellation("qam", 16), _lib.CONST_QAM)
    codebook = np.eye(4, dtype=np.complex128)
    calls = {
        "flat": (lambda ns: lambda count, cnt: engine.run_mimo_flat("blast", 1, 4, ns, 0.1, SEED, 0, count, dtype="f64", counters=cnt),
                 2 ** 29, 2 ** 29 - 1),
        "ia": (lambda ns: lambda count, cnt: engine.run_ia(ns, 0.1, SEED, 0, count, dtype="f64", counters=cnt), BIG, BIG - 1),
        "bd": (lambda ns: lambda count, cnt: engine.run_bd(3, 2, ns, 1.0, 0.1, SEED, 0, count, dtype="f64", counters=cnt), BIG, BIG - 1),
    }
    for name, (make, bad, good) in calls.items():
        _refused_untouched(engine, make(bad))
        make(good)(0, None)
    # (Engine.run_ia_quantized reports the library's invalid-argument status as ValueError, like every call of its family)
    with pytest.raises((McleError, ValueError), match="draw positions are 32-bit"):
        engine.run_ia_quantized(BIG, 0.1, SEED, 0, 1, codebook, dtype="f64")
    engine.run_ia_quantized(BIG - 1, 0.1, SEED, 0, 0, codebook, dtype="f64")


PAIR_COLUMNS = (2, 6, 12, 130)


@pytest.mark.parametrize("ns", PAIR_COLUMNS)
def test_fortran_pair_three_layers_flat(engine, ns):
    ref = flat_reference("blast", "qam", 16, 3, 4, ns, 10.0, False, False)
    assert ref["se"].max() > 0
    engine.set_constellation(ref["table"], _lib.CONST_QAM)
    res, se, be = engine.run_mimo_flat("blast", 3, 4, ns, ref["noise_var"], SEED, FLAT_FIRST, FLAT_COUNT, dtype="f64",
                                       per_realization=True)
    check(res, se.astype(np.int64), be.astype(np.int64), ref["se"], ref["be"], ref["nsym"], ref["nbits"], True)


@functools.lru_cache(maxsize=None)
def pilot_reference(ns):
    cfg = po.make_case(3, 4, 7, ns, 10.0, 1.0, True, "random")
    return cfg, po.run(cfg, po.FIRST, po.COUNT)


@pytest.mark.parametrize("ns", PAIR_COLUMNS)
def test_fortran_pair_three_layers_pilot_link(engine, ns):
    cfg, ref = pilot_reference(ns)
    assert ref["se"].max() > 0
    engine.set_constellation(po.table(), _lib.CONST_QAM)
    c_est, c_perf, se, be, _, _ = engine.run_mimo_pilot_link(3, 4, 7, ns, cfg["noise_var"], cfg["seed"], po.FIRST, po.COUNT,
                                                             pilot_power=cfg["pilot_power"], alpha=cfg["alpha"], mmse=cfg["mmse"],
                                                             dtype="f64", per_realization=True)
    se, be = se.astype(np.int64), be.astype(np.int64)
    for b, cnt in enumerate((c_est, c_perf)):
        check(cnt, se[b], be[b], ref["se"][b], ref["be"][b], ref["n_symbols"], ref["n_bits"], True)
