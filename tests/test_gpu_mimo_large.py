"""GPU: the large-array Blast link (csrc/pipeline_mimo_large.hip: mcle_run_mimo_large, 1 <= Nt <= 8, Nt <= Nr <= 16, on the matrix
cores) against oracle.chains.chain_mimo_scheme(scheme='blast'), which shares none of its code.

Complex128 must reproduce the oracle's per-realization symbol and bit error counts EXACTLY.  tests/test_mimo_large_cpu.py (no
GPU) holds what makes that a fair demand on these very inputs: the smallest decision margin is >= 1e6 times the difference
between the oracle's estimates and the kernels' formulation (Cholesky of the normal equations, A = G H / sqrt(Nt),
est = A x + G n) in every case.  Complex64: the project's bound (helpers.check(exact=False): totals within 1e-4 of the
symbols / bits) plus at most 3 symbol errors of difference in any realization -- the flat kernel's bound; the reference alone in
NumPy complex64 sits at 0 inside it (same file).  Every case prints the device's difference from the oracle before it asserts.

Every oracle run covers realizations 3 .. 72: a wavefront of the set-up kernel takes four (seventeen full and one of two), a
wavefront of the link sixteen (four full chunks and one of 6)."""
import numpy as np
import pytest

from oracle import chains
from oracle import modem as omodem
from pyphysim_amd import _lib, simulators
from pyphysim_amd._lib import McleError
from pyphysim_amd.engine import Engine
from pyphysim_amd.simulations import SimulationResults

from helpers import FLAT_COUNT, FLAT_FIRST, FORMS, SEED, check
from mimo_large_cases import (CASE_IDS, CASES, EDGE_COLUMNS, EDGE_SHAPES, EDGE_SNR, FLAT_NS, FLAT_SHAPES, FLAT_SNR, FORM_COLUMNS,
                              FORM_SHAPES, reference)

pytestmark = pytest.mark.gpu
DTYPES = [("f64", True), ("f32", False)]
KIND = {"qam": _lib.CONST_QAM, "bpsk": _lib.CONST_BPSK}
METHOD = {"mindist": _lib.DEMOD_MINDIST, "slicer": _lib.DEMOD_QAM_SLICER}
COUNTERS = ("n_realizations", "n_skipped", "sym_errors", "sym_errors_sq", "bit_errors", "bit_errors_sq")


def _run_and_check(engine, ref, nt, nr, ns, mmse, dt, exact, method=_lib.DEMOD_MINDIST):
    res, se, be = engine.run_mimo_large(nt, nr, ns, ref["noise_var"], SEED, FLAT_FIRST, FLAT_COUNT, mmse=mmse, method=method,
                                        dtype=dt, per_realization=True)
    se, be = se.astype(np.int64), be.astype(np.int64)
    d_se, d_be = se - ref["se"], be - ref["be"]
    print("large %dx%d columns=%d mmse=%d method=%d %s: device %d / oracle %d symbol errors (total diff %+d, max per realization %d), "
          "bit errors diff %+d" % (nt, nr, ns, mmse, method, dt, se.sum(), ref["se"].sum(), d_se.sum(), np.max(np.abs(d_se)),
                                   d_be.sum()))
    assert ref["se"].max() > 0                                   # an all-zero output cannot pass
    if exact:
        assert np.array_equal(se, ref["se"]) and np.array_equal(be, ref["be"])
    else:
        assert np.max(np.abs(d_se)) <= 3
    check(res, se, be, ref["se"], ref["be"], ref["nsym"], ref["nbits"], exact)
    return se, be


def _qam16(engine):
    engine.set_constellation(chains.constellation("qam", 16), _lib.CONST_QAM)


@pytest.mark.parametrize("dt,exact", DTYPES)
@pytest.mark.parametrize("nt,nr,mmse,snr,ns", CASES, ids=CASE_IDS)
def test_oracle_parity(engine, nt, nr, mmse, snr, ns, dt, exact):
    ref = reference(nt, nr, mmse, snr, ns)
    engine.set_constellation(ref["table"], _lib.CONST_QAM)
    se, _ = _run_and_check(engine, ref, nt, nr, ns, mmse, dt, exact)
    if mmse:                                                     # the zero-forcing filter cannot pass
        assert not np.array_equal(se, reference(nt, nr, False, snr, ns)["se"])


@pytest.mark.parametrize("ns", EDGE_COLUMNS)
@pytest.mark.parametrize("nt,nr", EDGE_SHAPES)
def test_tile_edges(engine, nt, nr, ns):
    """Column counts on each side of the 16- and 32-column tiles, odd and even, a single column."""
    ref = reference(nt, nr, False, EDGE_SNR, ns)
    engine.set_constellation(ref["table"], _lib.CONST_QAM)
    _run_and_check(engine, ref, nt, nr, ns, False, "f64", True)


@pytest.mark.parametrize("nt,nr", FLAT_SHAPES)
def test_agrees_with_the_flat_kernel(engine, nt, nr):
    """Inside the 4 x 4 envelope the two entry points draw the same realizations: equal counts in complex128, and the oracle's."""
    ref = reference(nt, nr, False, FLAT_SNR, FLAT_NS)
    engine.set_constellation(ref["table"], _lib.CONST_QAM)
    se, be = _run_and_check(engine, ref, nt, nr, FLAT_NS, False, "f64", True)
    _res, fse, fbe = engine.run_mimo_flat("blast", nt, nr, FLAT_NS, ref["noise_var"], SEED, FLAT_FIRST, FLAT_COUNT, dtype="f64",
                                          per_realization=True)
    assert np.array_equal(se, fse) and np.array_equal(be, fbe)


@pytest.mark.parametrize("dt,exact", DTYPES)
@pytest.mark.parametrize("ns", FORM_COLUMNS)
@pytest.mark.parametrize("nt,nr", FORM_SHAPES)
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f[0])
def test_decision_forms(engine, form, nt, nr, ns, dt, exact):
    """Every decision form (slicer, certificates, candidate grid, plain search) at 8 and 5 streams; n_symbols / n_bits are exact, so
    a counted padding stream fails.  64-QAM also with the certificates off."""
    _id, mod, M, method, snr = form
    ref = reference(nt, nr, False, snr, ns, mod, M)
    engine.set_constellation(ref["table"], KIND.get(mod, _lib.CONST_GENERIC))
    _run_and_check(engine, ref, nt, nr, ns, False, dt, exact, method=METHOD[method])
    if M == 64:
        with engine.options(demod_nocert=1):
            _run_and_check(engine, ref, nt, nr, ns, False, dt, exact, method=METHOD[method])


def test_ranges_and_statistics(engine):
    _qam16(engine)
    run = lambda first, count, **kw: engine.run_mimo_large(8, 8, 34, 0.01, SEED, first, count, dtype="f32",
                                                           method=_lib.DEMOD_QAM_SLICER, **kw)
    a, b, c = run(0, 100000), run(0, 33333), run(33333, 66667)
    for k in COUNTERS:
        assert a[k] == b[k] + c[k], k
    assert a["n_realizations"] == 100000 and a["sym_errors"] > 0 and a["n_symbols"] == 8 * 34 and a["n_bits"] == 4 * 8 * 34
    z = run(7, 0)
    assert all(z[k] == 0 for k in COUNTERS)
    for dt in ("f64", "f32"):
        clean = engine.run_mimo_large(8, 8, 34, 0.0, SEED, 0, 500, dtype=dt)
        assert clean["sym_errors"] == 0 and clean["bit_errors"] == 0 and clean["n_skipped"] == 0 and clean["n_realizations"] == 500
    zf = engine.run_mimo_large(8, 8, 20, 1.0, SEED, 0, 20000, dtype="f32")
    mm = engine.run_mimo_large(8, 8, 20, 1.0, SEED, 0, 20000, dtype="f32", mmse=True)
    print("8x8 0 dB: zero forcing %d, MMSE %d symbol errors" % (zf["sym_errors"], mm["sym_errors"]))
    assert mm["sym_errors"] < zf["sym_errors"]
    other = Engine(0, "f64")
    try:
        _qam16(other)
        for dt in ("f64", "f32"):
            mine = engine.run_mimo_large(5, 6, 51, 0.02, SEED, 3, 70, dtype=dt, per_realization=True)
            theirs = other.run_mimo_large(5, 6, 51, 0.02, SEED, 3, 70, dtype=dt, per_realization=True)
            assert mine[0] == theirs[0] and np.array_equal(mine[1], theirs[1]) and np.array_equal(mine[2], theirs[2])
    finally:
        other.close()


def test_envelope(engine):
    _qam16(engine)
    for nt, nr in ((0, 4), (9, 9), (8, 17), (5, 4)):
        with pytest.raises(McleError, match="antenna counts"):
            engine.run_mimo_large(nt, nr, 64, 0.1, SEED, 0, 4)
        assert engine.last_kernel() == ""
    with pytest.raises(McleError, match="n_symbols"):
        engine.run_mimo_large(8, 8, 0, 0.1, SEED, 0, 4)
    with pytest.raises(McleError, match="[Nn]oise variance"):
        engine.run_mimo_large(8, 8, 64, -0.1, SEED, 0, 4)
    with pytest.raises(McleError, match="at most 2\\^31-1"):
        engine.run_mimo_large(8, 8, 64, 0.1, SEED, 0, 2 ** 31)
    assert engine.last_kernel() == ""
    engine.run_mimo_large(8, 16, 64, 0.1, SEED, 0, 4, dtype="f64")
    assert engine.last_kernel() == "mimo_large_link f64 16x8 s12"
    engine.run_mimo_large(5, 6, 64, 0.1, SEED, 0, 4, dtype="f32")
    assert engine.last_kernel() == "mimo_large_link f32 6x5 s8"
    with pytest.raises(McleError):                               # the old entry point keeps its envelope
        engine.run_mimo_flat("blast", 5, 5, 64, 0.1, SEED, 0, 4)


def test_simulator(engine, tmp_path):
    kw = dict(Nt=8, Nr=8, NSymbs=64, rep_max=300, seed=11, dtype="f64", engine=engine, common_random_numbers=True)
    small = simulators.LargeMimoSimulator(SNR=[8, 14], batch_size=64, **kw)
    small.simulate()
    big = simulators.LargeMimoSimulator(SNR=[8, 14], batch_size=300, **kw)
    big.simulate()
    names = ("ser", "ber", "symbol_errors", "bit_errors", "num_symbols", "num_bits")
    for name in names:
        assert small.results.get_result_values_list(name) == big.results.get_result_values_list(name), name
    for i, snr in enumerate((8.0, 14.0)):
        engine.set_constellation(chains.constellation("qam", 16), _lib.CONST_QAM)
        c = engine.run_mimo_large(8, 8, 64, 1.0 / float(omodem.dB2Linear(snr)), 11, 0, 300, method=small.demod_method, dtype="f64")
        assert small.results.get_result_values_list("symbol_errors")[i] == c["sym_errors"] > 0
        assert small.results.get_result_values_list("bit_errors")[i] == c["bit_errors"]
        assert small.results.get_result_values_list("ser")[i] == c["sym_errors"] / (300 * 8 * 64)
        assert small.results.get_result_values_list("ber")[i] == c["bit_errors"] / (300 * 8 * 64 * 4)
    assert small.runned_reps == [300, 300]
    small.results.set_parameters(small.params)
    for ext in ("pickle", "json"):
        back = SimulationResults.load_from_file(small.results.save_to_file(str(tmp_path / ("large." + ext))))
        for name in names:
            assert back.get_result_values_list(name) == small.results.get_result_values_list(name), (ext, name)
    with pytest.raises(ValueError):
        simulators.LargeMimoSimulator(SNR=[10.0], Nt=9, Nr=9)
