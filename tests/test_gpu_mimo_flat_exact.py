"""GPU: the fused flat-fading MIMO pipeline (csrc/pipeline_mimo_flat.hip: mcle_run_mimo_flat) and the staged SVD / GMD
operators against an oracle that does not share their code.

SVD / GMD: jacobi_svd (csrc/mimo_svd.hpp) fixes the phase of every singular pair -- the largest-magnitude entry of each right
singular vector real and positive -- and oracle.mimo.canonical_svd is the NumPy statement of that convention on top of
LAPACK's SVD, so the complex128 kernel must reproduce the oracle's per-realization error counts EXACTLY, and the staged
operators its filters entry by entry.  tests/test_oracle_mimo_canonical.py (no GPU) holds the conditions on the inputs that
make "exactly" a fair demand: pivot lead >= 1e-6 (5.6e-4 on these channels), singular-value gap >= 1e-3 (4.8 %), every
estimate >= 1e-9 from a decision border (2.6e-7), and that the canonical and the LAPACK phases give OTHER counts (svd N = 3,
130 columns: 5645 against 5561), so a wrong rotation, an unsorted column or a bad pivot cannot pass.

MMSE: mmse=True routes the noise variance into blast_filter (Blast / MRC) and gmd_filters_dev (GMD); the oracle chain takes
the same flag, at an SNR where the MMSE and zero-forcing decisions differ.

Every run covers realizations 3 .. 72 (a wave takes 16: four full chunks and one of 6; the second workgroup has a single
busy wave) at 130 columns (even: two columns per lane, a last pass with one busy lane), 51 (odd: one column per lane, C
order for SVD / GMD) and 2 (a single pair).

Complex64: the project's bound for this kernel (helpers.check(exact=False): totals within 1e-4 of the symbols / bits of the
complex128 oracle) plus at most 3 symbol errors of difference in any realization.  Measured: the oracle's own link evaluated
in NumPy complex64 (est = A d + G n, A = G H W and G rounded from complex128:
test_oracle_mimo_canonical.py::test_the_reference_alone_stays_inside_the_complex64_bound) differs from the complex128
decisions in 0 symbols in every SVD / GMD case (27 cases, 70 realizations each); every complex64 case below prints the
device's difference from the oracle before it asserts."""
import numpy as np
import pytest

from oracle import mimo as omimo
from pyphysim_amd import _lib

from helpers import (FLAT_COLUMNS, FLAT_COUNT, FLAT_FIRST, FLAT_SNR, FORMS, FORM_COLUMNS, FORM_SHAPES, MMSE_CASES,
                     MMSE_COLUMNS, MMSE_SNR, SEED, SVD_GMD_CASES, check, flat_reference, relerr)

pytestmark = pytest.mark.gpu
DTYPES = [("f64", True), ("f32", False)]
KIND = {"qam": _lib.CONST_QAM, "bpsk": _lib.CONST_BPSK}
METHOD = {"mindist": _lib.DEMOD_MINDIST, "slicer": _lib.DEMOD_QAM_SLICER}


def _rel(a, b):
    """max |a - b| relative to the largest entry of b (helpers.relerr never scales by less than 1)."""
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def _run_and_check(engine, ref, scheme, nt, nr, ns, mmse, dt, exact, method=_lib.DEMOD_MINDIST):
    res, se, be = engine.run_mimo_flat(scheme, nt, nr, ns, ref["noise_var"], SEED, FLAT_FIRST, FLAT_COUNT, mmse=mmse,
                                       method=method, dtype=dt, per_realization=True)
    se, be = se.astype(np.int64), be.astype(np.int64)
    d_se, d_be = se - ref["se"], be - ref["be"]
    print("%s %dx%d columns=%d mmse=%d method=%d %s: device %d / oracle %d symbol errors (total diff %+d, max per realization %d), "
          "bit errors diff %+d" % (scheme, nt, nr, ns, mmse, method, dt, se.sum(), ref["se"].sum(), d_se.sum(),
                                   np.max(np.abs(d_se)), d_be.sum()))
    assert ref["se"].max() > 0                                   # an all-zero output cannot pass
    if exact:
        assert np.array_equal(se, ref["se"]) and np.array_equal(be, ref["be"])
    else:
        assert np.max(np.abs(d_se)) <= 3
    check(res, se, be, ref["se"], ref["be"], ref["nsym"], ref["nbits"], exact)
    return se, be


@pytest.mark.parametrize("dt,exact", DTYPES)
@pytest.mark.parametrize("ns", FLAT_COLUMNS)
@pytest.mark.parametrize("scheme,n,mmse", SVD_GMD_CASES, ids=lambda v: str(v))
def test_svd_gmd_against_the_canonical_oracle(engine, scheme, n, mmse, ns, dt, exact):
    """complex128: per-realization symbol and bit error counts EQUAL to chain_mimo_scheme(canonical=True); complex64: within the
    bound of the module docstring."""
    ref = flat_reference(scheme, "qam", 16, n, n, ns, FLAT_SNR, mmse, True)
    engine.set_constellation(ref["table"], _lib.CONST_QAM)
    _run_and_check(engine, ref, scheme, n, n, ns, mmse, dt, exact)


@pytest.mark.parametrize("dt,exact", DTYPES)
@pytest.mark.parametrize("ns", FLAT_COLUMNS)
def test_svd_gmd_with_the_slicer(engine, ns, dt, exact):
    """One case per scheme through the QAM slicer as well (complex64: the packed level-domain form at 3 layers)."""
    for scheme, n, mmse in (("svd", 3, False), ("gmd", 4, True)):
        ref = flat_reference(scheme, "qam", 16, n, n, ns, FLAT_SNR, mmse, True)
        engine.set_constellation(ref["table"], _lib.CONST_QAM)
        _run_and_check(engine, ref, scheme, n, n, ns, mmse, dt, exact, method=_lib.DEMOD_QAM_SLICER)


@pytest.mark.parametrize("dt,exact", DTYPES)
@pytest.mark.parametrize("ns", MMSE_COLUMNS)
@pytest.mark.parametrize("scheme,nt,nr", MMSE_CASES)
def test_blast_mrc_mmse(engine, scheme, nt, nr, ns, dt, exact):
    """mmse=True of Blast / MRC against chain_mimo_scheme(mmse=True) at 6 dB; the zero-forcing oracle's counts differ in some
    realization, so the zero-forcing filter cannot pass."""
    ref = flat_reference(scheme, "qam", 16, nt, nr, ns, MMSE_SNR, True, False)
    zf = flat_reference(scheme, "qam", 16, nt, nr, ns, MMSE_SNR, False, False)
    assert not np.array_equal(ref["se"], zf["se"])
    engine.set_constellation(ref["table"], _lib.CONST_QAM)
    se, _ = _run_and_check(engine, ref, scheme, nt, nr, ns, True, dt, exact)
    assert not np.array_equal(se, zf["se"])


@pytest.mark.parametrize("dt,exact", DTYPES)
@pytest.mark.parametrize("ns", FORM_COLUMNS)
@pytest.mark.parametrize("nt,nr", FORM_SHAPES)
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f[0])
def test_decision_forms_by_layer_count(engine, form, nt, nr, ns, dt, exact):
    """Every decision form of the symbol walk at 1 .. 4 layers (Blast zero forcing: a phase-free oracle).  complex64: the packed
    slicer masks the unused layers (layer_mask), the lockstep searches (candidate grid; plain search for M <= 8) carry
    est = 0 there; n_symbols / n_bits are exact, so a counted unused layer fails.  64-QAM also with the certificates off."""
    _id, mod, M, method, snr = form
    ref = flat_reference("blast", mod, M, nt, nr, ns, snr, False, False)
    engine.set_constellation(ref["table"], KIND.get(mod, _lib.CONST_GENERIC))
    _run_and_check(engine, ref, "blast", nt, nr, ns, False, dt, exact, method=METHOD[method])
    if M == 64:
        with engine.options(demod_nocert=1):
            _run_and_check(engine, ref, "blast", nt, nr, ns, False, dt, exact, method=METHOD[method])


@pytest.mark.parametrize("generic", [0, 1])
@pytest.mark.parametrize("n", [2, 3, 4])
def test_staged_svd_gmd_filters_entry_by_entry(engine, n, generic):
    """engine.svd_filters / gmd_filters on the 70 channels of the runs above: W and G within 1e-10 relative of the canonical
    oracle (double against double; singular-value gaps >= 4.8 %, so conditioning amplifies rounding by under about 1e3), R
    within 1e-11 (the bound of test_gmd_filters).  staged_generic = 1 selects the plain form wherever an operator has two;
    these two have a single form, so both settings must give the same answer."""
    H = flat_reference("svd", "qam", 16, n, n, 2, FLAT_SNR, False, True)["H"]
    with engine.options(staged_generic=generic):
        W, G, S = engine.svd_filters(H, dtype="f64")
        gm = {nv: engine.gmd_filters(H, nv, dtype="f64") for nv in (0.0, 0.05)}
    worst = 0.0
    for b in range(FLAT_COUNT):
        Wo, Go = omimo.scheme_filters("svd", H[b], canonical=True)
        worst = max(worst, _rel(W[b], Wo), _rel(G[b], Go))
        assert _rel(W[b], Wo) <= 1e-10 and _rel(G[b], Go) <= 1e-10, ("svd", n, b)
        assert relerr(S[b], np.linalg.svd(H[b])[1]) <= 1e-12
        Ro = omimo.gmd(*omimo.canonical_svd(H[b]))[1]
        for nv, (Wg, Gg, Rg) in gm.items():
            Wo, Go = omimo.scheme_filters("gmd", H[b], nv, canonical=True)
            worst = max(worst, _rel(Wg[b], Wo), _rel(Gg[b], Go))
            assert _rel(Wg[b], Wo) <= 1e-10 and _rel(Gg[b], Go) <= 1e-10, ("gmd", n, nv, b)
            assert relerr(Rg[b], Ro) <= 1e-11, ("gmd R", n, nv, b)
    print("N = %d staged_generic = %d: largest relative filter error %.3g" % (n, generic, worst))
