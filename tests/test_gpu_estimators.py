"""GPU: the staged LS / MMSE block-pilot estimators mcle_ls_estimate and mcle_mmse_estimate (csrc/kernels_estimators.hip)
against the reference's own numbers (tests/golden/g3_estimators.npz), batch-split invariance bit for bit, more
realizations than one pass of the grid holds, every argument rule, and the reference-shaped functions of
pyphysim_amd.estimators on top.  Tolerances: the project's operator tolerances, relative to the largest element of the
expected array."""
import ctypes
import os

import numpy as np
import pytest

import estimators_oracle as eo
from helpers import GOLDEN
from pyphysim_amd import _lib
from pyphysim_amd import estimators as est
from pyphysim_amd.engine import DeviceArray

pytestmark = pytest.mark.gpu

TOL = {"f64": 1e-11, "f32": 2e-5}
CDT = {"f64": np.complex128, "f32": np.complex64}
LS_CASES = ["nr3_2d", "nr5_shared", "nr5_per", "nr17_b37", "nr67_per", "p_eq_nt", "nr128"]
MMSE_CASES = ["nr3_2d", "nr3_b2", "nr3_per", "nr16_b37", "nr67", "nr128"]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "g3_estimators.npz"), allow_pickle=False)


def rel_err(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.max(np.abs(got.astype(np.complex128) - want)) / np.max(np.abs(want)))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("case", LS_CASES)
def test_ls_equals_the_reference(engine, gold, case, dtype):
    Y, s, want = gold["ls_%s_Y" % case], gold["ls_%s_s" % case], gold["ls_%s_out" % case]
    got = est.compute_ls_estimation(Y, s, engine=engine, dtype=dtype)
    e = rel_err(got, want)
    print(case, dtype, "ls %.3g" % e, engine.last_kernel())
    assert got.dtype == CDT[dtype] and e <= TOL[dtype]
    assert engine.last_kernel().startswith("ls_estimate %s nt" % dtype)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("case", MMSE_CASES)
def test_mmse_equals_the_reference(engine, gold, case, dtype):
    Y, s, C = gold["mmse_%s_Y" % case], gold["mmse_%s_s" % case], gold["mmse_%s_C" % case]
    want = gold["mmse_%s_out" % case]
    got = est.compute_mmse_estimation(Y, s, float(gold["mmse_%s_noise_power" % case]), C, engine=engine, dtype=dtype)
    e = rel_err(got, want)
    print(case, dtype, "mmse %.3g" % e, engine.last_kernel())
    assert got.dtype == CDT[dtype] and e <= TOL[dtype]
    assert engine.last_kernel() == "mmse_estimate %s ga" % dtype


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_batch_split_is_bit_identical(engine, gold, dtype):
    """The batch-37 cases in steps of 1, 2 and 16: a realization's place in a 16-realization tile, in a workgroup's trip and
    the masked tail all move; every output stays bit for bit."""
    Y, s = gold["ls_nr17_b37_Y"], gold["ls_nr17_b37_s"]
    Ym, sm, C = gold["mmse_nr16_b37_Y"], gold["mmse_nr16_b37_s"], gold["mmse_nr16_b37_C"]
    whole_ls = engine.ls_estimate(Y, s, dtype=dtype)
    whole_mm = engine.mmse_estimate(Ym, sm, 0.5, C, dtype=dtype)
    per = np.sqrt(1.5) * np.exp(2j * np.pi * np.random.RandomState(5).rand(37, 3, 7))
    whole_per = engine.ls_estimate(Y, per, dtype=dtype)
    for step in (1, 2, 16):
        cuts = list(range(0, 37, step))
        assert np.array_equal(np.concatenate([engine.ls_estimate(Y[c:c + step], s, dtype=dtype) for c in cuts]), whole_ls), step
        assert np.array_equal(np.concatenate([engine.mmse_estimate(Ym[c:c + step], sm, 0.5, C, dtype=dtype) for c in cuts]),
                              whole_mm), step
        assert np.array_equal(np.concatenate([engine.ls_estimate(Y[c:c + step], per[c:c + step], dtype=dtype) for c in cuts]),
                              whole_per), step


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_shared_pilots_equal_the_same_pilots_repeated(engine, gold, dtype):
    Y, s = gold["ls_nr17_b37_Y"], gold["ls_nr17_b37_s"]
    a = engine.ls_estimate(Y, s, dtype=dtype)
    b = engine.ls_estimate(Y, np.repeat(s[None], 37, axis=0), dtype=dtype)
    assert rel_err(b, gold["ls_nr17_b37_out"]) <= TOL[dtype] and rel_err(a, b.astype(np.complex128)) <= TOL[dtype]
    Ym, sm, C = gold["mmse_nr16_b37_Y"], gold["mmse_nr16_b37_s"], gold["mmse_nr16_b37_C"]
    a = engine.mmse_estimate(Ym, sm, 0.5, C, dtype=dtype)
    b = engine.mmse_estimate(Ym, np.repeat(sm[None], 37, axis=0), 0.5, C, dtype=dtype)
    assert rel_err(b, gold["mmse_nr16_b37_out"]) <= TOL[dtype] and rel_err(a, b.astype(np.complex128)) <= TOL[dtype]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_more_realizations_than_the_grid_holds(engine, dtype):
    """mcle_ls_estimate launches at most 8 workgroups per compute unit of 32 realizations a trip, mcle_mmse_estimate (with
    grid_oversub = 1) 16 one-wavefront workgroups per compute unit of 16 realizations: both hold 256 realizations per compute
    unit in one pass.  Twice that and a ragged tail makes every workgroup take a second and some a third trip (the LDS of
    the previous tile reused, the masked tail in a later trip).  Against the restatement, and bit for bit against a
    two-call split that moves every tile."""
    nr, P = 3, 4
    per_pass = 256 * engine.n_cu
    batch = 2 * per_pass + 37
    rng = np.random.RandomState(11)
    Y = (rng.randn(batch, nr, P) + 1j * rng.randn(batch, nr, P)).astype(CDT[dtype])
    s = np.sqrt(1.5) * np.exp(2j * np.pi * rng.rand(1, P))
    C = eo.toeplitz_cov(nr, 0.9, 0.49)
    d_Y = engine.to_device(Y)
    cut = per_pass + 3
    with engine.options(grid_oversub=1):
        ls = engine.ls_estimate(d_Y, engine.to_device(s, CDT[dtype]), dtype=dtype).get()
        mm = engine.mmse_estimate(d_Y, engine.to_device(s, CDT[dtype]), 0.5, C, dtype=dtype).get()
        ls2 = np.concatenate([engine.ls_estimate(Y[:cut], s, dtype=dtype), engine.ls_estimate(Y[cut:], s, dtype=dtype)])
        mm2 = np.concatenate([engine.mmse_estimate(Y[:cut], s, 0.5, C, dtype=dtype),
                              engine.mmse_estimate(Y[cut:], s, 0.5, C, dtype=dtype)])
    Y128 = Y.astype(np.complex128)
    e_ls, e_mm = rel_err(ls, eo.ls_estimate(Y128, s)), rel_err(mm, eo.mmse_estimate(Y128, s, 0.5, C))
    print(dtype, "batch", batch, "ls %.3g mmse %.3g" % (e_ls, e_mm))
    assert e_ls <= TOL[dtype] and e_mm <= TOL[dtype]
    assert np.array_equal(ls2, ls) and np.array_equal(mm2, mm)


def test_every_argument_rule_is_refused(engine):
    Y, s1, s2 = np.ones((2, 3, 10), complex), np.ones((1, 10), complex), np.ones((2, 10), complex)
    C = 0.49 * np.eye(3)
    d_Y, d_s, d_out = engine.to_device(Y), engine.to_device(s1), engine.empty((2, 3, 2), np.complex128)
    lib, ctx = engine.lib, engine.ctx
    c_ptr = np.ascontiguousarray(C, dtype=np.complex128).view(np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def ls(dtype=_lib.MCLE_F64, Y=d_Y.ptr, s=d_s.ptr, nr=3, nt=1, P=10, per=0, batch=2, out=d_out.ptr):
        return lib.mcle_ls_estimate(ctx, dtype, Y, s, nr, nt, P, per, batch, out)

    def mmse(dtype=_lib.MCLE_F64, Y=d_Y.ptr, s=d_s.ptr, nr=3, P=10, per=0, batch=2, noise=0.5, cov=c_ptr, out=d_out.ptr):
        return lib.mcle_mmse_estimate(ctx, dtype, Y, s, nr, P, per, batch, noise, cov, out)

    def refused(rc, word):
        assert rc == -1 and word in lib.mcle_last_error().decode(), (rc, lib.mcle_last_error().decode())
        assert engine.last_kernel() == ""

    assert ls() == 0 and engine.last_kernel() == "ls_estimate f64 nt1"
    for fn in (ls, mmse):
        refused(fn(dtype=7), "dtype")
        refused(fn(nr=0), "nr")
        refused(fn(nr=129), "nr")
        refused(fn(P=0), "n_pilots")
        refused(fn(P=1025), "n_pilots")
        refused(fn(per=2), "s_per_realization")
        refused(fn(Y=None), "null array")
        refused(fn(s=None), "null array")
        refused(fn(out=None), "null array")
        assert fn(batch=0, Y=None, s=None, out=None) == 0 and engine.last_kernel() == ""
    refused(ls(nt=0), "nt")
    refused(ls(nt=9), "nt")
    refused(ls(nt=8, P=7), "n_pilots")
    refused(mmse(noise=-0.1), "noise_power")
    refused(mmse(noise=float("nan")), "noise_power")
    refused(mmse(cov=None), "cov")
    bad = np.array(C, dtype=np.complex128)
    bad[1, 2] = np.inf
    refused(mmse(cov=bad.view(np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))), "cov")
    zero = np.zeros((3, 3), np.complex128)
    refused(mmse(noise=0.0, cov=zero.view(np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))), "singular")
    assert mmse() == 0 and engine.last_kernel() == "mmse_estimate f64 ga"
    # the Python layer's own shape rules
    with pytest.raises(ValueError, match="nt = 1"):
        engine.mmse_estimate(Y, np.ones((2, 10), complex), 0.5, C)
    with pytest.raises(ValueError, match="does not match"):
        engine.ls_estimate(Y, np.ones((3, 1, 10), complex))
    with pytest.raises(ValueError, match="2-D s"):
        est.compute_ls_estimation(Y[0], s2[None], engine=engine)
    with pytest.raises(ValueError, match=r"C must be \[3, 3\]"):
        engine.mmse_estimate(Y, s1, 0.5, np.eye(4))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_python_functions_return_the_reference_shapes(engine, gold, dtype):
    Y, s, C = gold["mmse_nr3_b2_Y"], gold["mmse_nr3_b2_s"], gold["mmse_nr3_b2_C"]
    per = gold["mmse_nr3_per_s"]
    kw = dict(engine=engine, dtype=dtype)
    for got, shape in ((est.compute_ls_estimation(Y[0], s, **kw), (3, 1)),
                       (est.compute_ls_estimation(Y, s, **kw), (2, 3, 1)),
                       (est.compute_ls_estimation(Y, per, **kw), (2, 3, 1)),
                       (est.compute_mmse_estimation(Y[0], s, 0.5, C, **kw), (3, 1)),
                       (est.compute_mmse_estimation(Y, s, 0.5, C, **kw), (2, 3, 1)),
                       (est.compute_mmse_estimation(Y, per, 0.5, C, **kw), (2, 3, 1))):
        assert isinstance(got, np.ndarray) and got.shape == shape and got.dtype == CDT[dtype]
    # a 2-D call is the first realization of the 3-D one
    assert np.array_equal(est.compute_mmse_estimation(Y[0], s, 0.5, C, **kw), est.compute_mmse_estimation(Y, s, 0.5, C, **kw)[0])
    # device arrays stay on the device
    d = est.compute_ls_estimation(engine.to_device(Y[0], CDT[dtype]), engine.to_device(s, CDT[dtype]), **kw)
    assert isinstance(d, DeviceArray) and d.shape == (3, 1)
    assert rel_err(d.get(), eo.ls_estimate(Y[0], s)) <= TOL[dtype]
