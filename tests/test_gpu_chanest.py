"""GPU: mcle_cazac_estimate (csrc/kernels_chanest.hip) and the Python estimator classes against the reference's own
numbers (tests/golden/g1_chanest.npz) and the NumPy restatement (tests/chanest_oracle.py)."""
import ctypes
import os

import numpy as np
import pytest

import chanest_oracle as co
from helpers import GOLDEN
from pyphysim_amd import _lib, reference_signals as rs
from pyphysim_amd.channel_estimation import CazacBasedChannelEstimator, CazacBasedWithOCCChannelEstimator

pytestmark = pytest.mark.gpu

F64_TOL, F32_TOL = 1e-11, 2e-5          # the project's operator tolerances (tests/test_gpu_operators.py)
TOL = {"f64": F64_TOL, "f32": F32_TOL}

# name -> (K, m, normalised): the cases of scripts/make_golden_chanest.py
CASES = {"ne36": (3, 2, False), "ne37_all": (36, 2, False), "ne64_m1": (8, 1, False), "ne150": (15, 2, False),
         "ne150_k70": (70, 2, False), "ne139_norm": (40, 2, True), "k0": (0, 2, False), "ne2048": (15, 2, False),
         "rows67": (5, 2, False)}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "g1_chanest.npz"), allow_pickle=False)


def rel(got, want):
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_operator_equals_the_reference(engine, gold, name, dtype):
    K, m, norm = CASES[name]
    ref, rx, want = (gold["est_%s_%s" % (name, k)] for k in ("ref", "rx", "out"))
    got = engine.cazac_estimate(ref, rx, K, size_multiplier=m, normalized=norm, dtype=dtype)
    assert got.shape == want.shape and got.dtype == (np.complex128 if dtype == "f64" else np.complex64)
    e = rel(got, want)
    print(name, dtype, "relative error %.3g" % e, engine.last_kernel())
    assert e <= TOL[dtype]
    assert engine.last_kernel().startswith("cazac_estimate " + dtype)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_table_in_global_memory(engine, dtype):
    """4096 samples with more than half the taps kept leave no room for the table in LDS (complex128): it is read from
    global memory; complex64 keeps it in LDS.  Checked against the restatement."""
    ne, K = 4096, 2100
    rng = np.random.RandomState(5)
    ref = np.exp(2j * np.pi * rng.rand(ne))
    rx = rng.randn(ne) + 1j * rng.randn(ne)
    got = engine.cazac_estimate(ref, rx, K, size_multiplier=1, dtype=dtype)
    e = rel(got, co.estimate(ref, rx, K, 1))
    print(dtype, "relative error %.3g" % e, engine.last_kernel())
    assert e <= TOL[dtype]
    assert engine.last_kernel().endswith(" gtw") == (dtype == "f64")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_batch_invariance(engine, gold, dtype):
    ref, rx = gold["est_rows67_ref"], gold["est_rows67_rx"]
    whole = engine.cazac_estimate(ref, rx, 5, dtype=dtype)
    for step in (1, 2, 64):
        parts = [engine.cazac_estimate(ref, rx[i:i + step], 5, dtype=dtype) for i in range(0, 67, step)]
        assert np.array_equal(np.concatenate(parts), whole), step


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_more_rows_than_the_grid_holds(engine, dtype):
    """The launcher caps the grid at 8 workgroups per compute unit, four rows each: with more rows than that every wavefront
    takes a second trip of the grid-stride loop (its LDS reused for another row).  Against the restatement, and the same
    rows in two calls (which moves every row of the second call to another wavefront and trip) bit for bit."""
    ne, K = 48, 5
    rows = 8 * engine.n_cu * 4 * 2 + 67
    rng = np.random.RandomState(11)
    ref = rs.SrsUeSequence(rs.RootSequence(root_index=7, size=ne), 5).seq_array()
    rx = rng.randn(rows, ne) + 1j * rng.randn(rows, ne)
    got = engine.cazac_estimate(ref, rx, K, dtype=dtype)
    assert engine.last_kernel().endswith("w4")
    want = co.estimate(ref, rx, K, 2)
    worst = float(np.max(np.max(np.abs(got - want), axis=1) / np.max(np.abs(want), axis=1)))          # row by row
    print(dtype, rows, "rows, worst row %.3g" % worst)
    assert worst <= TOL[dtype]
    cut = 8 * engine.n_cu * 4 + 1
    parts = [engine.cazac_estimate(ref, rx[:cut], K, dtype=dtype), engine.cazac_estimate(ref, rx[cut:], K, dtype=dtype)]
    assert np.array_equal(np.concatenate(parts), got)


def test_argument_rules_return_errors_without_launching(engine):
    lib, ctx = engine.lib, engine.ctx
    buf = engine.zeros(4098 * 2, np.complex128)
    args = dict(dtype=_lib.MCLE_F64, ne=48, rows=1, n_cover=1, K=5, m=2)

    def call(**kw):
        a = dict(args, **kw)
        rc = lib.mcle_cazac_estimate(ctx, a["dtype"], buf.ptr, a["ne"], buf.ptr, a["rows"], a["n_cover"], None, a["K"],
                                     a["m"], 0, buf.ptr)
        return rc, lib.mcle_last_error().decode(), engine.last_kernel()

    for kw, word in ((dict(dtype=7), "dtype"), (dict(ne=1), "at least 2"), (dict(K=48), "num_taps_to_keep"),
                     (dict(ne=2049), "4096"), (dict(m=0), "size_multiplier"), (dict(K=-1), "num_taps_to_keep"),
                     (dict(n_cover=9), "cover"), (dict(n_cover=0), "cover"), (dict(n_cover=2), "null cover")):
        rc, msg, kernel = call(**kw)
        assert rc == -1 and word in msg and kernel == "", (kw, rc, msg, kernel)
    assert 2 * 2049 == 4098
    rc, msg, kernel = call(rows=0)
    assert rc == 0 and kernel == ""
    assert lib.mcle_cazac_estimate(None, 1, None, 48, None, 1, 1, None, 5, 2, 0, None) == -1
    with pytest.raises(ValueError, match="num_taps_to_keep"):
        engine.cazac_estimate(np.ones(8), np.ones(8), 8)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_python_estimator_shapes(engine, gold, dtype):
    """1-D, 2-D and batched 3-D input, a sequence object and a plain array: all equal the restatement."""
    rng = np.random.RandomState(9)
    ue = rs.SrsUeSequence(rs.RootSequence(root_index=25, size=150), 3)
    for seq, norm in ((ue, False), (ue.seq_array(), False),
                      (rs.SrsUeSequence(rs.RootSequence(root_index=17, Nzc=139), 7, normalize=True), True)):
        est = CazacBasedChannelEstimator(seq, size_multiplier=2, engine=engine, dtype=dtype)
        arr = seq if isinstance(seq, np.ndarray) else seq.seq_array()
        for shape in ((arr.size,), (4, arr.size), (5, 4, arr.size)):
            y = (rng.randn(*shape) + 1j * rng.randn(*shape)) * (1 / np.sqrt(arr.size) if norm else 1.0)
            got = est.estimate_channel_freq_domain(y, 15)
            want = co.estimate(arr, y, 15, 2, norm)
            assert got.shape == want.shape and rel(got, want) <= TOL[dtype], shape
    with pytest.raises(ValueError):
        est.estimate_channel_freq_domain(np.zeros((2, 2, 2, 139), dtype=complex), 3)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_cover_code_estimator_layouts(engine, gold, dtype):
    ue = rs.DmrsUeSequence(rs.RootSequence(root_index=15, size=48), 4, cover_code=np.array([1, -1]))
    assert float(np.max(np.abs(ue.seq_array() - gold["occ_ref"]))) <= 1e-12
    est = CazacBasedWithOCCChannelEstimator(ue, engine=engine, dtype=dtype)
    rx = gold["occ_rx"]                                                       # [3 antennas, 2, 48]
    for got, want in ((est.estimate_channel_freq_domain(rx, 5), gold["occ_out"]),
                      (est.estimate_channel_freq_domain(rx.reshape(3, 96), 5, extra_dimension=False), gold["occ_out_flat"]),
                      (est.estimate_channel_freq_domain(rx[0], 5), gold["occ_out_1ant"]),
                      (est.estimate_channel_freq_domain(rx[0].reshape(96), 5, extra_dimension=False), gold["occ_out_1ant"]),
                      (est.estimate_channel_freq_domain(np.stack([rx, 2 * rx]), 5), np.stack([gold["occ_out"], 2 * gold["occ_out"]])),
                      (est.estimate_channel_freq_domain(np.stack([rx, 2 * rx]).reshape(2, 3, 96), 5, extra_dimension=False),
                       np.stack([gold["occ_out"], 2 * gold["occ_out"]]))):
        assert got.shape == want.shape and rel(got, want) <= TOL[dtype]
    with pytest.raises(RuntimeError):
        est.estimate_channel_freq_domain(np.zeros((2, 2, 2, 2, 48), dtype=complex), 5)
