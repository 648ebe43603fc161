"""GPU: the codebook channel quantizer mcle_quantize_links (csrc/kernels_quant.hip) against the NumPy restatement
(tests/quant_oracle.py) and the reference's own results (tests/golden/g6_quant_ia.npz).

Tolerance on a distance: 8 x the worst error of the restatement in the same arithmetic against the reference's calc_dist /
calc_angle_dist rows of the fixture (computed here, printed; about 1.8e-14 / 6e-15 in complex128 and 8.5e-6 / 2.8e-6 in
complex64).  An index is compared only where the restatement's gap between the link's two smallest distances exceeds twice that
tolerance; at most 1 % of a case's links may be left out that way (tests/test_quant_cpu.py asserts that the inputs meet the
cap).  The one exception is by construction: with dim = 1 under 'chordal' every codeword is at distance 0 from every link, all
links tie, and only the distances and big_Hq are checked."""
import ctypes
import functools

import numpy as np
import pytest

import quant_oracle as qo
from conftest import load_golden
from pyphysim_amd import _lib

pytestmark = pytest.mark.gpu

NP_DTYPE = {"f64": np.complex128, "f32": np.complex64}
CASE_ID = lambda c: "C%d_%dx%d_K%d_b%d" % c


@functools.lru_cache(maxsize=None)
def tolerance(metric, dtype):
    return qo.distance_tolerance(load_golden("g6_quant_ia"), metric, NP_DTYPE[dtype])


@functools.lru_cache(maxsize=None)
def want(case, metric, dtype):
    """The complex128 restatement on the case's inputs as rounded to `dtype`, computed once and shared."""
    C, nr, nt, K, batch = case
    H, cb = qo.operator_inputs(case, NP_DTYPE[dtype])
    return H, cb, qo.quantize(H, cb, K, nr, nt, metric)


def gather(cb, idx, K, nr, nt):
    b = idx.shape[0]
    return cb[idx].reshape(b, K, K, nr, nt).transpose(0, 1, 3, 2, 4).reshape(b, K * nr, K * nt)


def bit_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8),
                                                                         np.ascontiguousarray(b).view(np.uint8))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("metric", qo.METRICS)
@pytest.mark.parametrize("case", qo.OPERATOR_CASES, ids=CASE_ID)
def test_against_the_restatement(engine, case, metric, dtype):
    C, nr, nt, K, batch = case
    H, cb, w = want(case, metric, dtype)
    tol = tolerance(metric, dtype)
    idx, Hq, dist = engine.quantize_links(H, cb, K, nr, nt, metric=metric, dtype=dtype, with_dist=True)
    assert engine.last_kernel() == "quantize_links %s m%d" % (dtype, qo.METRICS.index(metric))
    err = float(np.abs(dist - w["dist"]).max())
    compared = w["gap"] > 2 * tol
    print("%s %s %s: worst |distance - restatement| %.3g (tolerance %.3g), %d of %d links compared"
          % (case, metric, dtype, err, tol, compared.sum(), compared.size))
    assert err <= tol
    if not (metric == "chordal" and nr * nt == 1):
        assert (~compared).sum() <= int(qo.GAP_CAP * compared.size)
    assert idx.dtype == np.int32 and idx.min() >= 0 and idx.max() < C
    assert np.array_equal(idx[compared], w["index"][compared])
    assert bit_equal(Hq, gather(cb, idx, K, nr, nt))


@pytest.mark.parametrize("ci", [0, 1, 2])
def test_fixture_gives_my_quant_func_exactly(engine, ci):
    g = load_golden("g6_quant_ia")
    pre = "cb%d_" % ci
    C, nr, nt, K = (int(x) for x in g[pre + "cfg"])
    idx, Hq = engine.quantize_links(g[pre + "H"], g[pre + "codebook"], K, nr, nt, dtype="f64")
    assert np.array_equal(idx, g[pre + "index"])
    assert bit_equal(Hq, g[pre + "Hq"])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("metric", qo.METRICS)
def test_duplicated_codewords_lower_index_wins(engine, metric, dtype):
    case = (512, 2, 2, 3, 33)
    H, cb, _ = want(case, metric, dtype)
    H, dup = H.copy(), cb.copy()
    pairs = [(0, 5), (3, 16), (17, 500)]
    for lo, hi in pairs:
        dup[hi] = dup[lo]
    # three links that ARE a duplicated word (scaled): both of its rows are at the same, smallest distance
    planted = [(0, 0, 0, 0), (1, 1, 2, 3), (2, 2, 1, 17)]
    for b, k1, k2, lo in planted:
        H[b, 2 * k1:2 * k1 + 2, 2 * k2:2 * k2 + 2] = (0.75 * cb[lo]).reshape(2, 2)
    idx_d = engine.quantize_links(H, dup, 3, 2, 2, metric=metric, dtype=dtype)[0]
    assert not np.isin(idx_d, [hi for _, hi in pairs]).any()
    keep = np.array([i for i in range(512) if i not in (5, 16, 500)])
    idx_k = engine.quantize_links(H, dup[keep], 3, 2, 2, metric=metric, dtype=dtype)[0]
    assert np.array_equal(keep[idx_k], idx_d)
    wk = qo.quantize(H, dup[keep], 3, 2, 2, metric)           # the restatement on the codebook without the upper rows
    compared = wk["gap"] > 2 * tolerance(metric, dtype)
    assert np.array_equal(idx_d[compared], keep[wk["index"]][compared])
    for b, k1, k2, lo in planted:
        assert idx_d[b, k1, k2] == lo


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("metric", qo.METRICS)
@pytest.mark.parametrize("case", [(17, 2, 2, 3, 7), (64, 6, 6, 2, 5)], ids=CASE_ID)
def test_scale_and_phase(engine, case, metric, dtype):
    C, nr, nt, K, batch = case
    H, cb, _ = want(case, metric, dtype)
    base = engine.quantize_links(H, cb, K, nr, nt, metric=metric, dtype=dtype, with_dist=True)
    for s in (2.0 ** -3, 2.0 ** 5):
        out = engine.quantize_links((H * s).astype(H.dtype), cb, K, nr, nt, metric=metric, dtype=dtype, with_dist=True)
        assert np.array_equal(out[0], base[0]) and bit_equal(out[1], base[1]) and bit_equal(out[2], base[2])
    Hj = H.copy()
    Hj[1, nr:2 * nr, 0:nt] *= 1j                       # link (1, 0) of realization 1
    if metric == "chordal":
        out = engine.quantize_links(Hj, cb, K, nr, nt, metric=metric, dtype=dtype, with_dist=True)
        assert np.array_equal(out[0], base[0]) and bit_equal(out[1], base[1]) and bit_equal(out[2], base[2])
    else:
        out = engine.quantize_links((1j * H).astype(H.dtype), (1j * cb).astype(cb.dtype), K, nr, nt, metric=metric, dtype=dtype)
        assert np.array_equal(out[0], base[0])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("metric", qo.METRICS)
def test_batch_position(engine, metric, dtype):
    """Whole, split at every position mod 16 of the flattened link index, and in reverse order: the same per-link output."""
    case = (17, 2, 2, 3, 33)          # K^2 = 9: the cut after b realizations is at link 9 b, every residue mod 16 for b = 1 .. 16
    H, cb = qo.operator_inputs(case, NP_DTYPE[dtype])
    whole = engine.quantize_links(H, cb, 3, 2, 2, metric=metric, dtype=dtype, with_dist=True)
    assert {(9 * b) % 16 for b in range(1, 17)} == set(range(16))
    for b in range(1, 17):
        lo = engine.quantize_links(H[:b], cb, 3, 2, 2, metric=metric, dtype=dtype, with_dist=True)
        hi = engine.quantize_links(H[b:], cb, 3, 2, 2, metric=metric, dtype=dtype, with_dist=True)
        for k in range(3):
            assert bit_equal(np.concatenate([lo[k], hi[k]]), whole[k]), (b, k)
    rev = engine.quantize_links(H[::-1].copy(), cb, 3, 2, 2, metric=metric, dtype=dtype, with_dist=True)
    for k in range(3):
        assert bit_equal(rev[k][::-1], whole[k])
    with engine.options(grid_oversub=1):
        one = engine.quantize_links(H, cb, 3, 2, 2, metric=metric, dtype=dtype, with_dist=True)
    for k in range(3):
        assert bit_equal(one[k], whole[k])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("metric", qo.METRICS)
def test_zero_block(engine, metric, dtype):
    H, cb = qo.operator_inputs((17, 2, 2, 3, 7), NP_DTYPE[dtype])
    H[2, 2:4, 4:6] = 0
    idx, Hq, dist = engine.quantize_links(H, cb, 3, 2, 2, metric=metric, dtype=dtype, with_dist=True)
    assert idx[2, 1, 2] == 0 and np.isnan(dist[2, 1, 2]) and np.isfinite(np.delete(dist.reshape(-1), 2 * 9 + 5)).all()
    assert bit_equal(Hq[2, 2:4, 4:6], cb[0].reshape(2, 2))


def test_argument_rules(engine):
    lib, ctx = engine.lib, engine.ctx
    H = engine.to_device(np.ones((2, 6, 6), dtype=np.complex128))
    cb = engine.to_device(np.ones((8, 4), dtype=np.complex128))
    idx = engine.empty((2, 3, 3), np.int32)

    def call(K=3, nr=2, nt=2, C=8, metric=0, bigH=H.ptr, codebook=cb.ptr, index=idx.ptr, cfg=True, dtype=_lib.dtype_code("f64")):
        q = _lib.QuantCfg(K, nr, nt, C, metric)
        rc = lib.mcle_quantize_links(ctx, dtype, ctypes.byref(q) if cfg else None, bigH, codebook, index, None, None, 2)
        return rc, lib.mcle_last_error().decode()

    assert call()[0] == 0
    for kw, word in ((dict(K=5), "K"), (dict(K=0), "K"), (dict(nr=7), "nr"), (dict(nt=0), "nt"), (dict(C=0), "n_codewords"),
                     (dict(C=4097), "n_codewords"), (dict(metric=2), "metric"), (dict(bigH=None), "d_bigH"),
                     (dict(codebook=None), "d_codebook"), (dict(index=None), "d_index"), (dict(cfg=False), "cfg"),
                     (dict(dtype=7), "dtype")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    with pytest.raises(ValueError):
        engine.quantize_links(np.ones((2, 6, 6)), np.ones((8, 4)), 3, 2, 2, metric=2)
    with pytest.raises(ValueError):
        engine.quantize_links(np.ones((2, 6, 6)), np.ones((8, 9)), 3, 2, 2)
    # batch 0 launches nothing
    q = _lib.QuantCfg(3, 2, 2, 8, 0)
    assert lib.mcle_quantize_links(ctx, _lib.dtype_code("f64"), ctypes.byref(q), None, None, None, None, None, 0) == 0


def test_quantization_module_on_the_engine(engine):
    from pyphysim_amd import quantization as qz
    g = load_golden("g6_quant_ia")
    cb, H = g["cb2_codebook"], g["cb2_H"]
    assert np.array_equal(qz.my_quant_func(H[0], 2, 2, 3, cb, engine=engine), g["cb2_Hq"][0])
    assert np.array_equal(qz.my_quant_func(H, 2, 2, 3, cb, engine=engine), g["cb2_Hq"])
    assert np.array_equal(qz.quant_small_matrix(H[1, 2:4, 0:2], cb, engine=engine), g["cb2_Hq"][1, 2:4, 0:2])
    book = qz.gen_codebook(33, 4, seed=11, engine=engine)
    assert book.shape == (33, 4) and np.allclose(np.linalg.norm(book, axis=1), 1.0, rtol=0, atol=1e-15)
    assert np.array_equal(book, qz.gen_codebook(33, 4, seed=11, engine=engine)) and not np.array_equal(book, qz.gen_codebook(33, 4, seed=12, engine=engine))
