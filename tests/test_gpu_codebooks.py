"""GPU: the chordal-distance operator mcle_chordal_min_dist (csrc/kernels_codebook.hip) on the nine stored codebooks of
tests/golden/g4_codebooks.npz against the reference's own values, in both arithmetics, and the Python surface on top of it
(subspace.chordal_distances, CodebookFinder.calc_min_chordal_dist).

Tolerance: absolute on d^2, 8 x the error of the NumPy restatement (tests/codebook_oracle.py) in the same arithmetic against
the reference on the same nine codebooks (2.3e-15 and 6.2e-7 here; tests/test_codebooks_cpu.py holds them below 2.4e-15 and
6.5e-7) -- the factor covers another summation order, Gram-Schmidt against Householder and the accumulation of the matrix
cores."""
import itertools

import numpy as np
import pytest

import codebook_oracle as co
from conftest import load_golden
from pyphysim_amd import subspace
from pyphysim_amd.codebooks import CodebookFinder

pytestmark = pytest.mark.gpu

NP_DTYPE = {"f64": np.complex128, "f32": np.complex64}


@pytest.fixture(scope="module")
def golden():
    return load_golden("g4_codebooks")


@pytest.fixture(scope="module")
def tolerance(golden):
    """8 x the restatement's worst |d^2 error| against the reference on the nine codebooks, per arithmetic; computed once"""
    tol = {}
    for name, dtype in NP_DTYPE.items():
        worst = 0.0
        for Nt, Ns, K in golden["stored_shapes"]:
            key = "g%d_%d_k%d" % (Nt, Ns, K)
            d2 = co.d2_matrix(golden[key + "_codebook"].astype(dtype))
            worst = max(worst, float(np.abs(co.pair_vector(d2) - golden[key + "_pair_d2"]).max()))
        tol[name] = 8.0 * worst
    return tol


def keys(g):
    return ["g%d_%d_k%d" % (Nt, Ns, K) for Nt, Ns, K in g["stored_shapes"]]


def upper(d2):
    K = d2.shape[0]
    iu = np.triu_indices(K, 1)
    return d2[iu]                                  # row-major upper triangle = itertools.combinations order


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_operator_on_the_stored_codebooks(engine, golden, tolerance, dtype):
    tol, worst = tolerance[dtype], 0.0
    for key in keys(golden):
        C = golden[key + "_codebook"]
        K = len(C)
        m, pair, d2 = engine.chordal_min_dist(C, dtype=dtype, full=True)
        assert engine.last_kernel() == "chordal_min_dist %s p%d" % (dtype, 16 // (K * C.shape[2]) if K * C.shape[2] <= 8 else 1)
        assert d2.shape == (K, K) and np.array_equal(d2, d2.T) and not d2.diagonal().any()
        err = float(np.abs(upper(d2) - golden[key + "_pair_d2"]).max())
        worst = max(worst, err)
        print("%s %s: worst |d^2 - reference| %.3g (tolerance %.3g)" % (key, dtype, err, tol))
        assert err <= tol, key
        want = list(itertools.combinations(range(K), 2))[int(np.argmin(golden[key + "_pair_dist"]))]
        assert tuple(pair) == want, key
        assert m == d2[want]                                               # the minimum IS the matrix entry
        bd = float(golden[key + "_best_dist"])
        assert abs(m - bd * bd) <= tol, key
        assert abs(np.sqrt(m) - bd) <= tol / bd, key
        # without the matrix, and with the other form: the same bits
        m2, pair2 = engine.chordal_min_dist(C, dtype=dtype)
        assert m2 == m and np.array_equal(pair2, pair)
        with engine.options(codebook_no_pack=1):
            m3, pair3, d3 = engine.chordal_min_dist(C, dtype=dtype, full=True)
        assert m3 == m and np.array_equal(pair3, pair) and np.array_equal(d3, d2)
    print("operator %s: worst |d^2 - reference| over the nine codebooks %.3g" % (dtype, worst))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_python_surface_on_the_stored_codebooks(engine, golden, tolerance, dtype):
    tol = tolerance[dtype]
    for key in keys(golden):
        C = golden[key + "_codebook"]
        D = subspace.chordal_distances(C, engine=engine, dtype=dtype)
        assert D.shape == (len(C), len(C)) and not D.diagonal().any()
        assert np.abs(upper(D) ** 2 - golden[key + "_pair_d2"]).max() <= tol + 1e-15, key
        md, angles = CodebookFinder.calc_min_chordal_dist(C, engine=engine, dtype=dtype)
        bd = float(golden[key + "_best_dist"])
        assert abs(md - bd) <= tol / bd, key
        # host arccos of singular values near 1: a rounding of 2e-16 in s moves the angle by up to sqrt(2 x 2e-16) = 2e-8
        np.testing.assert_allclose(angles, golden[key + "_best_principal_angles"], rtol=0, atol=1e-7, err_msg=key)
        assert abs(subspace.calc_chordal_distance_from_principal_angles(angles) - bd) <= 1e-13, key


def test_a_batch_of_codebooks_equals_one_at_a_time(engine, golden):
    """[n, K, Nt, Ns] in one call: every codebook as when it is alone (n not a multiple of the codebooks per trip)."""
    for key, n in (("g3_1_k3", 7), ("g3_2_k16", 3)):
        C = golden[key + "_codebook"]
        rs = np.random.RandomState(5)
        batch = np.stack([C] + [C[rs.permutation(len(C))] * np.exp(2j * np.pi * rs.rand()) for _ in range(n - 1)])
        for dtype in ("f64", "f32"):
            m, pair, d2 = engine.chordal_min_dist(batch, dtype=dtype, full=True)
            assert m.shape == (n,) and pair.shape == (n, 2) and d2.shape == (n, len(C), len(C))
            for i in range(n):
                mi, pi, di = engine.chordal_min_dist(batch[i], dtype=dtype, full=True)
                assert mi == m[i] and np.array_equal(pi, pair[i]) and np.array_equal(di, d2[i]), (key, dtype, i)
    m, pair = engine.chordal_min_dist(np.zeros((0, 4, 3, 1), dtype=np.complex128))
    assert m.shape == (0,) and pair.shape == (0, 2) and engine.last_kernel() == ""
