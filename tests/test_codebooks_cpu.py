"""CPU: the NumPy restatement of the codebook search (tests/codebook_oracle.py) against the reference's values in
tests/golden/g4_codebooks.npz, the host functions of pyphysim_amd.subspace against the same fixture, the positions of the
draw ledger, and every argument rule of mcle_chordal_min_dist / mcle_codebook_generate / mcle_run_codebook_search (the
shape rules are checked before the context, so they can be told without a device)."""
import ctypes
import itertools
from ctypes import byref

import numpy as np
import pytest

import codebook_oracle as co
from conftest import load_golden
from oracle import philox
from pyphysim_amd import _lib, subspace
from pyphysim_amd.codebooks import CodebookFinder

SEED = 20261018
# what the issue measured for the restatement against the reference over all 51 stored codebooks; the nine of the fixture stay below
BASE_LIMIT = {np.complex128: 2.4e-15, np.complex64: 6.5e-7}


@pytest.fixture(scope="module")
def golden():
    return load_golden("g4_codebooks")


def stored_keys(g):
    return ["g%d_%d_k%d" % (Nt, Ns, K) for Nt, Ns, K in g["stored_shapes"]]


def restatement_base_error(g, dtype):
    """Worst |d^2 of the restatement in `dtype` - the reference's| over every pair of the nine stored codebooks: the base
    figure of the GPU tolerance (times 8, tests/test_gpu_codebooks.py)."""
    worst = 0.0
    for key in stored_keys(g):
        d2 = co.d2_matrix(g[key + "_codebook"].astype(dtype))
        worst = max(worst, float(np.abs(co.pair_vector(d2) - g[key + "_pair_d2"]).max()))
    return worst


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
def test_restatement_reproduces_the_reference_on_the_stored_codebooks(golden, dtype):
    base = restatement_base_error(golden, dtype)
    print("restatement against the reference, %s: worst |d^2 error| %.3g" % (np.dtype(dtype).name, base))
    assert base <= BASE_LIMIT[dtype]
    for key in stored_keys(golden):
        C = golden[key + "_codebook"]
        d2 = co.d2_matrix(C.astype(dtype))
        assert np.array_equal(d2, d2.T) and not d2.diagonal().any()
        m, pair = co.min_and_pair(d2)
        want = int(np.argmin(golden[key + "_pair_dist"]))                       # the reference's argmin
        assert pair == list(itertools.combinations(range(len(C)), 2))[want], key
        bd = float(golden[key + "_best_dist"])
        assert abs(m - bd * bd) <= 8 * BASE_LIMIT[dtype], key
        assert abs(np.sqrt(m) - bd) <= 8 * BASE_LIMIT[dtype] / bd, key


def test_stored_distances_are_consistent(golden):
    for key in stored_keys(golden):
        d, d2 = golden[key + "_pair_dist"], golden[key + "_pair_d2"]
        np.testing.assert_allclose(d * d, d2, rtol=0, atol=1e-15)
        assert abs(d.min() - float(golden[key + "_best_dist"])) <= 1e-14


def test_restatement_on_the_drawn_pairs(golden):
    for name in golden["drawn_names"]:
        key = "drawn_%s" % name
        A, B = golden[key + "_A"], golden[key + "_B"]
        d2 = co.d2_matrix(np.stack([A, B]).astype(np.complex128))[0, 1]
        for ref in ("_dist_from_angles", "_dist", "_dist2"):
            assert abs(np.sqrt(d2) - float(golden[key + ref])) <= 1e-13, (name, ref)


def test_subspace_host_functions_match_the_reference(golden):
    for name in golden["drawn_names"]:
        key = "drawn_%s" % name
        A, B, v, M = (golden[key + s] for s in ("_A", "_B", "_v", "_M"))
        pa = subspace.calc_principal_angles(A, B)
        np.testing.assert_allclose(pa, golden[key + "_angles"], rtol=0, atol=2e-8)      # (arccos near 1 loses half the digits)
        tight = dict(rtol=0, atol=1e-13)
        np.testing.assert_allclose(subspace.calc_chordal_distance_from_principal_angles(golden[key + "_angles"]),
                                   golden[key + "_dist_from_angles"], **tight)
        np.testing.assert_allclose(subspace.calc_chordal_distance_from_principal_angles(pa), golden[key + "_dist_from_angles"],
                                   **tight)
        np.testing.assert_allclose(subspace.calc_chordal_distance(A, B), golden[key + "_dist"], **tight)
        np.testing.assert_allclose(subspace.calc_chordal_distance_2(A, B), golden[key + "_dist2"], **tight)
        P = subspace.Projection(A)
        np.testing.assert_allclose(P.Q, golden[key + "_Q"], **tight)
        np.testing.assert_allclose(P.oQ, golden[key + "_oQ"], **tight)
        np.testing.assert_allclose(subspace.calcProjectionMatrix(A), golden[key + "_calcQ"], **tight)
        np.testing.assert_allclose(subspace.calcOrthogonalProjectionMatrix(A), golden[key + "_calcoQ"], **tight)
        for x, tag in ((v, "v"), (M, "M")):
            np.testing.assert_allclose(P.project(x), golden[key + "_project_" + tag], **tight)
            np.testing.assert_allclose(P.oProject(x), golden[key + "_oproject_" + tag], **tight)
            np.testing.assert_allclose(P.reflect(x), golden[key + "_reflect_" + tag], **tight)
        assert P.project(x).dtype == golden[key + "_project_M"].dtype


def test_ledger_positions():
    """Candidate 5 of the seed, K = 3 precoders in G(2, 1): entry i = (k Nt + t) Ns + s."""
    z = philox.cnormal(SEED, 5, 6, philox.STREAM_CHAN)
    u = philox.uniforms(SEED, 5, 6, philox.STREAM_PHASE)
    assert abs(z[0] - (1.5857079798247364 + 1.0117403879448321j)) < 1e-15
    assert abs(u[5] - 0.7872336222790182) < 1e-16
    C = co.codebook(SEED, 5, 3, 2, 1, "complex")
    np.testing.assert_allclose(C.reshape(3, 2), z.reshape(3, 2) / np.linalg.norm(z.reshape(3, 2), axis=1, keepdims=True), atol=1e-15)
    known = {"complex": [0.6519881602564268 + 0.41599258034016007j, -0.04359580877232182 - 0.6324247128669648j,
                         0.41250648062803613 + 0.2318652680346984j],
             "real": [0.8430219279844284, 0.5378791954866977, -0.81656926353159],
             "qegt": [0.9982813721491132 + 0.05860291818744043j, 0.19295908799095154 + 0.9812068030551461j,
                      -0.7847985670034475 + 0.6197509251540777j]}
    for kind, want in known.items():
        got = co.codebook(SEED, 5, 3, 2, 1, kind).reshape(-1)[[0, 1, 5]]
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-15, err_msg=kind)
    R = co.codebook(SEED, 5, 3, 2, 1, "real")
    # real: entries 2 j and 2 j + 1 are the two parts of CN sample j
    raw = np.sqrt(2.0) * np.stack([z[:3].real, z[:3].imag], axis=-1)
    np.testing.assert_allclose(R.reshape(3, 2), raw / np.linalg.norm(raw, axis=1, keepdims=True), atol=1e-15)
    assert not R.imag.any()
    Q = co.codebook(SEED, 5, 3, 2, 1, "qegt")
    np.testing.assert_allclose(Q.reshape(-1), np.exp(1j * np.pi * u), atol=1e-15)
    # a larger shape: entry (k, t, s) sits at (k Nt + t) Ns + s
    z = philox.cnormal(SEED, 7, 4 * 3 * 2, philox.STREAM_CHAN).reshape(4, 3, 2)
    C = co.codebook(SEED, 7, 4, 3, 2, "complex")
    np.testing.assert_allclose(C[2, 1, 1] * np.linalg.norm(z[2]), z[2, 1, 1], atol=1e-15)
    np.testing.assert_allclose(np.linalg.norm(C, axis=(1, 2)), 1.0, atol=1e-15)


def test_orthonormal_bases_and_search_rules():
    C = co.codebook(SEED, 1, 9, 4, 3, "complex")
    Q = co.orthonormal_bases(C)
    G = np.einsum("kts,ktu->ksu", Q.conj(), Q)
    np.testing.assert_allclose(G, np.broadcast_to(np.eye(3), G.shape), atol=1e-15)
    # the same subspace as the reduced QR
    for k in range(9):
        Qr = np.linalg.qr(C[k])[0]
        np.testing.assert_allclose(Q[k] @ Q[k].conj().T, Qr @ Qr.conj().T, atol=1e-14)
    res = co.search(SEED, 3, 6, 3, 2, 1, "complex")
    assert res["best_index"] == 3 + int(np.argmax(res["min_d2"])) and res["best_min_d2"] == res["min_d2"].max()
    d2 = np.zeros((3, 3))
    d2[0, 1] = d2[1, 0] = d2[1, 2] = d2[2, 1] = 0.25
    d2[0, 2] = d2[2, 0] = 0.5
    assert co.min_and_pair(d2) == (0.25, (0, 1))                      # the first of two equal pairs


def test_finder_surface_without_a_device():
    assert (CodebookFinder.COMPLEX, CodebookFinder.REAL, CodebookFinder.COMPLEX_QEGT) == (0, 1, 2)
    assert CodebookFinder.type_to_string(CodebookFinder.REAL) == "Real"
    f = CodebookFinder(3, 1, 16, CodebookFinder.COMPLEX_QEGT, prng_seed=4)
    assert f.type == "Complex QEG" and f.min_dist == 0 and f.codebook is None and "G(3,1)" in repr(f)
    with pytest.raises(ValueError):
        CodebookFinder(2, 2, 4)


# ---- the argument rules of the C ABI ---------------------------------------------------------------------------------
SHAPE_RULES = [
    # (K, Nt, Ns), fragment of the message
    ((4, 1, 1), b"Nt must be in [2, 8] (got 1)"),
    ((4, 9, 1), b"Nt must be in [2, 8] (got 9)"),
    ((4, 4, 0), b"Ns must be in [1, min(Nt - 1, 4)] (got 0 with Nt 4)"),
    ((4, 4, 4), b"Ns must be in [1, min(Nt - 1, 4)] (got 4 with Nt 4)"),
    ((4, 8, 5), b"Ns must be in [1, min(Nt - 1, 4)] (got 5 with Nt 8)"),
    ((1, 4, 2), b"K must be at least 2 (got 1)"),
    ((-3, 4, 2), b"K must be at least 2 (got -3)"),
    ((257, 2, 1), b"K * Ns must be at most 256 (got 257)"),
    ((65, 8, 4), b"K * Ns must be at most 256 (got 260)"),
]


def _refused(rc, lib, fragment):
    assert rc == -1
    assert fragment in lib.mcle_last_error(), lib.mcle_last_error()


@pytest.mark.parametrize("shape,fragment", SHAPE_RULES)
def test_shape_rules_of_the_three_entry_points(shape, fragment):
    lib = _lib.load()
    K, Nt, Ns = shape
    res = _lib.CodebookResult()
    for dt in (_lib.MCLE_F32, _lib.MCLE_F64):
        _refused(lib.mcle_chordal_min_dist(None, dt, None, 1, K, Nt, Ns, None, None, None), lib, fragment)
        _refused(lib.mcle_codebook_generate(None, dt, 0, K, Nt, Ns, 1, 0, 1, None), lib, fragment)
        cfg = _lib.CodebookCfg(K, Nt, Ns, 0)
        _refused(lib.mcle_run_codebook_search(None, dt, byref(cfg), 1, 0, 1, byref(res), None, None), lib, fragment)


def test_the_other_rules_that_precede_the_context():
    lib = _lib.load()
    res = _lib.CodebookResult()
    good = _lib.CodebookCfg(16, 3, 1, 0)
    for dt in (-1, 2):
        _refused(lib.mcle_chordal_min_dist(None, dt, None, 1, 16, 3, 1, None, None, None), lib, b"dtype must be MCLE_F32 or MCLE_F64")
        _refused(lib.mcle_codebook_generate(None, dt, 0, 16, 3, 1, 1, 0, 1, None), lib, b"dtype must be MCLE_F32 or MCLE_F64")
        _refused(lib.mcle_run_codebook_search(None, dt, byref(good), 1, 0, 1, byref(res), None, None), lib,
                 b"dtype must be MCLE_F32 or MCLE_F64")
    for t in (-1, 3):
        fragment = b"type must be 0 (complex), 1 (real) or 2 (qegt) (got %d)" % t
        _refused(lib.mcle_codebook_generate(None, 1, t, 16, 3, 1, 1, 0, 1, None), lib, fragment)
        cfg = _lib.CodebookCfg(16, 3, 1, t)
        _refused(lib.mcle_run_codebook_search(None, 1, byref(cfg), 1, 0, 1, byref(res), None, None), lib, fragment)
    big = 1 << 31
    _refused(lib.mcle_chordal_min_dist(None, 1, None, big, 16, 3, 1, None, None, None), lib, b"n_codebooks must be at most 2^31-1")
    _refused(lib.mcle_codebook_generate(None, 1, 0, 16, 3, 1, 1, 0, big, None), lib, b"count must be at most 2^31-1")
    _refused(lib.mcle_run_codebook_search(None, 1, byref(good), 1, 0, big, byref(res), None, None), lib,
             b"count must be at most 2^31-1")
    _refused(lib.mcle_run_codebook_search(None, 1, None, 1, 0, 1, byref(res), None, None), lib, b"null cfg")
    _refused(lib.mcle_run_codebook_search(None, 1, byref(good), 1, 0, 1, None, None, None), lib, b"null out")
    # a valid request without a context
    _refused(lib.mcle_chordal_min_dist(None, 1, None, 1, 16, 3, 1, None, None, None), lib, b"null context")
    _refused(lib.mcle_codebook_generate(None, 1, 0, 16, 3, 1, 1, 0, 1, None), lib, b"null context")
    _refused(lib.mcle_run_codebook_search(None, 1, byref(good), 1, 0, 1, byref(res), None, None), lib, b"null context")


def test_structures_match_the_header():
    assert ctypes.sizeof(_lib.CodebookCfg) == 16 and ctypes.sizeof(_lib.CodebookResult) == 32
    assert _lib.CodebookResult.pair.offset == 16 and _lib.CodebookResult.n_candidates.offset == 24
    assert _lib.OPTIONS["codebook_no_pack"] == 17 and _lib.CODEBOOK_TYPES == {"complex": 0, "real": 1, "qegt": 2}
