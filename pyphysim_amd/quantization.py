"""Limited-feedback channel quantization: the functions of the reference's apps/ia/simple_maxsinr_quantized.py (:15-154) under
their own names.  Every link of an interference channel is replaced by the nearest word of a vector codebook.

With an ``engine`` the searches run on the GPU (Engine.quantize_links, csrc/kernels_quant.hip); without one they are plain NumPy.
"""
import numpy as np

METRICS = ("euclidean", "chordal")


def gen_codebook(codebook_size, dimension, seed=0, engine=None, dtype="f64"):
    """A random vector codebook [codebook_size, dimension] of unit-norm rows h / ||h||, h ~ CN(0, I): row i is the CN samples
    0 .. dimension - 1 of the channel stream of realization i of ``seed`` (mcle-philox-v1, Engine.randn_c_batch), normalised on
    the host -- once-per-scenario code.

    The reference takes U[:, 0] of an SVD of h, which is h / ||h|| times a phase that LAPACK chooses: the same distribution
    (isotropic on the unit sphere), not the same numbers."""
    own = engine is None
    if own:
        from .engine import Engine
        engine = Engine(0, dtype)
    try:
        h = engine.randn_c_batch(int(dimension), int(seed), 0, int(codebook_size), dtype=dtype).get()
    finally:
        if own:
            engine.close()
    h = h.astype(np.complex128)
    return h / np.linalg.norm(h, axis=1, keepdims=True)


def calc_dist(vec, codeword):
    """|| vec / ||vec|| - codeword ||^2 (app :40-63)."""
    vec, codeword = np.asarray(vec), np.asarray(codeword)
    return np.linalg.norm(vec / np.linalg.norm(vec) - codeword) ** 2


def calc_angle_dist(vec, codeword):
    """1 - |vec^H codeword|^2 / (||vec||^2 ||codeword||^2): the squared sine of the angle between the two (app :66-87)."""
    vec, codeword = np.asarray(vec), np.asarray(codeword)
    cos_sq = np.abs(np.vdot(vec, codeword) / (np.linalg.norm(vec) * np.linalg.norm(codeword))) ** 2
    return 1 - cos_sq


def _metric_fn(metric):
    if metric not in METRICS:
        raise ValueError("metric must be 'euclidean' or 'chordal' (got %r)" % (metric,))
    return calc_dist if metric == "euclidean" else calc_angle_dist


def quant_small_matrix(small_matrix, codebook, metric="euclidean", engine=None):
    """The codeword nearest to the link ``small_matrix`` [Nr, Nt], reshaped to its shape (app :90-110).  ``codebook``
    [C, Nr Nt], a row per codeword.  A matrix of zeros takes codeword 0 (argmin over all-NaN distances)."""
    small_matrix, codebook = np.asarray(small_matrix), np.asarray(codebook)
    nr, nt = small_matrix.shape
    if engine is not None:
        return np.asarray(engine.quantize_links(small_matrix, codebook, 1, nr, nt, metric=metric)[1])
    fn = _metric_fn(metric)
    with np.errstate(invalid="ignore", divide="ignore"):
        dists = [fn(small_matrix.reshape(-1), c) for c in codebook]
    return codebook[int(np.argmin(dists))].reshape(small_matrix.shape)


def my_quant_func(true_matrix, Nr, Nt, K, codebook, metric="euclidean", engine=None):
    """Quantizes the K x K links of ``true_matrix`` [K Nr, K Nt] (or a batch [n, K Nr, K Nt] with an engine) (app :113-154)."""
    true_matrix, codebook = np.asarray(true_matrix), np.asarray(codebook)
    Nr, Nt, K = int(Nr), int(Nt), int(K)
    if engine is not None:
        return np.asarray(engine.quantize_links(true_matrix, codebook, K, Nr, Nt, metric=metric)[1])
    if true_matrix.shape != (K * Nr, K * Nt):
        raise ValueError("true_matrix must be [K*Nr, K*Nt] (got %s)" % (true_matrix.shape,))
    out = np.empty(true_matrix.shape, dtype=complex)
    for k1 in range(K):
        for k2 in range(K):
            rows, cols = slice(k1 * Nr, (k1 + 1) * Nr), slice(k2 * Nt, (k2 + 1) * Nt)
            out[rows, cols] = quant_small_matrix(true_matrix[rows, cols], codebook, metric)
    return out
