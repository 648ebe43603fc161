"""NumPy restatement of the Grassmannian codebook search: the draw ledger, the chordal distances, the pair minimum and the
best candidate.  TEST INFRASTRUCTURE.

Written from the definitions (include/mcle.h) and the draw ledger of DESIGN section 4 against
oracle/philox.py; shares no code with the product.

A precoder C_k is [Nt, Ns]; Q_k an orthonormal basis of its column space by modified Gram-Schmidt with one
re-orthogonalisation pass; d^2(a, b) = Ns - sum_{s, s'} |q_{a,s}^H q_{b,s'}|^2, clamped at 0.

Ledger (mcle-philox-v1), candidate index = realization, flat entry index i = (k Nt + t) Ns + s:
    complex (0):  CN sample i of stream 2, then each precoder / its Frobenius norm
    real    (1):  sqrt(2) x the real (even i) / imaginary (odd i) part of CN sample i // 2 of stream 2, then normalised alike
    qegt    (2):  e^{j pi u_i}, u_i = uniform i of stream 3, not normalised
"""
import itertools

import numpy as np

from oracle import philox

COMPLEX, REAL, QEGT = 0, 1, 2
TYPES = {"complex": COMPLEX, "real": REAL, "qegt": QEGT}


def codebook(seed, index, K, Nt, Ns, kind, dtype=np.complex128):
    """The candidate `index` of `seed` as it is before orthonormalisation: [K, Nt, Ns]"""
    kind = TYPES.get(kind, kind)
    n = K * Nt * Ns
    if kind == COMPLEX:
        C = philox.cnormal(seed, index, n, philox.STREAM_CHAN)
    elif kind == REAL:
        z = philox.cnormal(seed, index, (n + 1) // 2, philox.STREAM_CHAN)
        C = (np.sqrt(2.0) * np.stack([z.real, z.imag], axis=-1).reshape(-1)[:n]).astype(np.complex128)
    else:
        C = np.exp(1j * np.pi * philox.uniforms(seed, index, n, philox.STREAM_PHASE))
    C = C.reshape(K, Nt, Ns)
    if kind != QEGT:
        C = C / np.sqrt(np.sum(np.abs(C) ** 2, axis=(1, 2), keepdims=True))
    return C.astype(dtype)


def codebooks(seed, first, count, K, Nt, Ns, kind, dtype=np.complex128):
    return np.stack([codebook(seed, first + r, K, Nt, Ns, kind, dtype) for r in range(count)])


def orthonormal_bases(C):
    """[..., Nt, Ns] -> Q of the same shape and dtype: modified Gram-Schmidt, every projection taken twice; the arithmetic
    stays in the dtype of C"""
    Q = np.array(C, copy=True)
    Ns = Q.shape[-1]
    for s in range(Ns):
        v = Q[..., s].copy()
        for _ in range(2):
            for j in range(s):
                q = Q[..., j]
                r = np.sum(np.conj(q) * v, axis=-1, keepdims=True)
                v = v - r * q
        nrm = np.sqrt(np.sum(v.real * v.real + v.imag * v.imag, axis=-1, keepdims=True))
        Q[..., s] = v / nrm.astype(v.real.dtype)
    return Q


def d2_matrix(C):
    """[K, Nt, Ns] -> the symmetric [K, K] float64 matrix of d^2 with a zero diagonal, the arithmetic up to |.|^2 in the
    dtype of C"""
    Q = orthonormal_bases(C)
    K, _, Ns = Q.shape
    G = np.einsum("ats,btu->absu", np.conj(Q), Q)
    w = (G.real.astype(np.float64) ** 2 + G.imag.astype(np.float64) ** 2).sum(axis=(2, 3))
    d2 = np.maximum(Ns - w, 0.0)
    d2 = np.triu(d2, 1)
    return d2 + d2.T


def pair_vector(d2):
    """the d^2 of the pairs a < b in itertools.combinations order"""
    K = d2.shape[0]
    return np.array([d2[a, b] for a, b in itertools.combinations(range(K), 2)])


def min_and_pair(d2):
    """(min d^2, (a, b)): the first smallest pair in itertools.combinations order"""
    K = d2.shape[0]
    pairs = list(itertools.combinations(range(K), 2))
    v = np.array([d2[a, b] for a, b in pairs])
    i = int(np.argmin(v))
    return float(v[i]), pairs[i]


def two_smallest_gap(d2):
    """gap between the two smallest pair d^2 (inf when there is one pair)"""
    v = np.sort(pair_vector(d2))
    return float(v[1] - v[0]) if len(v) > 1 else float("inf")


def search(seed, first, count, K, Nt, Ns, kind, dtype=np.complex128):
    """dict(min_d2 [count], pair [count, 2], gap [count] between each candidate's two smallest d^2, best_index (absolute),
    best_min_d2, best_pair, best_gap between the best and the second-best candidate)"""
    md2, pairs, gaps = np.empty(count), np.empty((count, 2), dtype=np.int32), np.empty(count)
    for r in range(count):
        d2 = d2_matrix(codebook(seed, first + r, K, Nt, Ns, kind, dtype))
        md2[r], pairs[r] = min_and_pair(d2)
        gaps[r] = two_smallest_gap(d2)
    best = -1
    for r in range(count):                       # strict >: a tie stays with the lower index
        if best < 0 or md2[r] > md2[best]:
            best = r
    out = dict(min_d2=md2, pair=pairs, gap=gaps)
    if count:
        srt = np.sort(md2)
        out.update(best_index=first + best, best_min_d2=float(md2[best]), best_pair=tuple(int(v) for v in pairs[best]),
                   best_gap=float(srt[-1] - srt[-2]) if count > 1 else float("inf"))
    return out
