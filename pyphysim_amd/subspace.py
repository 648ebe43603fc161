"""Subspace metrics and projections, with the reference's names and shapes (subspace/metrics.py, subspace/projections.py).

The two-matrix functions take one pair of matrices and run in host NumPy: principal angles and projections are on no hot
path.  The batched form, :func:`chordal_distances`, takes a whole codebook [K, Nt, Ns] and returns the K x K matrix of
chordal distances through the GPU operator ``Engine.chordal_min_dist`` (csrc/kernels_codebook.hip)."""
import math

import numpy as np

__all__ = ["calc_principal_angles", "calc_chordal_distance_from_principal_angles", "calc_chordal_distance",
           "calc_chordal_distance_2", "chordal_distances", "Projection", "calcProjectionMatrix",
           "calcOrthogonalProjectionMatrix"]


def _basis(matrix):
    """Orthonormal basis of the column space (the Q of a reduced QR)"""
    return np.linalg.qr(np.asarray(matrix))[0]


def calc_principal_angles(matrix1, matrix2):
    """Principal angles between the column spaces of two 2-D arrays: arccos of the singular values of Q1^H Q2 (values
    above 1 by rounding are taken as 1).  1-D array, ascending."""
    sv = np.linalg.svd(_basis(matrix1).conj().T @ _basis(matrix2), compute_uv=False)
    return np.arccos(np.minimum(sv, 1.0))


def calc_chordal_distance_from_principal_angles(principalAngles):
    """sqrt(sum_i sin^2 theta_i)"""
    return math.sqrt(float(np.sum(np.sin(np.asarray(principalAngles)) ** 2)))


def calc_chordal_distance(matrix1, matrix2):
    """Chordal distance between the column spaces of two 2-D arrays: |Q1 Q1^H - Q2 Q2^H|_F / sqrt(2)"""
    Q1, Q2 = _basis(matrix1), _basis(matrix2)
    return float(np.linalg.norm(Q1 @ Q1.conj().T - Q2 @ Q2.conj().T, "fro") / math.sqrt(2.0))


def calc_chordal_distance_2(matrix1, matrix2):
    """The same from the two projection matrices A (A^H A)^-1 A^H"""
    return float(np.linalg.norm(calcProjectionMatrix(matrix1) - calcProjectionMatrix(matrix2), "fro") / math.sqrt(2.0))


def chordal_distances(codebook, engine=None, dtype=None):
    """K x K matrix of the chordal distances between the K precoders of `codebook` [K, Nt, Ns] (zero diagonal), on the GPU.
    engine: an :class:`~pyphysim_amd.engine.Engine` (one on device 0 is created and closed when None)."""
    own = engine is None
    if own:
        from .engine import Engine
        engine = Engine(0, "f64")
    try:
        _, _, d2 = engine.chordal_min_dist(np.asarray(codebook), dtype=dtype, full=True)
    finally:
        if own:
            engine.close()
    return np.sqrt(d2)


class Projection:
    """Projection, orthogonal projection and reflection with respect to the subspace spanned by the columns of A."""

    def __init__(self, A):
        self._A = np.asarray(A)
        self.Q = Projection.calcProjectionMatrix(self._A)
        self.oQ = Projection.calcOrthogonalProjectionMatrix(self._A)

    def project(self, M):
        """Projection of M (vector or matrix) into the subspace"""
        return self.Q @ np.asarray(M)

    def oProject(self, M):
        """Projection of M into the orthogonal complement of the subspace"""
        return self.oQ @ np.asarray(M)

    def reflect(self, M):
        """(I - 2 Q) M, as the reference defines the reflection"""
        return (np.eye(self.Q.shape[0]) - 2.0 * self.Q) @ np.asarray(M)

    @staticmethod
    def calcProjectionMatrix(A):
        """A (A^H A)^-1 A^H"""
        A = np.asarray(A)
        Ah = A.conj().T
        return (A @ np.linalg.inv(Ah @ A)) @ Ah

    @staticmethod
    def calcOrthogonalProjectionMatrix(A):
        """I - A (A^H A)^-1 A^H"""
        Q = Projection.calcProjectionMatrix(A)
        return np.eye(Q.shape[0]) - Q


calcProjectionMatrix = Projection.calcProjectionMatrix
calcOrthogonalProjectionMatrix = Projection.calcOrthogonalProjectionMatrix
