"""Random search for Grassmannian codebooks with a large minimum chordal distance (the reference's apps/find_codebook.py
CodebookFinder), on the GPU.

Every candidate codebook is a pure function of (seed, candidate index) -- the draw ledger of DESIGN section 4 -- so the
search is ``Engine.run_codebook_search`` over a range of indices (csrc/kernels_codebook.hip: generate, orthonormalise,
Gram matrix on the matrix cores, pair minimum, best candidate, all in one kernel) and only the winner is ever fetched
(``Engine.codebook_generate``).  The reference's NumPy ``RandomState(prng_seed)`` stream is not replayed."""
import math
import os

import numpy as np

from . import subspace


class CodebookFinder:
    """Finds K precoders in G(Nt, Ns) by random search: the candidate whose smallest pairwise chordal distance is largest.

    ``find_codebook(rep_max)`` examines rep_max + 1 candidates, continues at the next candidate index on a later call and
    keeps the best across calls."""
    (COMPLEX, REAL, COMPLEX_QEGT) = range(3)

    def __init__(self, Nt, Ns, K, codebook_type=COMPLEX, prng_seed=None, dtype="f64", engine=None, batch_size=1 << 16):
        if not Ns < Nt:
            raise ValueError("Ns must be lower than Nt (got Ns %d, Nt %d)" % (Ns, Nt))
        if codebook_type not in (self.COMPLEX, self.REAL, self.COMPLEX_QEGT):
            raise ValueError("codebook_type must be COMPLEX, REAL or COMPLEX_QEGT (got %r)" % (codebook_type,))
        if int(batch_size) < 1:
            raise ValueError("batch_size must be positive (got %r)" % (batch_size,))
        self._Nt, self._Ns, self._K = int(Nt), int(Ns), int(K)
        self._codebook_type = codebook_type
        self._seed = int.from_bytes(os.urandom(8), "little") if prng_seed is None else int(prng_seed) & 0xFFFFFFFFFFFFFFFF
        self._dtype = dtype
        self._engine, self._own_engine = engine, False
        self._batch = int(batch_size)
        self._next = 0                 # the next candidate index
        self._best_d2 = -1.0
        self._best_index = None
        self._min_dist = 0
        self._principal_angle = 0
        self._best_C = None

    def __repr__(self):
        return "CodebookFinder: {0} {1} precoders in G({2},{3}) with minimum distance {4:.4f}".format(
            self._K, self.type, self._Nt, self._Ns, self._min_dist)

    @staticmethod
    def type_to_string(codebook_type):
        return {CodebookFinder.COMPLEX: "Complex", CodebookFinder.COMPLEX_QEGT: "Complex QEG",
                CodebookFinder.REAL: "Real"}[codebook_type]

    @staticmethod
    def calc_min_chordal_dist(codebook, engine=None, dtype=None):
        """(min_dist, principal_angles) of a codebook [K, Nt, Ns]: the smallest chordal distance over the pairs of precoders
        (the first such pair in itertools.combinations order) from the GPU operator, and that pair's principal angles."""
        codebook = np.asarray(codebook)
        own = engine is None
        if own:
            from .engine import Engine
            engine = Engine(0, "f64")
        try:
            d2, pair = engine.chordal_min_dist(codebook, dtype=dtype)
        finally:
            if own:
                engine.close()
        return math.sqrt(float(d2)), subspace.calc_principal_angles(codebook[pair[0]], codebook[pair[1]])

    def _get_engine(self):
        if self._engine is None:
            from .engine import Engine
            self._engine, self._own_engine = Engine(0, self._dtype), True
        return self._engine

    def close(self):
        """Closes the engine this finder created (one passed in is left alone)."""
        if self._own_engine and self._engine is not None:
            self._engine.close()
        if self._own_engine:
            self._engine, self._own_engine = None, False

    def find_codebook(self, rep_max=100):
        """Examines the next rep_max + 1 candidates."""
        eng = self._get_engine()
        todo = int(rep_max) + 1
        improved = None
        while todo > 0:
            n = min(todo, self._batch)
            res = eng.run_codebook_search(self._K, self._Nt, self._Ns, self._seed, self._next, n,
                                          codebook_type=self._codebook_type, dtype=self._dtype)
            if res["best_min_d2"] > self._best_d2:              # (strict: a tie stays with the lower index)
                self._best_d2, self._best_index, improved = res["best_min_d2"], res["best_index"], res["pair"]
            self._next += n
            todo -= n
        if improved is not None:
            C = eng.codebook_generate(self._K, self._Nt, self._Ns, self._seed, self._best_index, 1,
                                      codebook_type=self._codebook_type, dtype=self._dtype)[0]
            self._best_C = C
            self._min_dist = math.sqrt(self._best_d2)
            self._principal_angle = subspace.calc_principal_angles(C[improved[0]], C[improved[1]])

    @property
    def min_dist(self):
        """Minimum chordal distance between the precoders of the best codebook found."""
        return self._min_dist

    @property
    def principal_angles(self):
        """Principal angles of the closest pair of the best codebook found."""
        return self._principal_angle

    @property
    def codebook(self):
        """The best codebook found, [K, Nt, Ns]."""
        return self._best_C

    @property
    def best_index(self):
        """Candidate index of the best codebook found (None before the first search)."""
        return self._best_index

    @property
    def type(self):
        return CodebookFinder.type_to_string(self._codebook_type)


def find_codebook(Nt, Ns, K, rep_max, prng_seed=None, codebook_type=CodebookFinder.COMPLEX, dtype="f64", engine=None):
    """Creates a CodebookFinder, searches rep_max + 1 candidates and returns the codebook found."""
    cb = CodebookFinder(Nt, Ns, K, codebook_type, prng_seed, dtype=dtype, engine=engine)
    try:
        cb.find_codebook(rep_max)
    finally:
        cb.close()
    return cb.codebook
