"""Uplink reference signals: Zadoff-Chu root sequences and the SRS / DMRS sequences of one user.

The public names, signatures, properties and error types are those of the reference's
``reference_signals`` package, so code written against it runs unchanged; the implementation is
this project's own, from the defining formulas:

    Zadoff-Chu root     a_u[n] = exp(-j pi u n (n + 1 + 2 q) / Nzc),        n = 0 .. Nzc-1
    cyclic extension    x[n]   = a_u[n mod Nzc],                            n = 0 .. size-1
    cyclic shift        r[n]   = exp(j 2 pi n_cs n / D) x[n],               D = 8 (SRS), 12 (DMRS)
    cover code          r_c[n] = w_c r[n]                                   (DMRS, one row per slot)

All of this is host code: a sequence is built once per scenario.  The per-realization arithmetic
that uses it -- the channel estimators -- runs on the GPU (:mod:`pyphysim_amd.channel_estimation`).

Not provided: base sequences of 12 and 24 elements (one and two resource blocks).  The standard
defines those by phi(n) tables, not by a formula, and the tables are not part of this package:
``RootSequence`` raises ``ValueError`` for ``size <= 24``.  "Largest prime <= size" comes from a
sieve, so it is right for every size (the reference looks it up in a list that ends at 1009).
"""
import numpy as np

__all__ = ["calcBaseZC", "get_shifted_root_seq", "get_extended_ZF", "get_srs_seq", "get_dmrs_seq", "RootSequence",
           "UeSequence", "SrsUeSequence", "DmrsUeSequence"]

SRS_SHIFTS, DMRS_SHIFTS = 8, 12
MIN_ZC_SIZE = 25          # below: the table-defined base sequences


def calcBaseZC(Nzc, u, q=0):
    """Zadoff-Chu root sequence of length `Nzc` and root index `u` (0 < u < Nzc for the CAZAC property)."""
    if not u < Nzc:
        raise AssertionError("the root index must be lower than the sequence length (u = %r, Nzc = %r)" % (u, Nzc))
    n = np.arange(Nzc)
    # The phase reaches ~10^4 rad already at Nzc = 139, where one rounding is ~2e-12 rad, so its association decides whether
    # the reference's own numbers (tests/golden/g1_chanest.npz) are met to 1e-12: products left to right, then times the
    # reciprocal of Nzc (what NumPy's complex division by a real does) reproduces them; dividing by Nzc instead is off by
    # 1.8e-12, and the exact form (u n (n + 1) reduced mod 2 Nzc in integers first) by 2.6e-12.
    phase = np.pi * u * n * (n + 1 + 2 * q) * (1.0 / Nzc)
    return np.cos(phase) - 1j * np.sin(phase)


def get_shifted_root_seq(root_seq, n_cs, denominator):
    """`root_seq` with cyclic shift `n_cs` out of `denominator` (a phase ramp of n_cs / denominator turns per element)."""
    if not -denominator < n_cs < denominator:
        raise AssertionError("cyclic shift %r outside (-%d, %d)" % (n_cs, denominator, denominator))
    root_seq = np.asarray(root_seq)
    ramp = np.exp(2j * np.pi * (n_cs / denominator) * np.arange(root_seq.size))
    return ramp * root_seq


def get_extended_ZF(root_seq, size):
    """`root_seq` repeated cyclically up to `size` elements."""
    root_seq = np.asarray(root_seq)
    return np.resize(root_seq, size)


def get_srs_seq(root_seq, n_cs):
    """SRS sequence of the user with cyclic shift `n_cs` (0 .. 7)."""
    return get_shifted_root_seq(root_seq, n_cs, SRS_SHIFTS)


def get_dmrs_seq(root_seq, n_cs):
    """DMRS sequence of the user with cyclic shift `n_cs` (0 .. 11)."""
    return get_shifted_root_seq(root_seq, n_cs, DMRS_SHIFTS)


def largest_prime_not_above(n):
    """Largest prime <= n by the sieve of Eratosthenes; ValueError below 2."""
    n = int(n)
    if n < 2:
        raise ValueError("there is no prime <= %d" % n)
    is_prime = np.ones(n + 1, dtype=bool)
    is_prime[:2] = False
    for p in range(2, int(n ** 0.5) + 1):
        if is_prime[p]:
            is_prime[p * p::p] = False
    return int(np.flatnonzero(is_prime)[-1])


class _ArrayLike:
    """Arithmetic and indexing of a sequence object act on its array (`seq_array()`), and give arrays."""

    def seq_array(self):
        raise NotImplementedError

    def __getitem__(self, index):
        return self.seq_array()[index]

    def __add__(self, other):
        return self.seq_array() + other

    def __mul__(self, other):
        return self.seq_array() * other

    __radd__, __rmul__ = __add__, __mul__

    def conj(self):
        return np.conj(self.seq_array())

    conjugate = conj


class RootSequence(_ArrayLike):
    """The root sequence of a cell: Zadoff-Chu of length `Nzc`, cyclically extended to `size`.

    root_index: u.  size: elements wanted (default: Nzc).  Nzc: Zadoff-Chu length (default: the largest
    prime <= size).  AttributeError when neither length is given or size < Nzc; ValueError for size <= 24
    (see the module docstring).
    """

    def __init__(self, root_index, size=None, Nzc=None):
        if size is None:
            if Nzc is None:
                raise AttributeError("RootSequence needs 'size', 'Nzc' or both")
            size = Nzc
        size = int(size)
        if size < MIN_ZC_SIZE:
            raise ValueError("a root sequence of %d elements is one of the standard's phi(n) table sequences, which this "
                             "package does not carry (sizes >= %d are Zadoff-Chu)" % (size, MIN_ZC_SIZE))
        zc_len = largest_prime_not_above(size) if Nzc is None else int(Nzc)
        if zc_len > size:
            raise AttributeError("'size' (%d) cannot be smaller than 'Nzc' (%d)" % (size, zc_len))
        self._u = root_index
        self._zc_len = zc_len
        self._seq = get_extended_ZF(calcBaseZC(zc_len, root_index), size)

    @property
    def Nzc(self):
        """Length of the Zadoff-Chu sequence before extension."""
        return self._zc_len

    @property
    def size(self):
        """Number of elements, extension included."""
        return int(self._seq.size)

    @property
    def index(self):
        """The root index u."""
        return self._u

    def seq_array(self):
        """The sequence as a complex128 array."""
        return self._seq

    def __repr__(self):
        return "RootSequence(root_index=%r, size=%d, Nzc=%d)" % (self._u, self.size, self._zc_len)


class UeSequence(_ArrayLike):
    """Reference sequence of one user; base of :class:`SrsUeSequence` and :class:`DmrsUeSequence`.

    user_seq_array is [Ne], or [Nc, Ne] with a cover code (one row per slot).  normalize=True scales it so that
    one row has unit Euclidean norm.
    """

    def __init__(self, root_seq, n_cs, user_seq_array, normalize=False):
        seq = np.asarray(user_seq_array)
        self._normalized = normalize
        if normalize is True:
            seq = seq / np.sqrt(np.sum(np.abs(seq.reshape(-1, seq.shape[-1])[0]) ** 2))
        self._seq = seq
        self._shift = n_cs
        self._u = root_seq.index

    @property
    def normalized(self):
        """Whether the sequence was scaled to unit norm."""
        return self._normalized

    @property
    def size(self):
        """Number of sequence elements Ne (a cover code does not count)."""
        return int(self._seq.shape[-1])

    @property
    def shape(self):
        return self._seq.shape

    def seq_array(self):
        """The sequence as a complex128 array."""
        return self._seq

    def __repr__(self):
        return "%s(root_index=%r, n_cs=%r)" % (type(self).__name__, self._u, self._shift)


class SrsUeSequence(UeSequence):
    """Sounding reference signal of the user with cyclic shift `n_cs` (0 .. 7) of `root_seq`."""

    def __init__(self, root_seq, n_cs, normalize=False):
        super().__init__(root_seq, n_cs, get_srs_seq(root_seq.seq_array(), n_cs), normalize=normalize)


class DmrsUeSequence(UeSequence):
    """Demodulation reference signal of the user with cyclic shift `n_cs` (0 .. 11) of `root_seq`.

    cover_code (optional, e.g. ``np.array([1, -1])``): the user sends the sequence in len(cover_code) slots, slot c
    multiplied by cover_code[c]; `seq_array()` is then [Nc, Ne].
    """

    def __init__(self, root_seq, n_cs, cover_code=None, normalize=False):
        seq = get_dmrs_seq(root_seq.seq_array(), n_cs)
        if cover_code is not None:
            if not isinstance(cover_code, np.ndarray):
                raise AssertionError("cover_code must be a NumPy array")
            cover_code.setflags(write=False)          # the object keeps the caller's array
            seq = np.multiply.outer(cover_code, seq)
        self._cover = cover_code
        super().__init__(root_seq, n_cs, seq, normalize=normalize)

    @property
    def cover_code(self):
        """The cover code, or None."""
        return self._cover

    def __repr__(self):
        return "%s(root_index=%r, n_cs=%r, cover_code=%r)" % (type(self).__name__, self._u, self._shift, self._cover)
