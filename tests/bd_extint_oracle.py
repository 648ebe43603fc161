"""50-digit reference of block diagonalisation with external interference (WhiteningBD / EnhancedBD, mcle_bd_extint) and the
input classes it is tested on.  TEST INFRASTRUCTURE; follows tests/mimo_ops_oracle.py.  It does not import pyphysim_amd.

Plain mpmath at mp.dps = 50 restates, per user k of one channel big_H = [H | H_ext] ([K r, K r + n_ext]):
    Re_k = pe H_ext,k H_ext,k^H + nv I, its eigen-decomposition (ascending), Wf_k = diag(L^-1/2) V^H, Re_k^-1,
    P_k  = I - A^H (A A^H)^-1 A, the projector on the null space of the other users' rows A,
    EnhancedBD's reduction exactly as oracle/bd.py::enhanced_bd states it, on a GIVEN Ms_bad (reduce()): Pk (identity for
    'naive' and for ns == r unless 'fixed'), the norm term, Heq_red, Pbar = Pk Pk^H, W = pinv(Pbar Heq_red) Pbar,
    _calc_linear_SINRs (linear_sinrs()), the first maximum of sum log2(1 + sinr) (first_max()).
Results leave as np.clongdouble / np.longdouble; the predicates below run in long double on them, so that an error of a few
eps of complex128 is measured and not the predicate's own rounding.  Every predicate returns {name: (error, scale)}.

What is unique and what is not.  Ms_bad has a phase per column, V a phase per column: so solutions are compared through
Ms Ms^H, W^H W and |W H_k Ms|, as tests/test_gpu_bd_extint.py does.  The whitening filter Wf_k is unique only up to a
rotation inside an eigenspace of Re_k, but Wf_k^H Wf_k = Re_k^-1 always is, and the whitening predicates are written with
Re_k^-1: the Gram matrix of E_w = Wf_k H_k Ms_k is E^H Re_k^-1 E with E = H_k Ms_k.  A stream cut V[:, :ns] is unique when
lambda_ns < lambda_{ns+1} (cut_kind() == "unique": relative gap >= GAP) and arbitrary inside the eigenspace when the two are
equal ("degenerate": relative gap <= TIE).  In between lies only the class `ext_weak`, by construction: pe H_ext H_ext^H is 1e-6
of nv I there, so every gap is 7e-9 .. 1e-6 of lambda_max ("between") while being >= 1e-3 of the interference's own largest
eigenvalue; those cuts ARE compared with the 50-digit solution, at a scale that carries lambda_max / gap (cut_factor(), up to
1.4e8: PM and PW of such a cut are held to about 1e-7, which is what complex128 can give for an eigenvector of that gap).
tests/test_bd_extint_oracle_cpu.py asserts all of this.  The SINRs of a cut additionally need every eigenvalue below the cut
simple (sinr_unique()).  Degenerate cuts, and only they, are held to the properties of properties() instead of to a 50-digit
solution.

Scales come from the 50-digit quantities: exact_norms() gives ||W_k||_F and its whitened counterpart from P_k, Re_k and H_k
alone (||W||_F^2 = tr((H_k Ms_k Ms_k^H H_k^H)^-1) with Ms_k Ms_k^H = iPu / r P_k).  Only properties() and the `sinr5` check, which
by their nature have no 50-digit solution to take norms from, use the norms of the solution under test.

Input classes (cases()): PER_CLASS seeded channels per (class, K, r), their n_ext cycling over the class's share of
{0, 1, r - 1, r, 8}; Haar factors at 50 digits, rounded once.  A GPU batch is one parameter group tiled to BATCH = 70."""
import collections
import functools
import math

import mpmath as mp
import numpy as np

from mimo_ops_oracle import BATCH, EPS, FACTOR, _H, _from_spectrum, _rayleigh, bound, to_ld, to_mp   # noqa: F401
from oracle import bd as obd

mp.mp.dps = 50

PER_CLASS = 6
GEOMETRIES = ((1, 1), (1, 2), (1, 3), (1, 4), (2, 1), (2, 2), (2, 3), (2, 4), (3, 1), (3, 2), (4, 1), (4, 2))   # (K, r)
CLASSES = ("rayleigh", "graded", "ext_lowrank", "ext_strong", "ext_weak", "scaled", "pe_zero", "nv_zero", "singular",
           "ext_dependent")
GRADED_CONDS = (1e2, 1e4, 1e6, 1e8)
GAP, TIE = 1e-3, 1e-13
IPU, NV, PE = 1.75, 0.05, 0.8
EPS64 = EPS["f64"]

Case = collections.namedtuple("Case", "big_H K r n_ext iPu nv pe")


def n_ext_values(r):
    return sorted({0, 1, r - 1, r, 8})


def class_n_ext(cls, r):
    """The class's share of n_ext_values(r); empty: the class does not exist at this r."""
    v = n_ext_values(r)
    if cls == "ext_lowrank":                    # rank(H_ext,k) = 1 < min(r, n_ext), r >= 3
        return [e for e in v if e >= 2] if r >= 3 else []
    if cls in ("ext_strong", "ext_weak"):
        return [e for e in v if e >= 1]
    if cls == "ext_dependent":                  # n_ext = r, two equal external columns
        return [r] if r >= 2 else []
    return v


def pairs():
    """Every (K, r, class) that exists."""
    return [(K, r, c) for (K, r) in GEOMETRIES for c in CLASSES
            if class_n_ext(c, r) and not (c == "singular" and K * r < 2)]


@functools.lru_cache(maxsize=None)
def cases(cls, K, r):
    """-> tuple of PER_CLASS Case.  (class, geometry) seeds were chosen so that tests/test_bd_extint_oracle_cpu.py's
    conditions hold (gaps at the cuts, capacity margins)."""
    n = K * r
    rs = np.random.RandomState(7100 + 131 * CLASSES.index(cls) + 10 * K + r)
    share = class_n_ext(cls, r)
    out = []
    for i in range(PER_CLASS):
        e = share[i % len(share)]
        iPu, nv, pe = IPU, NV, PE
        H = _rayleigh(rs, n, n)
        X = _rayleigh(rs, n, e)
        if cls == "graded":
            kappa = GRADED_CONDS[i % len(GRADED_CONDS)] if n > 1 else 1.0
            H = _from_spectrum(rs, n, n, tuple(kappa ** (-j / max(n - 1, 1)) for j in range(n)))
        elif cls == "ext_lowrank":
            X = np.vstack([_rayleigh(rs, r, 1) @ _rayleigh(rs, 1, e) for _ in range(K)])
        elif cls in ("ext_strong", "ext_weak"):     # pe ||H_ext,k||_F^2 = 1e6 nv or 1e-6 nv, for every user
            for k in range(K):
                blk = X[k * r:(k + 1) * r]
                blk *= math.sqrt((1e6 if cls == "ext_strong" else 1e-6) * nv / (pe * float(np.sum(np.abs(blk) ** 2))))
        elif cls == "pe_zero":
            pe = 0.0
        elif cls == "nv_zero":
            nv = 0.0
            if i == PER_CLASS - 1:                  # nv = pe = 0: no interference and no noise at all
                pe = 0.0
        elif cls == "singular":
            H[n - 1] = H[0]
        elif cls == "ext_dependent":
            nv = 0.0
            X[:, e - 1] = X[:, 0]
        big = np.hstack([H, X])
        if cls == "scaled":                         # the CoMP link's path-loss regime
            big = big * 2.0 ** -40
            nv = nv * 2.0 ** -80
        big = np.ascontiguousarray(big, dtype=np.complex128)
        big.setflags(write=False)
        out.append(Case(big, K, r, e, iPu, nv, pe))
    return tuple(out)


def groups(cls, K, r):
    """The cases of one (class, geometry) by call parameters -> {(n_ext, iPu, nv, pe): [case index, ...]}."""
    g = collections.OrderedDict()
    for i, c in enumerate(cases(cls, K, r)):
        g.setdefault((c.n_ext, c.iPu, c.nv, c.pe), []).append(i)
    return g


def tiled(cs):
    """[Case, ...] of one group -> big_H [BATCH, n, n + n_ext]: row b is case b % len(cs)."""
    return np.ascontiguousarray(np.stack([cs[b % len(cs)].big_H for b in range(BATCH)]))


# ---- 50 digits -----------------------------------------------------------------------------------------------------
def _sub(M, r0, r1, c0, c1):
    out = mp.matrix(r1 - r0, c1 - c0)
    for i in range(r0, r1):
        for j in range(c0, c1):
            out[i - r0, j - c0] = M[i, j]
    return out


def _eigh_sorted(R):
    E, Q = mp.eigh(R)
    order = sorted(range(len(E)), key=lambda i: E[i])
    V = mp.matrix(Q.rows, Q.cols)
    for c, o in enumerate(order):
        for i in range(Q.rows):
            V[i, c] = Q[i, o]
    return [E[o] for o in order], V


def _rank(M):
    """Numerical rank of a matrix that was rounded to complex128 once (a product a b^H is rank 1 to about 1e-16)."""
    if M.cols == 0 or M.rows == 0:
        return 0
    S = mp.svd_c(M, compute_uv=False)
    return sum(1 for i in range(len(S)) if S[i] > S[0] * mp.mpf(10) ** -12) if S[0] > 0 else 0


@functools.lru_cache(maxsize=None)
def _exact_cached(cls, K, r, i):
    return exact(cases(cls, K, r)[i])


def exact(c):
    """The 50-digit quantities of one Case.  mp matrices per user in "mp" (H, Hk, Hext, Re, lam, V), long double arrays
    per user: Re, lam, V, Wf (None when Re_k is singular), Rinv (None likewise), P; ext_rank and gap (relative gaps
    (lam_{j+1} - lam_j) / lam_max at the cuts j = 1 .. r - 1; all zero when Re_k = 0)."""
    K, r, n = c.K, c.r, c.K * c.r
    big = to_mp(c.big_H) if c.big_H.shape[1] > 0 else mp.matrix(n, 0)
    Hm = _sub(big, 0, n, 0, n)
    out = dict(H=np.asarray(c.big_H[:, :n]), Hext=[np.asarray(c.big_H[k * r:(k + 1) * r, n:]) for k in range(K)],
               Re=[], lam=[], V=[], Wf=[], Rinv=[], P=[], ext_rank=[], gap=[], mp=[])
    for k in range(K):
        Hk = _sub(Hm, k * r, (k + 1) * r, 0, n)
        X = _sub(big, k * r, (k + 1) * r, n, n + c.n_ext) if c.n_ext else mp.matrix(r, 0)
        Re = mp.mpf(c.nv) * mp.eye(r)
        if c.n_ext:
            Re = Re + mp.mpf(c.pe) * (X * _H(X))
        lam, V = _eigh_sorted(Re)
        top = lam[-1]
        if lam[0] > top * mp.mpf(10) ** -30 and top > 0:
            Wf = mp.matrix(r, r)
            Vh = _H(V)
            for i in range(r):
                for j in range(r):
                    Wf[i, j] = Vh[i, j] / mp.sqrt(lam[i])
            Wf_ld, Rinv_ld = to_ld(Wf), to_ld(mp.inverse(Re))
        else:
            Wf_ld = Rinv_ld = None
        if K > 1:
            A = mp.matrix(n - r, n)
            rows = [i for i in range(n) if not k * r <= i < (k + 1) * r]
            for a, i in enumerate(rows):
                for j in range(n):
                    A[a, j] = Hm[i, j]
            G = A * _H(A)
            try:
                P = mp.eye(n) - _H(A) * mp.inverse(G) * A
            except ZeroDivisionError:               # two equal rows: the class `singular`
                P = None
        else:
            P = mp.eye(n)
        out["mp"].append(dict(Hk=Hk, Re=Re, lam=lam, V=V))
        out["Re"].append(to_ld(Re))
        out["lam"].append(to_ld(lam))
        out["V"].append(to_ld(V))
        out["Wf"].append(Wf_ld)
        out["Rinv"].append(Rinv_ld)
        out["P"].append(None if P is None else to_ld(P))
        out["ext_rank"].append(_rank(X) if c.pe > 0 else 0)
        out["gap"].append([float((lam[j] - lam[j - 1]) / top) if top > 0 else 0.0 for j in range(1, r)])
    return out


def cut_kind(ex, k, ns):
    """"unique" / "degenerate" / "between" for the cut V[:, :ns] of user k (ns == r cuts nothing: unique)."""
    gaps = ex["gap"][k]
    if ns > len(gaps):
        return "unique"
    g = gaps[ns - 1]
    return "unique" if g >= GAP else ("degenerate" if g <= TIE else "between")


def sinr_unique(ex, k, ns, r):
    """The SINRs of the capacity-rule candidate with ns streams are unique: identity Pk (ns == r), or every eigenvalue up to
    the cut simple ("unique" or, in `ext_weak`, "between": simple, with a gap of 7e-9 .. 1e-6 of lambda_max that the
    comparison's scale carries through cut_factor())."""
    return ns == r or all(cut_kind(ex, k, j) != "degenerate" for j in range(1, ns + 1))


def linear_sinrs(Hred, W, Re):
    """EnhancedBD._calc_linear_SINRs (oracle/bd.py::ebd_linear_sinrs) at 50 digits -> list of mpf."""
    M = W * Hred
    D = W * Re * _H(W)
    out = []
    for i in range(M.rows):
        desired = abs(M[i, i]) ** 2
        internal = mp.fsum([abs(M[i, j]) ** 2 for j in range(M.cols) if j != i])
        den = internal + abs(mp.re(D[i, i]))
        out.append(mp.inf if den == 0 else desired / den)
    return out


def reduce(c, ex, k, Msk, rule, ns):
    """One candidate of oracle/bd.py::enhanced_bd (lines 272-288) at 50 digits on the given unit-norm directions
    Msk [n, r] of user k.  rule: 'naive' (identity columns), 'fixed' (V[:, :ns]), 'auto' (the capacity / candidates /
    per-user rule: V[:, :ns] for ns < r, identity for ns == r).  -> (MsPk [n, ns], W [ns, r], sinrs) in mp."""
    r = c.r
    m = ex["mp"][k]
    Mm = to_mp(Msk)
    if rule == "naive" or (rule == "auto" and ns == r):
        Pk = _sub(mp.eye(r), 0, r, 0, ns)
    else:
        Pk = _sub(m["V"], 0, r, 0, ns)
    MsPk = Mm * Pk
    norm_term = mp.sqrt(mp.fsum([abs(MsPk[i, j]) ** 2 for i in range(MsPk.rows) for j in range(ns)])) / mp.sqrt(mp.mpf(c.iPu))
    MsPk = MsPk / norm_term
    Hred = (m["Hk"] * Mm) * Pk / norm_term
    Pbar = Pk * _H(Pk)
    A = Pbar * Hred                                         # r x ns, full column rank
    W = mp.inverse(_H(A) * A) * _H(A) * Pbar
    return MsPk, W, linear_sinrs(Hred, W, m["Re"])


def first_max(rows):
    """np.argmax of sum log2(1 + sinr) over the candidates -> (index of the first maximum, the values as mpf)."""
    vals = [mp.inf if any(s == mp.inf for s in row) else mp.fsum([mp.log(1 + s, 2) for s in row]) for row in rows]
    best = 0
    for i, v in enumerate(vals):
        if v > vals[best]:
            best = i
    return best, vals


def capacity_margin(vals):
    """Relative distance of the best capacity value to the second best (inf: a single candidate)."""
    s = sorted(vals, reverse=True)
    if len(s) < 2:
        return float("inf")
    if s[0] == mp.inf:
        return float("inf") if s[1] != mp.inf else 0.0
    return float((s[0] - s[1]) / s[0])


# ---- long double predicates ----------------------------------------------------------------------------------------
LD = np.clongdouble


def ld(a):
    return np.asarray(a).astype(LD)


def _amax(a):
    a = np.asarray(a)
    if a.size == 0:
        return 0.0
    v = float(np.max(np.abs(a)))
    return v if np.isfinite(v) else float("inf")


def ld_inv(A):
    """Inverse of a small matrix in long double (Gauss-Jordan, partial pivoting); numpy.linalg has no long double."""
    A = ld(A).copy()
    n = A.shape[0]
    B = np.eye(n, dtype=LD)
    for c in range(n):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        if p != c:
            A[[c, p]] = A[[p, c]]
            B[[c, p]] = B[[p, c]]
        piv = A[c, c]
        A[c] = A[c] / piv
        B[c] = B[c] / piv
        for i in range(n):
            if i != c:
                f = A[i, c]
                A[i] = A[i] - f * A[c]
                B[i] = B[i] - f * B[c]
    return B


def _amp(Hk, M, W):
    """||W||_F ||H_k||_F ||M||_F >= about 1: how far W (H_k M) moves per relative eps of M when H_k M is a cancelled
    product (an ill-conditioned channel); the scale of every 'W H_k M = I' kind of predicate."""
    f = lambda A: float(np.sqrt(np.sum(np.abs(A) ** 2)))
    v = f(W) * f(Hk) * f(M)
    return max(1.0, v) if np.isfinite(v) else 1.0


def exact_norms(c, ex, k):
    """From the 50-digit quantities alone, for the full-stream solutions (metric None, whitening) of user k:
    (||W_k||_F, amp, whitened amp).  W_k = (H_k Ms_k)^-1 and Ms_k Ms_k^H = iPu / r P_k whatever the column phases, so
    ||W_k||_F^2 = tr(S^-1) with S = iPu / r H_k P_k H_k^H; amp = ||W_k||_F ||H_k||_F ||Ms_k||_F (_amp()).  WhiteningBD forms
    W_k = pinv(Wf H_k Ms_k) Wf, a product whose first factor's loss is carried by the second: its amplification is
    ||pinv(Wf H_k Ms_k)||_F ||Wf||_F ||H_k||_F ||Ms_k||_F >= amp (the Frobenius norm is submultiplicative), with
    ||pinv(Wf H_k Ms_k)||_F^2 = tr((Wf S Wf^H)^-1) and ||Wf||_F^2 = tr(Re^-1): the same for every valid Wf."""
    r = c.r
    Hk = ld(ex["H"])[k * r:(k + 1) * r]
    S = Hk @ (ex["P"][k] * np.longdouble(c.iPu / r)) @ Hk.conj().T
    f = lambda A: float(np.sqrt(np.sum(np.abs(A) ** 2)))
    wn = math.sqrt(max(float(np.real(np.trace(ld_inv(S)))), 0.0))
    base = f(Hk) * math.sqrt(c.iPu)
    amp_w = None
    if ex["Wf"][k] is not None:
        Wf = ex["Wf"][k]
        pn = math.sqrt(max(float(np.real(np.trace(ld_inv(Wf @ S @ Wf.conj().T)))), 0.0))
        amp_w = max(1.0, pn * math.sqrt(float(np.real(np.trace(ex["Rinv"][k])))) * base)
    return wn, max(1.0, wn * base), amp_w


def _offdiag(G):
    return G - np.diag(np.diag(G))


def bd_validity(c, ex, k, Msk):
    """Predicates of unit-norm BD directions Msk [n, r] of user k.  Also "order": 0 when the column norms of E_k = H_k Msk
    ascend (the kernel's order, sigma ascending) else 1, and "phase_sign": 0 when each column's largest entry is positive."""
    K, r, n = c.K, c.r, c.K * c.r
    H, M = ld(ex["H"]), ld(Msk)
    out = {}
    leak, hs = 0.0, 0.0
    for l in range(K):
        if l != k:
            Hl = H[l * r:(l + 1) * r]
            leak = max(leak, _amax(Hl @ M))
            hs = max(hs, float(np.sqrt(np.max(np.sum(np.abs(Hl) ** 2, axis=1)))))
    out["leak"] = (leak, hs)
    out["orth"] = (_amax(M.conj().T @ M - np.eye(r)), 1.0)
    if ex["P"][k] is not None:
        out["proj"] = (_amax(M @ M.conj().T - ex["P"][k]), 1.0)
    E = H[k * r:(k + 1) * r] @ M
    G = E.conj().T @ E
    d = np.real(np.diag(G))
    hm = float(np.sum(np.abs(H[k * r:(k + 1) * r]) ** 2)) * r            # ||H_k||_F^2 ||Msk||_F^2, unit-norm columns
    out["gram"] = (_amax(_offdiag(G)), max(float(np.max(d)), hm))     # an eps of Msk moves E by eps ||H_k|| ||Msk||
    out["order"] = (0.0 if np.all(np.diff(d) >= 0) else 1.0, 0.0)
    piv = np.array([M[int(np.argmax(np.abs(np.asarray(Msk)[:, j]))), j] for j in range(r)])
    out["phase"] = (_amax(piv.imag), 1.0)
    out["phase_sign"] = (0.0 if np.all(piv.real > 0) else 1.0, 0.0)
    return out


def whitening_checks(c, ex, k, Msk, Wk):
    """Predicates of a WhiteningBD solution of user k (Msk [n, r] with ||Msk||_F^2 = iPu, Wk [r, r]), written with
    Re_k^-1 = Wf_k^H Wf_k: the Gram matrix of E_w = Wf_k H_k Ms_k, E^H Re^-1 E, is diagonal and ascends; W Re W^H is its
    inverse (so diagonal); W H_k Ms_k = I."""
    r = c.r
    H, M, W = ld(ex["H"]), ld(Msk), ld(Wk)
    E = H[k * r:(k + 1) * r] @ M
    Gw = E.conj().T @ ex["Rinv"][k] @ E
    d = np.real(np.diag(Gw))
    T = ld_inv(Gw)
    D = W @ ex["Re"][k] @ W.conj().T
    hm = float(np.sum(np.abs(H[k * r:(k + 1) * r]) ** 2)) * c.iPu * _amax(ex["Rinv"][k])      # ||Msk||_F^2 = iPu
    wn, _, amp = exact_norms(c, ex, k)                      # scales from the 50 digits: |W Re W^H| <= ||W||_F^2 ||Re||_F
    cov = wn ** 2 * float(np.sqrt(np.sum(np.abs(ex["Re"][k]) ** 2)))
    return {"wgram": (_amax(_offdiag(Gw)), max(float(np.max(d)), hm)),
            "worder": (0.0 if np.all(np.diff(d) >= 0) else 1.0, 0.0),
            "wcov": (_amax(D - T), cov * amp),
            "wcov_diag": (_amax(_offdiag(D)), cov * amp),
            "wid": (_amax(W @ E - np.eye(r)), amp)}


def scaled_validity(c, ex, k, Msk):
    """BD validity of a full-stream solution whose columns all have norm sqrt(iPu / r) (whitening: without the order of
    E's Gram matrix, which is that of the whitened channel; metric None: with it)."""
    return bd_validity(c, ex, k, np.asarray(Msk) / math.sqrt(c.iPu / c.r))


def inverse_checks(c, ex, k, Msk, Wk):
    """Metric None: W_k = (H_k Ms_k)^-1."""
    r = c.r
    Hk = ld(ex["H"])[k * r:(k + 1) * r]
    E = Hk @ ld(Msk)
    T = ld_inv(E)
    wn, amp, _ = exact_norms(c, ex, k)
    return {"winv": (_amax(ld(Wk) - T), wn * amp), "wid": (_amax(ld(Wk) @ E - np.eye(r)), amp)}


def invariants(ex, k, r, MsPk, W):
    """The phase-free invariants of a (reduced) solution in long double: Ms Ms^H, W^H W, |W H_k Ms|."""
    M, Wl = ld(MsPk), ld(W)
    Hk = ld(ex["H"])[k * r:(k + 1) * r]
    return M @ M.conj().T, Wl.conj().T @ Wl, np.abs(Wl @ Hk @ M)


def cut_factor(ex, k, ns, r, upto=False):
    """lambda_max / (lambda_{ns+1} - lambda_ns) >= 1: how far span(V[:, :ns]) turns per relative eps of Re_k (the
    conditioning of an invariant subspace is the reciprocal of its gap); `upto`: the smallest gap of the cuts 1 .. ns, which
    is what the single eigenvectors below the cut, and so the per-stream SINRs, feel.  1 where nothing is cut."""
    gaps = ex["gap"][k][(0 if upto else ns - 1):ns]
    gaps = [g for g in gaps if g > 0]
    return max(1.0, 1.0 / min(gaps)) if gaps and ns < r + (1 if upto else 0) else 1.0


def invariant_errors(ex, k, r, got, want, factor=1.0):
    """got, want: (MsPk, W) pairs -> {"PM", "PW", "EQ"}: (error, scale).  Scales: the largest entry of the exact invariant,
    times `factor` (cut_factor() for a solution cut along V, else 1) for PM and PW, which move with the cut, and times
    _amp() for PW and EQ, which move with W (EQ = |W H_k MsPk| = I for whatever cut)."""
    a, b = invariants(ex, k, r, *got), invariants(ex, k, r, *want)
    amp = _amp(ld(ex["H"])[k * r:(k + 1) * r], ld(want[0]), ld(want[1]))
    scale = {"PM": factor, "PW": factor * amp, "EQ": amp}
    return {name: (_amax(x - y), _amax(y) * scale[name]) for name, x, y in zip(("PM", "PW", "EQ"), a, b)}


def properties(c, ex, k, Msb_k, MsPk, W, ns, cut=True):
    """What holds for every valid answer of a reduced solution (MsPk [n, ns], W [ns, r]) whichever basis a repeated
    eigenvalue's space was given: W H_k MsPk = I, ||MsPk||_F^2 = iPu, H_l MsPk = 0, the columns of MsPk lie in
    span(Ms_bad,k), and -- for a cut V[:, :ns] (`cut`), not for identity columns -- W H_ext,k = 0 when
    ns <= r - rank(H_ext,k) and pe > 0."""
    K, r = c.K, c.r
    H, M, Wl, B = ld(ex["H"]), ld(MsPk), ld(W), ld(Msb_k)
    out = {"p_id": (_amax(Wl @ H[k * r:(k + 1) * r] @ M - np.eye(ns)), _amp(H[k * r:(k + 1) * r], M, Wl)),
           "p_pow": (abs(float(np.sum(np.abs(M) ** 2)) - c.iPu), c.iPu)}
    leak, hs = 0.0, 0.0
    for l in range(K):
        if l != k:
            leak = max(leak, _amax(H[l * r:(l + 1) * r] @ M))
            hs = max(hs, float(np.sqrt(np.max(np.sum(np.abs(H[l * r:(l + 1) * r]) ** 2, axis=1)))))
    out["p_leak"] = (leak, hs * math.sqrt(c.iPu))
    out["p_span"] = (_amax(M - B @ (B.conj().T @ M)), math.sqrt(c.iPu))
    if cut and c.pe > 0 and c.n_ext and ns <= r - ex["ext_rank"][k]:
        # the rows of W lie in span(V[:, :ns]), inside the noise eigenspace; that space turns towards H_ext,k by
        # eps lambda_max / (lambda_interference,min - lambda_noise) per relative eps of Re_k (1e6 eps in `ext_weak`)
        X = ld(ex["Hext"][k])
        lam = [float(v) for v in ex["lam"][k]]
        turn = max(1.0, lam[-1] / (lam[r - ex["ext_rank"][k]] - lam[0]))
        out["p_ext"] = (_amax(Wl @ X), _amax(np.sum(np.abs(Wl), axis=1)) * _amax(X) * turn)
    return out


def sinrs_of(c, ex, k, MsPk, W):
    """The 50-digit SINR formula on a given (MsPk, W) -> (long double [ns], sensitivity [ns], sensitivity of a SOLVE [ns]).
    The last is for SINRs of a solution computed from the channel rather than evaluated on given (MsPk, W): there W itself
    moves: delta W = -W delta E W with ||delta E|| <= eps ||H_k||_F ||MsPk||_F, so every row W_i moves by the relative
    eps ||W||_F ||H_k||_F ||MsPk||_F = eps _amp().  SINR_i ~ |m_ii|^2 / ext_i is linear in W_i twice in the numerator
    (|m_ii|^2, m_ii = W_i h_i) and twice in the denominator (ext_i = W_i Re W_i^H): 2 + 2 = 4 relative eps _amp() on top.
    The sensitivity is the
    first-order relative change of SINR_i = |m_ii|^2 / (internal_i + ext_i), m = W H_k MsPk, per relative eps of its inputs:
    m_ii ~ 1 moves by eps a_i with a_i = ||W_i|| ||H_k||_F ||MsPk||_F (2 a_i on the square), ext_i = W_i Re W_i^H by
    eps ||W_i||^2 ||Re||_F; so a value computed from the kernel's unrounded (MsPk, W) may differ from the formula on the
    returned ones by eps (2 a_i + ||W_i||^2 ||Re||_F / den_i)."""
    m = ex["mp"][k]
    s = linear_sinrs(m["Hk"] * to_mp(MsPk), to_mp(W), m["Re"])
    out = np.array([np.longdouble("inf") if v == mp.inf else to_ld([v])[0] for v in s], dtype=np.longdouble)
    Wl, r = ld(W), c.r
    wn = np.sqrt(np.sum(np.abs(Wl) ** 2, axis=1)).astype(float)
    a = wn * float(np.sqrt(np.sum(np.abs(ld(ex["H"])[k * r:(k + 1) * r]) ** 2)) * np.sqrt(np.sum(np.abs(ld(MsPk)) ** 2)))
    M = Wl @ (ld(ex["H"])[k * r:(k + 1) * r] @ ld(MsPk))
    den = (np.abs(np.diag(M)) ** 2 / out).astype(float)
    amp = _amp(ld(ex["H"])[k * r:(k + 1) * r], ld(MsPk), Wl)
    sens = 2.0 * a + wn ** 2 * float(np.sqrt(np.sum(np.abs(ex["Re"][k]) ** 2))) / den
    return out, np.maximum(sens, 1.0), np.maximum(4.0 * amp + sens, 1.0)


# ---- NumPy complex128 on the same inputs -----------------------------------------------------------------------------
def whitening_with(c, Wf):
    """WhiteningBD.block_diagonalize_no_waterfilling (oracle/bd.py::whitening_bd) with the given whitening filters Wf_k
    -> (Ms per user, W per user)."""
    from scipy.linalg import block_diag
    K, r = c.K, c.r
    big_wf = block_diag(*Wf)
    newH, Ms = obd.block_diagonalize_no_waterfilling(big_wf @ c.big_H[:, :K * r], K, c.iPu)
    big_W = np.linalg.pinv(newH) @ big_wf
    return [Ms[:, k * r:(k + 1) * r] for k in range(K)], [big_W[k * r:(k + 1) * r, k * r:(k + 1) * r] for k in range(K)]


def np_whitening(c):
    """oracle/bd.py::whitening_bd in complex128 with the whitening filter from numpy.linalg.eigh.  The reference takes
    numpy.linalg.eig, which returns a NON-orthogonal basis of a repeated eigenvalue's space (n_ext < r - 1, rank-deficient
    H_ext,k); V diag(L^-1/2) then does not whiten and the equivalent channels' columns are not orthogonal under Re^-1.  With
    simple eigenvalues the two agree (tests/test_bd_extint_oracle_cpu.py).  The kernel whitens in every case, so this is
    the complex128 yardstick; Ms Ms^H, W^H W and |W H_k Ms| are the same for either."""
    Re = obd.cov_extint_plus_noise(c.big_H, c.K, c.r, c.K * c.r, c.pe, c.nv)
    Wf = []
    for R in Re:
        L, V = np.linalg.eigh(R)
        Wf.append(np.diag(L ** -0.5) @ V.conj().T)
    Ms, W = whitening_with(c, Wf)
    return Ms, W, [c.r] * c.K


def np_enhanced(c, metric=None, num_streams=None, Ms_bad=None):
    return obd.enhanced_bd(c.big_H, c.K, c.r, c.r, c.iPu, c.nv, c.pe, metric, num_streams, None, Ms_bad=Ms_bad)


def np_ms_bad(c):
    """The reference's unit-norm BD directions in the kernel's phase convention."""
    return obd.canonical_columns(obd.bd_no_power_scaling(c.big_H[:, :c.K * c.r], c.K)[0])


def np_candidate(c, k, Msk, rule, ns):
    """One candidate of oracle/bd.py::enhanced_bd in complex128 -> (MsPk, W, sinrs)."""
    r, n = c.r, c.K * c.r
    Re = obd.cov_extint_plus_noise(c.big_H, c.K, r, n, c.pe, c.nv)[k]
    Heq = c.big_H[k * r:(k + 1) * r, :n] @ Msk
    Pk = np.eye(r)[:, :ns] if (rule == "naive" or (rule == "auto" and ns == r)) else obd.stream_reduction_matrix(Re, ns)
    norm_term = np.linalg.norm(Msk @ Pk, "fro") / np.sqrt(c.iPu)
    Hred = Heq @ (Pk / norm_term)
    W = obd.ebd_receive_filter(Hred, Pk)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = obd.ebd_linear_sinrs(Hred, W, Re)
    return Msk @ Pk / norm_term, W, s
