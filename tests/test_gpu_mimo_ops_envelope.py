"""The per-channel MIMO operators (csrc/kernels_mimo.hip, mimo.hpp, mimo_svd.hpp) against a 50-digit oracle on the channels
where such kernels break -- repeated singular values, a singular value at the geometric mean, real-valued, ill
conditioned, scaled by 2^+-40, rank deficient -- in complex128 and complex64, at a batch of one full workgroup and a
ragged one, across the grid stride, and the shape-generic operators up to 64 antennas.

Tolerances come from the reference at the same dtype, measured at run time against the same oracle
(tests/mimo_ops_oracle.py): for a quantity q with oracle value q*, e_np = |q_numpy - q*|_max, e_gpu = |q_gpu - q*|_max and
the bound is e_gpu <= 8 max(e_np, eps_dt scale), per class and size as the worst over the twelve matrices.  Every test
prints the ratio e_gpu / max(e_np, eps_dt scale) per class before it asserts (pytest -s); the worst of each is in DESIGN.md.

Where this file had to read the issue that set it:
  * the Blast filter of `deficient` must be flagged at noise_var = 0.  At noise_var = 0.1 the matrix that is factored,
    H^H H + 0.1 I, is positive definite with cond <= 1 + 10 sigma_1^2: such a call must NOT be flagged and meets the MMSE bound.
  * the GMD's receive filter is the Blast filter of the equivalent channel (the same normal-equations Cholesky), so `graded`
    takes part in the flag and in the G comparison up to the Blast filter's limits (cond 1e6 in f64, 1e2 in f32); R, W and
    Q^H Q are checked at every cond where the call is not flagged.
  * R is a function of S alone only while the decomposition's comparisons d >= sigma_bar are decided by S and not by
    rounding: with a singular value AT the geometric mean or a repeated pair the planar rotation is 0/0 and any angle gives
    a valid decomposition, so R is compared entry by entry on rayleigh, real, diagonal, graded and scaled, and by its
    invariants (triangular, constant diagonal, Heq^H Heq = R^T R, i.e. Q unitary) on every class."""
import math

import numpy as np
import pytest

import mimo_ops_oracle as mo
from oracle import mimo as omimo

pytestmark = pytest.mark.gpu

DTS = ("f64", "f32")
LD, CLD = np.longdouble, np.clongdouble
KAPPA_MAX = {"f64": 1e6, "f32": 1e2}            # the Blast filter's contract (include/mcle.h at mcle_blast_filter)
R_UNIQUE = ("rayleigh", "real", "diagonal", "graded", "scaled")


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def twelve(*arrays):
    """The outputs of a tiled batch -> their first twelve items, after checking every copy against its twin bit for bit."""
    out = []
    for a in arrays:
        assert bits_equal(a, a[np.arange(a.shape[0]) % mo.PER_CLASS]), "a tiled copy differs from its twin"
        out.append(a[:mo.PER_CLASS])
    return out


class Report:
    """Collects (label, e_gpu, limit-without-the-factor) triples, prints the ratios, asserts them all at the end."""

    def __init__(self, title):
        self.title, self.rows, self.fails = title, [], []

    def check(self, label, e_gpu, e_np, eps, scale, extra=1.0):
        base = max(float(e_np), eps * float(scale)) * extra
        ratio = float(e_gpu) / base if base > 0 else (0.0 if e_gpu == 0 else float("inf"))
        self.rows.append((label, ratio))
        if not ratio <= mo.FACTOR:
            self.fails.append("%s: e_gpu %.3g, e_np %.3g, eps*scale %.3g, x%.3g -> ratio %.3g" % (label, e_gpu, e_np, eps * scale, extra, ratio))

    def require(self, cond, label):
        if not cond:
            self.fails.append(label)

    def finish(self):
        worst = {}
        for label, ratio in self.rows:
            key = label.split("|")[0]
            worst[key] = max(worst.get(key, 0.0), ratio)
        print("\n%s: e_gpu / max(e_np, eps scale)" % self.title)
        for key, ratio in worst.items():
            print("    %-34s %8.3f" % (key, ratio))
        assert not self.fails, "%s\n  %s" % (self.title, "\n  ".join(self.fails))


def recon(U, S, Vn, H):
    """|U diag(S) Vn^H - H|_max in long double."""
    U, Vn = np.asarray(U).astype(CLD), np.asarray(Vn).astype(CLD)
    if not (np.all(np.isfinite(U)) and np.all(np.isfinite(Vn))):
        return float("inf")
    return float(np.max(np.abs((U * np.asarray(S).astype(LD)[None, :]) @ Vn.conj().T - H.astype(CLD))))


# ---- SVD filters ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", mo.SIZES)
@pytest.mark.parametrize("dt", DTS)
def test_svd_filters(engine, dt, n):
    eps, root = mo.EPS[dt], math.sqrt(n)
    rep = Report("svd_filters %s n=%d" % (dt, n))
    keep = {}
    for cls in mo.CLASSES:
        o = mo.oracle(cls, n, n, dt)
        meta = mo.matrices(cls, n, n)[1]
        W, G, S = twelve(*engine.svd_filters(mo.tiled(o["H"]).astype(mo.CDT[dt]), dtype=dt))
        keep[cls] = (W, G, S)
        ref = [mo.np_svd_filters(o["H"][i], dt) for i in range(mo.PER_CLASS)]
        nsv = [mo.np_svd(o["H"][i], dt) for i in range(mo.PER_CLASS)]
        s1 = max(float(s[0]) for s in o["S"])
        rank = meta["rank"] if cls == "deficient" else [n] * mo.PER_CLASS
        rng = range(mo.PER_CLASS)
        rep.require(np.all(np.isfinite(S)) and np.all(np.isfinite(W)), cls + ": S or W not finite")
        rep.check(cls + " S", max(mo.maxerr(S[i], o["S"][i]) for i in rng), max(mo.maxerr(ref[i][2], o["S"][i]) for i in rng), eps, s1)
        rep.check(cls + " W unitary", max(mo.unitarity(W[i] * root) for i in rng),
                  max(mo.unitarity(nsv[i][2].conj().T) for i in rng), eps, 1.0)
        # U = G^H diag(S) / sqrt(n): the columns of a non-zero sigma (all of them outside `deficient`)
        Ug = [(G[i].astype(CLD).conj().T * S[i].astype(LD)[None, :] / root)[:, :rank[i]] for i in rng]
        rep.check(cls + " U unitary", max(mo.unitarity(Ug[i]) for i in rng), max(mo.unitarity(nsv[i][0][:, :rank[i]]) for i in rng), eps, 1.0)
        rep.check(cls + " U S V^H = H", max(recon(Ug[i], S[i][:rank[i]], (W[i] * root)[:, :rank[i]], o["H"][i]) for i in rng),
                  max(recon(nsv[i][0], nsv[i][1], nsv[i][2].conj().T, o["H"][i]) for i in rng), eps, s1)
        if cls in ("rayleigh", "graded"):
            use = [i for i in rng if o["cond"][i] <= 1.01e6]
            for q, got, k in (("W", W, 0), ("G", G, 1)):
                e_np = max(mo.maxerr(ref[i][k], o[q][i]) for i in use)
                scale = max(float(np.max(np.abs(o[q][i]))) for i in use)
                for i in use:
                    rep.check("%s %s entries|%d" % (cls, q, i), mo.maxerr(got[i], o[q][i]), e_np, eps, scale, extra=1.0 / o["gap"][i])
    # scaled: every threshold of jacobi_svd is relative, so a power of two goes straight through
    (Wr, Gr, Sr), (Ws, Gs, Ss) = keep["rayleigh"], keep["scaled"]
    f = np.where(np.arange(mo.PER_CLASS) < mo.PER_CLASS // 2, 2.0 ** -40, 2.0 ** 40)
    rep.require(bits_equal(Ss, Sr * f[:, None]), "scaled: S is not exactly 2^+-40 times the unscaled S")
    rep.require(bits_equal(Ws, Wr), "scaled: W differs from the unscaled W")
    rep.require(bits_equal(Gs, (Gr / f[:, None, None]).astype(Gr.dtype)), "scaled: G is not exactly 2^-+40 times the unscaled G")
    rep.finish()


# ---- GMD filters ---------------------------------------------------------------------------------------------------
def np_gmd(H, dt):
    """oracle/mimo.py's GMD from NumPy's SVD at the call's dtype -> (Q, R, P), or None where it cannot be formed."""
    U, S, Vh = mo.np_svd(H, dt)
    try:
        with np.errstate(all="ignore"):
            return omimo.gmd(U, S.astype(float), Vh)        # (the product of four float32 values near 2^-40 underflows)
    except (ZeroDivisionError, ValueError):                  # a singular value that is 0 at this dtype
        return None


@pytest.mark.parametrize("nv", [0.0, 0.05])
@pytest.mark.parametrize("n", mo.SIZES)
@pytest.mark.parametrize("dt", DTS)
def test_gmd_filters(engine, dt, n, nv):
    eps, root = mo.EPS[dt], math.sqrt(n)
    rep = Report("gmd_filters %s n=%d nv=%g" % (dt, n, nv))
    for cls in mo.CLASSES:
        o = mo.oracle(cls, n, n, dt)
        W, G, R, sk = twelve(*engine.gmd_filters(mo.tiled(o["H"]).astype(mo.CDT[dt]), nv, dtype=dt, return_skipped=True))
        if cls == "deficient":
            rep.require(np.all(sk == 1), "deficient: unflagged %s" % np.flatnonzero(sk == 0).tolist())
            continue
        rng = range(mo.PER_CLASS)
        inside = [i for i in rng if o["cond"][i] <= 1.01 * KAPPA_MAX[dt]]
        rep.require(not sk[inside].any(), cls + ": flagged %s" % np.flatnonzero(sk).tolist())
        live = [i for i in rng if sk[i] == 0]
        rep.require(all(np.all(np.isfinite(W[i])) and np.all(np.isfinite(R[i])) for i in live), cls + ": W or R not finite")
        rep.require(all(np.all(np.isfinite(G[i])) for i in inside), cls + ": G not finite")
        R50 = mo.oracle_gmd_R(cls, n, dt)
        ref = {i: np_gmd(o["H"][i], dt) for i in live}          # (a live channel's sigma_min is far from 0 in the dtype)
        s1 = max(float(o["S"][i][0]) for i in live)
        lref = [i for i in live if ref[i] is not None]       # where the reference at the dtype has an answer
        rep.require(len(lref) > 0 and all(ref[i] is not None for i in inside), cls + ": no NumPy reference")
        bar = max(float(R50[i][0, 0]) for i in live)
        for i in live:
            rep.require(not np.tril(R[i], -1).any() and np.all(np.diag(R[i]) == R[i][0, 0]), "%s %d: R not triangular with a constant diagonal" % (cls, i))
        rep.check(cls + " R diagonal", max(mo.maxerr(np.diag(R[i]), np.diag(R50[i])) for i in live),
                  max(mo.maxerr(np.diag(ref[i][1]), np.diag(R50[i])) for i in lref), eps, bar)
        if cls in R_UNIQUE:
            rep.check(cls + " R", max(mo.maxerr(R[i], R50[i]) for i in live), max(mo.maxerr(ref[i][1], R50[i]) for i in lref), eps, bar)
        rep.check(cls + " W unitary", max(mo.unitarity(W[i] * root) for i in live), max(mo.unitarity(ref[i][2]) for i in lref), eps, 1.0)

        def gram_err(Wn, Rm, i):
            Heq = o["H"][i].astype(CLD) @ np.asarray(Wn).astype(CLD)
            Rm = np.asarray(Rm).astype(LD)
            return float(np.max(np.abs(Heq.conj().T @ Heq - Rm.T @ Rm)))
        rep.check(cls + " Heq^H Heq = R^T R", max(gram_err(W[i] * root, R[i], i) for i in live),
                  max(gram_err(ref[i][2], ref[i][1], i) for i in lref), eps, s1 * s1)
        # G against the 50-digit Blast filter of Heq = H W sqrt(n), W the one that came with it (the device's filter is that
        # of its own Q R, which is H W sqrt(n) to rounding; the NumPy chain -- pinv / solve of its Q R -- is held to the same)
        def g_err(Wn, Gf, i):
            G50 = mo.to_ld(mo.blast_filter(o["Hm"][i] * mo.to_mp(np.asarray(Wn).astype(np.complex128)), nv))
            return mo.maxerr(Gf, G50), float(np.max(np.abs(G50)))
        part = [i for i in inside if sk[i] == 0]
        dev = [g_err(W[i] * root, G[i], i) for i in part]
        npy = [g_err(ref[i][2], mo.np_blast_filter(ref[i][0] @ ref[i][1], nv, dt), i) for i in part]
        if nv > 0:
            rep.check(cls + " G MMSE", max(e for e, _ in dev), max(e for e, _ in npy), eps, max(s for _, s in dev))
        else:
            for i, (e, s), (e_np, _) in zip(part, dev, npy):        # normal equations: one more power of cond
                rep.check("%s G ZF|%d" % (cls, i), e, e_np, eps, s, extra=o["cond"][i])
    rep.finish()


# ---- Blast filter --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nr,nt", mo.BLAST_SHAPES)
@pytest.mark.parametrize("dt", DTS)
def test_blast_filter(engine, dt, nr, nt):
    eps = mo.EPS[dt]
    rep = Report("blast_filter %s %dx%d" % (dt, nr, nt))
    for cls in mo.CLASSES:
        o = mo.oracle(cls, nr, nt, dt)
        Hb = mo.tiled(o["H"]).astype(mo.CDT[dt])
        inside = [i for i in range(mo.PER_CLASS) if o["cond"][i] <= 1.01 * KAPPA_MAX[dt] or cls == "deficient"]
        for nv in (0.0, 0.1):
            G50 = mo.oracle_blast(cls, nr, nt, dt, nv)
            ref = [mo.np_blast_filter(o["H"][i], nv, dt) for i in range(mo.PER_CLASS)]
            for generic in (0, 1):
                with engine.options(staged_generic=generic):
                    G, sk = twelve(*engine.blast_filter(Hb, nv, dtype=dt))
                tag = "%s nv=%g %s" % (cls, nv, "direct" if generic else "default")
                if cls == "deficient" and nv == 0:
                    rep.require(np.all(sk == 1), "%s: %d of %d unflagged %s, |G|_max %.3g" % (
                        tag, int(np.sum(sk == 0)), mo.PER_CLASS, np.flatnonzero(sk == 0).tolist(),
                        max([float(np.max(np.abs(G[i]))) for i in np.flatnonzero(sk == 0)] or [0.0])))
                    continue
                rep.require(not sk[inside].any(), tag + ": flagged %s" % np.flatnonzero(sk).tolist())
                rep.require(all(np.all(np.isfinite(G[i])) for i in inside), tag + ": G not finite")
                if nv > 0:
                    rep.check("%s nv=%g MMSE" % (cls, nv), max(mo.maxerr(G[i], G50[i]) for i in inside),
                              max(mo.maxerr(ref[i], G50[i]) for i in inside), eps, max(float(np.max(np.abs(G50[i]))) for i in inside))
                else:
                    for i in inside:                      # normal equations: one more power of cond than the pseudo-inverse
                        rep.check("%s ZF|%d" % (cls, i), mo.maxerr(G[i], G50[i]), mo.maxerr(ref[i], G50[i]), eps,
                                  float(np.max(np.abs(G50[i]))), extra=o["cond"][i])
    rep.finish()


# ---- grid stride ---------------------------------------------------------------------------------------------------
def test_grid_stride_items_equal_their_twins(engine):
    """batch = n_cu * 16 * 64 + 70 complex64 rayleigh tiles: more than the capped grid takes in one step, so every workgroup
    walks its stride at least once and the last step is ragged; every item equals its twin of the 70-batch bit for bit."""
    big = engine.device_info()["n_cu"] * 16 * 64 + 70
    idx = np.arange(big) % mo.PER_CLASS
    for n in (2, 4):
        H12 = mo.rounded("rayleigh", n, n, "f32")[0].astype(np.complex64)
        small, large = mo.tiled(H12), np.ascontiguousarray(H12[idx])
        for name, call in (("svd_filters", lambda H: engine.svd_filters(H, dtype="f32")),
                           ("gmd_filters", lambda H: engine.gmd_filters(H, 0.05, dtype="f32", return_skipped=True)),
                           ("blast_filter", lambda H: engine.blast_filter(H, 0.1, dtype="f32"))):
            want = twelve(*call(small))
            got = call(large)
            assert engine.last_kernel() == "blast_filter staged" or name != "blast_filter"
            for w, g in zip(want, got):
                assert g.shape[0] == big and bits_equal(g, w[idx]), (name, n, np.flatnonzero(np.any((g != w[idx]).reshape(big, -1), axis=1))[:8])
            del got


# ---- shapes up to 64 -----------------------------------------------------------------------------------------------
def crandn(rs, shape, dt):
    return ((rs.randn(*shape) + 1j * rs.randn(*shape)) / math.sqrt(2)).astype(mo.CDT[dt])


def assert_within(got, want, limit, what):
    """|got - want| <= limit elementwise (long double), got finite."""
    assert np.all(np.isfinite(got)), what
    err = np.abs(np.asarray(got).astype(CLD) - want)
    bad = err > limit
    assert not bad.any(), "%s: worst err / bound %.3g" % (what, float(np.max(err[bad] / limit[bad])))
    with np.errstate(all="ignore"):
        print("    %-40s worst err / bound %.3g" % (what, float(np.max(np.where(limit > 0, err / np.where(limit > 0, limit, 1), 0)))))


@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("nt", [1, 2, 5, 63, 64])
@pytest.mark.parametrize("dt", DTS)
def test_mrt_up_to_64(engine, dt, nt, n):
    """X[a] = exp(-j angle(h_a)) / sqrt(nt) x (one product: k = 1); out = y sqrt(nt) / sum |h| (k = nt terms in the divisor)."""
    rs, eps = np.random.RandomState(100 + nt), mo.EPS[dt]
    h, x = crandn(rs, (3, nt), dt), crandn(rs, (3, n), dt)
    h[1, nt // 2] = 0                                          # angle(0) = 0: the precoder entry is 1 / sqrt(nt)
    if nt == 1:
        h[1, 0], h[2, 0] = 0, -1.0                            # (an all-zero h has no decoder: only encoded)
    hl, xl = h.astype(CLD), x.astype(CLD)
    mag = np.abs(hl)
    w = np.where(mag > 0, hl.conj() / np.where(mag > 0, mag, 1), 1) / np.sqrt(LD(nt))
    want = w[:, :, None] * xl[:, None, :]
    assert_within(engine.mrt_encode(h, x, dtype=dt), want, 4 * eps * np.abs(want), "mrt_encode %s nt=%d n=%d" % (dt, nt, n))
    rows = [b for b in range(3) if mag[b].sum() > 0]
    g = np.sqrt(LD(nt)) / mag[rows].sum(axis=1)
    want = xl[rows] * g[:, None]
    assert_within(engine.mrt_decode(h[rows], x[rows], dtype=dt), want, 4 * nt * eps * np.abs(want), "mrt_decode %s nt=%d n=%d" % (dt, nt, n))


@pytest.mark.parametrize("n", [2, 258])
@pytest.mark.parametrize("nr", [1, 3, 64])
@pytest.mark.parametrize("dt", DTS)
def test_alamouti_up_to_64(engine, dt, nr, n):
    """Decode: 2 nr products per output over |H|_F^2 (2 nr squares): the inner-product bound on the numerator plus the same
    relative error on the divisor."""
    rs, eps = np.random.RandomState(200 + nr), mo.EPS[dt]
    x, H, Y = crandn(rs, (3, n), dt), crandn(rs, (3, nr, 2), dt), crandn(rs, (3, nr, n), dt)
    xl = x.astype(CLD)
    want = np.empty((3, 2, n), dtype=CLD)
    want[:, 0, 0::2], want[:, 0, 1::2] = xl[:, 0::2], -xl[:, 1::2].conj()
    want[:, 1, 0::2], want[:, 1, 1::2] = xl[:, 1::2], xl[:, 0::2].conj()
    want /= np.sqrt(LD(2))
    assert_within(engine.alamouti_encode(x, batch=3, dtype=dt), want, 4 * eps * np.abs(want), "alamouti_encode %s n=%d" % (dt, n))
    Hl, Yl = H.astype(CLD), Y.astype(CLD)
    h0, h1 = Hl[:, :, 0], Hl[:, :, 1]
    fro2 = np.sum(np.abs(Hl) ** 2, axis=(1, 2))[:, None]
    want = np.empty((3, n), dtype=CLD)
    want[:, 0::2] = np.einsum("br,brc->bc", h0.conj(), Yl[:, :, 0::2]) + np.einsum("br,brc->bc", h1, Yl[:, :, 1::2].conj())
    want[:, 1::2] = np.einsum("br,brc->bc", h1.conj(), Yl[:, :, 0::2]) - np.einsum("br,brc->bc", h0, Yl[:, :, 1::2].conj())
    want = want / fro2 * np.sqrt(LD(2))
    mass = np.einsum("br,brc->bc", np.abs(h0) + np.abs(h1), np.abs(Yl[:, :, 0::2]) + np.abs(Yl[:, :, 1::2]))
    limit = np.repeat(2 * 4 * (2 * nr) * eps * mass / fro2 * np.sqrt(LD(2)), 2, axis=1)
    assert_within(engine.alamouti_decode(H, Y, dtype=dt), want, limit, "alamouti_decode %s nr=%d n=%d" % (dt, nr, n))


GENERIC_SHAPES = [(1, 1), (5, 3), (64, 64), (64, 1), (1, 64)]


@pytest.mark.parametrize("ns", [1, 7])
@pytest.mark.parametrize("nr,nt", GENERIC_SHAPES)
@pytest.mark.parametrize("dt", DTS)
def test_blast_decode_up_to_64(engine, dt, nr, nt, ns):
    rs, eps = np.random.RandomState(300 + nr + 64 * nt), mo.EPS[dt]
    G, Y = crandn(rs, (3, nt, nr), dt), crandn(rs, (3, nr, ns), dt)
    Gl, Yl = G.astype(CLD), Y.astype(CLD)
    want = np.transpose(Gl @ Yl, (0, 2, 1)).reshape(3, -1)           # est[c nt + a]
    limit = 4 * nr * eps * np.transpose(np.abs(Gl) @ np.abs(Yl), (0, 2, 1)).reshape(3, -1)
    assert_within(engine.blast_decode(G, Y, dtype=dt), want, limit, "blast_decode %s %dx%d ns=%d" % (dt, nr, nt, ns))


@pytest.mark.parametrize("ns", [1, 7])
@pytest.mark.parametrize("nr,nt", GENERIC_SHAPES)
@pytest.mark.parametrize("dt", DTS)
def test_mimo_channel_up_to_64(engine, dt, nr, nt, ns):
    """Y = H X + sqrt(noise_var) noise with the noise injected: nt + 1 terms."""
    rs, eps, nv = np.random.RandomState(400 + nr + 64 * nt), mo.EPS[dt], 0.3
    H, X, Z = crandn(rs, (3, nr, nt), dt), crandn(rs, (3, nt, ns), dt), crandn(rs, (3, nr, ns), dt)
    Hl, Xl, Zl = H.astype(CLD), X.astype(CLD), Z.astype(CLD)
    sigma = np.sqrt(LD(nv))
    assert_within(engine.mimo_channel(H, X, noise=Z, noise_var=nv, dtype=dt), Hl @ Xl + sigma * Zl,
                  4 * (nt + 1) * eps * (np.abs(Hl) @ np.abs(Xl) + sigma * np.abs(Zl)), "mimo_channel %s %dx%d ns=%d" % (dt, nr, nt, ns))


@pytest.mark.parametrize("nv", [0.0, 0.07])
@pytest.mark.parametrize("nr,nt,ns", [(1, 1, 1), (5, 3, 2), (64, 3, 1), (64, 64, 64)])
def test_post_processing_sinrs_up_to_64(engine, nr, nt, ns, nv):
    """SINR_i = |E_ii|^2 / (|sum_{j != i} E_ij|^2 + nv |g_i|^2), E = G H W (complex128 only).  The inner-product bound on every
    E_ij (nr + nt nested terms), on the row sum (ns terms) and on |g_i|^2 (nr terms), carried through the squares and the
    quotient without linearising: the largest value minus the smallest value the quotient can take."""
    rs, eps = np.random.RandomState(500 + nr + nt + ns), mo.EPS["f64"]
    H, W, G = crandn(rs, (3, nr, nt), "f64"), crandn(rs, (3, nt, ns), "f64"), crandn(rs, (3, ns, nr), "f64")
    Hl, Wl, Gl = H.astype(CLD), W.astype(CLD), G.astype(CLD)
    E = Gl @ Hl @ Wl
    dE = 4 * (nr + nt) * eps * (np.abs(Gl) @ np.abs(Hl) @ np.abs(Wl))
    diag, ddiag = np.abs(np.einsum("bii->bi", E)), np.einsum("bii->bi", dE)
    off = np.abs(E.sum(axis=2) - np.einsum("bii->bi", E))
    doff = (dE.sum(axis=2) + 4 * ns * eps * np.abs(E).sum(axis=2)) * (ns > 1)      # (one stream: the kernel's row - diag is exactly 0)
    gn = np.sum(np.abs(Gl) ** 2, axis=2)
    N, dN = nv * gn, 4 * (nr + 1) * eps * nv * gn
    D_lo = np.maximum(off - doff, 0) ** 2 + N - dN
    D_hi, D = (off + doff) ** 2 + N + dN, off ** 2 + N
    got = engine.post_processing_sinrs(H, W, G, nv)
    if nv == 0 and ns == 1:
        assert np.all(np.isposinf(got))                                # S / 0, as the reference's division gives
        return
    assert np.all(D_lo > 0)
    want = diag ** 2 / D
    limit = np.maximum((diag + ddiag) ** 2 / D_lo - want, want - np.maximum(diag - ddiag, 0) ** 2 / D_hi) + 4 * eps * want
    assert_within(got, want, limit, "post_processing_sinrs %dx%dx%d nv=%g" % (nr, nt, ns, nv))
    if (nr, nt, ns) == (5, 3, 2):                                      # the long-double reference against the 50 digits, once
        s50 = mo.post_processing_linear_sinrs(mo.to_mp(H[0]), mo.to_mp(W[0]), mo.to_mp(G[0]), nv)
        assert mo.maxerr(want[0].astype(float), mo.to_ld(s50)) <= 1e-15 * float(np.max(want[0]))


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(engine):
    """65 or 0 antennas, an odd Alamouti length and an SVD / GMD size outside 2..4 are ValueErrors, and the output a refused
    call was given is untouched.  (Every buffer is large enough for 65 antennas.)"""
    lib, ctx, dt = engine.lib, engine.ctx, engine._dt("f64")
    n, b = 6, 2
    src = engine.to_device(np.ones(b * 65 * 65 * n, dtype=np.complex128))
    sentinel = np.full(b * 65 * 65 * n, -7.25 + 3.5j, dtype=np.complex128)
    out = engine.to_device(sentinel)
    out2 = engine.to_device(sentinel)
    S = engine.to_device(np.full(b * 65, -7.25))
    sk = engine.to_device(np.full(b, 77, dtype=np.uint32))
    calls = []
    for bad in (0, 65):
        calls += [lambda a=bad: lib.mcle_mrt_encode(ctx, dt, src.ptr, src.ptr, a, n, out.ptr, b),
                  lambda a=bad: lib.mcle_mrt_decode(ctx, dt, src.ptr, src.ptr, a, n, out.ptr, b),
                  lambda a=bad: lib.mcle_alamouti_decode(ctx, dt, src.ptr, src.ptr, a, n, out.ptr, b),
                  lambda a=bad: lib.mcle_blast_decode(ctx, dt, src.ptr, src.ptr, a, 2, n, out.ptr, b),
                  lambda a=bad: lib.mcle_blast_decode(ctx, dt, src.ptr, src.ptr, 2, a, n, out.ptr, b),
                  lambda a=bad: lib.mcle_mimo_channel(ctx, dt, src.ptr, src.ptr, None, 0.0, a, 2, n, out.ptr, b),
                  lambda a=bad: lib.mcle_mimo_channel(ctx, dt, src.ptr, src.ptr, None, 0.0, 2, a, n, out.ptr, b),
                  lambda a=bad: lib.mcle_post_processing_sinrs(ctx, src.ptr, src.ptr, src.ptr, 0.1, a, 2, 2, S.ptr, b),
                  lambda a=bad: lib.mcle_post_processing_sinrs(ctx, src.ptr, src.ptr, src.ptr, 0.1, 2, a, 2, S.ptr, b),
                  lambda a=bad: lib.mcle_post_processing_sinrs(ctx, src.ptr, src.ptr, src.ptr, 0.1, 2, 2, a, S.ptr, b)]
    calls += [lambda: lib.mcle_alamouti_encode(ctx, dt, src.ptr, 7, out.ptr, b),
              lambda: lib.mcle_alamouti_decode(ctx, dt, src.ptr, src.ptr, 2, 7, out.ptr, b)]
    for bad in (1, 5):
        calls += [lambda a=bad: lib.mcle_svd_filters(ctx, dt, src.ptr, a, out.ptr, out2.ptr, S.ptr, b),
                  lambda a=bad: lib.mcle_gmd_filters(ctx, dt, src.ptr, a, 0.0, out.ptr, out2.ptr, S.ptr, sk.ptr, b)]
    for k, call in enumerate(calls):
        with pytest.raises(ValueError):
            engine._raise_value(call())
    engine.sync()
    assert bits_equal(out.get(), sentinel) and bits_equal(out2.get(), sentinel)
    assert np.all(S.get() == -7.25) and np.all(sk.get() == 77)
    # the same through the Python surface
    rs = np.random.RandomState(1)
    with pytest.raises(ValueError):
        engine.mrt_encode(crandn(rs, (2, 65), "f64"), crandn(rs, (2, 4), "f64"))
    with pytest.raises(ValueError):
        engine.blast_decode(crandn(rs, (2, 65, 2), "f64"), crandn(rs, (2, 2, 4), "f64"))
    with pytest.raises(ValueError):
        engine.alamouti_decode(crandn(rs, (2, 3, 2), "f64"), crandn(rs, (2, 3, 7), "f64"))
    for bad in (1, 5):
        with pytest.raises(ValueError):
            engine.svd_filters(crandn(rs, (2, bad, bad), "f64"))
        with pytest.raises(ValueError):
            engine.gmd_filters(crandn(rs, (2, bad, bad), "f64"))
