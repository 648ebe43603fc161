"""Shared by tests/test_decide_forms_cpu.py and tests/test_gpu_decide_forms.py: constellation tables, probe points chosen at the
places where a symbol decision can go wrong, their grouping orders, and the exhaustive reference with its rounding bounds.

TABLES.  The stock tables (QAM 4 / 16 / 64 / 256, PSK 4, PSK 8 / 16 at offsets 0 and 0.3, QPSK, BPSK), the generic tables of
tests/test_demod_grid.py (irregular16, irregular64, apsk32, duplicates8: exact duplicates, the first index must win) and marker32:
24 points on a circle of radius 1e-3 inside an 8-PSK ring of radius 1, so that the candidate-grid cells around the origin
hold more than seven candidates and carry the 0xFF "sweep everything" marker (mcle_set_constellation wants a power of two).

POINTS (make_points; the structure of test_gpu_decide_probe._points).  Perpendicular bisectors of neighbouring pairs (each
point's eight nearest), inside the segment and up to three spacings along the boundary, moved off it by +-2^-k of the spacing:
complex128 k = 20 ... 42 (certificate margin 2^-30), complex64 k = 6, 9, 12, 14, 16, 18, 21 (margins: QAM / quadrant / on-axis 2^-15,
PSK sector 2^-12 -- k <= 12 is vouched for, k >= 16 takes the fallback); the table itself; rings at 1.5 / 4 / 50 / 300 radii;
random points; the exact-tie lines re = 0 / im = 0 where the table is exactly mirror-symmetric; points one and two float32 steps on
either side of the complex64 range limits of the certificates (QAM: 16 spacings beyond the outer level; PSK sector: [1/8, 8] rho;
on-axis: 8 a; quadrant: 256 max(a, b)), their other coordinate both anywhere and next to a decision boundary; and a point inside every
cell of the candidate grid, so that every list length the grid has is reached.  complex64 points are rounded to float32 BEFORE
anything else is computed.  Every point is finite: NaN and infinite inputs are left out on purpose -- how the device treats them is
not what these tests look for.

REFERENCE (Reference).  The exhaustive argmin of |p - c_m|^2 over the operands the device sees (complex64: point and table rounded
to float32), first index on exact ties.  float64 is enough wherever the runner-up is farther than 2^-40 of the distance; rows with a
closer contender are recomputed in numpy.longdouble (64-bit significand: the coordinate differences of float32 operands are exact
there, the squares carry 2^-64), and entries that still tie there are compared in rational arithmetic (fractions.Fraction of the
operands: exact), so an EXACT tie is one -- mirror images and duplicates -- and a gap of 2^-70 is a gap.

BOUNDS, from the code (u = 2^-24 / 2^-53, the unit roundoff).
  literal metric  d = dx * dx + dy * dy with dx = r.x - c.x (demod_mindist, demod_grid_search, walk_sweep): dx and dy carry u each,
      hence 2 u on a square; the product dx * dx one more, dy * dy one more unless it is fused, the sum one more: at most 4 u d, fused
      or not.
  two-FMA metric  h = fma(-r.y, c.y, fma(-r.x, c.x, c.z)), c.z = fl(|c|^2 / 2), which orders like |c - r|^2 / 2 (|r|^2 / 2 is common):
      one rounding for c.z (u |c|^2 / 2), one for the inner fma (u (|c|^2 / 2 + |r.x c.x|)), one for the outer (u (|c|^2 / 2 + |r.x c.x| +
      |r.y c.y|)): at most 3 u (|c|^2 / 2 + |r| |c|).
  slicers  t = x sc + off in level coordinates (spacing 1): the rounded scale moves t by u |x| sc, the multiply-adds by at most
      2 u (|x| sc + off), the rounded table entries move the true boundary by u |x| sc: a point is slicer-clear when both its level
      coordinates keep 4 u (|x| sc + off + 1) off every half-integer boundary.  (Exact boundaries are never clear: the slicers round
      half to even / half up there where the argmin takes the first index.)
A point is CLEAR for a metric when the exact gap from the nearest entry to every other entry exceeds the sum of the two entries'
bounds: there the label must be the reference's.  So it must where the nearest entry ties exactly with its mirror images in an axis
the point lies on, or with duplicates, and all the rest are clear of them (first index: such distances are the same numbers in
either metric; an exact tie of unrelated entries binds nobody).  On every other point the chosen
entry's exact distance must be within those bounds of the minimum, and an entry that ties exactly with the minimum must be the first
of them.  None of these figures is fitted to device output."""
import functools
from fractions import Fraction

import numpy as np

import test_demod_cert as tdc
import test_demod_grid as tdg
from pyphysim_amd import _lib
from pyphysim_amd.modulators import constellation

LD = np.longdouble
U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
OFFSETS = {"f64": (20, 29, 30, 31, 33, 38, 42), "f32": (6, 9, 12, 14, 16, 18, 21)}
UNCLEAR_CAP = 0.25
KS = (1, 2, 3, 4)
NS = (2, 4, 6)


def _tables():
    gen = dict(tdg.tables())
    marker = np.concatenate([1e-3 * np.exp(2j * np.pi * np.arange(24) / 24), np.exp(2j * np.pi * np.arange(8) / 8)])
    Q, G = _lib.CONST_QAM, _lib.CONST_GENERIC
    # name -> (table, kind, certificate that serves it, WDEC form of the min-distance walk)
    t = {"qam4": (constellation("qam", 4), Q, "qam", "qam_cert"), "qam16": (constellation("qam", 16), Q, "qam", "qam_cert"),
         "qam64": (constellation("qam", 64), Q, "qam", "qam_cert"), "qam256": (constellation("qam", 256), Q, "qam", "qam_cert"),
         "psk4": (constellation("psk", 4), G, "axis", "axis4_cert"),
         "psk8": (constellation("psk", 8), G, "psk", "generic"), "psk8+0.3": (constellation("psk", 8, 0.3), G, "psk", "generic"),
         "psk16": (constellation("psk", 16), G, "psk", "generic"), "psk16+0.3": (constellation("psk", 16, 0.3), G, "psk", "generic"),
         "qpsk": (constellation("qpsk"), G, "quad", "quad_cert"), "bpsk": (constellation("bpsk"), G, None, "generic")}
    for name in ("irregular16", "irregular64", "apsk32", "duplicates8"):
        t[name] = (gen[name], G, None, "generic")
    t["marker32"] = (marker, G, None, "generic")
    return {k: (np.asarray(v[0], dtype=np.complex128),) + v[1:] for k, v in t.items()}


TABLES = _tables()
NAMES = list(TABLES)
DTYPES = ("f32", "f64")


def operands(z, dtype):
    """what the device sees of a complex128 array in this arithmetic, held in complex128"""
    z = np.asarray(z, dtype=np.complex128)
    return z.astype(np.complex64).astype(np.complex128) if dtype == "f32" else z


def _steps32(v):
    """v rounded to float32 and its two float32 neighbours on either side (the device may compute a limit one step off)"""
    v = np.float32(v)
    out, lo, hi = [v], v, v
    for _ in range(2):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        out += [lo, hi]
    return np.array(out, dtype=np.float64)


def _range_points(table, cert, dtype, rs):
    """points on either side of the complex64 range limit of the table's certificate"""
    offs = [2.0 ** -k for k in OFFSETS[dtype]]
    out = []
    if cert == "qam":
        M = table.size
        L = int(round(np.sqrt(M)))
        scale = np.float32(np.sqrt((M - 1) * 2.0 / 3.0))
        rmax = (np.float32(16.0) + np.float32(L - 1) * np.float32(0.5)) / (scale * np.float32(0.5))
        spacing = 2.0 / np.sqrt((M - 1) * 2.0 / 3.0)
        bounds = (np.arange(L - 1) - (L - 2) / 2.0) * spacing
        ext = np.abs(table.real).max()
        for v in _steps32(rmax):
            for sgn in (-1.0, 1.0):
                near = np.concatenate([rs.choice(bounds, 2) + s * o * spacing for o in offs for s in (-1.0, 1.0)])
                other = np.concatenate([rs.uniform(-1.2, 1.2, 12) * ext, near])
                out += [sgn * v + 1j * other, other + 1j * sgn * v]
    elif cert == "psk":
        M = table.size
        rad = abs(table[0])
        phi0 = np.fmod(np.arctan2(table[0].imag, table[0].real), 2 * np.pi / M)
        phi0 += 2 * np.pi / M if phi0 < 0 else 0.0
        for lim in (rad * 0.125, rad * 8.0):
            for v in _steps32(lim):
                lo = rs.uniform(0.0, 1.0, 24) * v
                # next to the sector boundaries inside the octant too
                th = (2 * rs.randint(0, max(M // 8, 1), 14) + 1) * np.pi / M
                lo = np.concatenate([lo, v * np.tan(th) * (1.0 + np.repeat(offs, 2) * np.tile([-1.0, 1.0], len(offs)))])
                u = v + 1j * lo
                u = np.where(rs.randint(0, 2, u.size) == 1, u.imag + 1j * u.real, u)
                u = u.real * rs.choice([-1.0, 1.0], u.size) + 1j * u.imag * rs.choice([-1.0, 1.0], u.size)
                out += [u * np.exp(1j * phi0)]
    elif cert in ("axis", "quad"):
        a = np.max(np.abs(np.concatenate([table.real, table.imag])))
        lim = a * (8.0 if cert == "axis" else 256.0)
        for v in _steps32(lim):
            for sgn in (-1.0, 1.0):
                other = rs.uniform(-1.0, 1.0, 20) * lim
                out += [sgn * v + 1j * other, other + 1j * sgn * v]
    return out


def make_points(table, dtype, seed, cert=None, grid=None, max_pairs=1000):
    rs = np.random.RandomState(seed)
    M = table.size
    dist = np.abs(table[:, None] - table[None, :])
    local = np.where(dist > 0, dist, np.inf).min(axis=1)          # each point's spacing: its nearest distinct neighbour
    offs = np.array([2.0 ** -k for k in OFFSETS[dtype]])
    pts = [table.copy()]
    pairs = []
    for i in range(M):
        for j in np.argsort(dist[i], kind="stable")[1:9]:
            if j > i and dist[i, j] > 0:
                pairs.append((i, int(j)))
    if len(pairs) > max_pairs:
        pairs = [pairs[k] for k in np.sort(rs.choice(len(pairs), max_pairs, replace=False))]
    for i, j in pairs:
        mid, u = 0.5 * (table[i] + table[j]), (table[j] - table[i]) / abs(table[j] - table[i])
        s = min(local[i], local[j])
        for along in (0.0, 0.25, -0.4, 1.0, -3.0):
            base = mid + 1j * u * along * s
            pts += [base + u * offs * s, base - u * offs * s]
    ext = np.max(np.abs(table))
    t = rs.uniform(-1.2, 1.2, 600) * ext
    ops = operands(table, dtype)
    as_set = lambda v: set(zip(v.real.tolist(), v.imag.tolist()))
    if as_set(-np.conj(ops)) == as_set(ops):
        pts += [1j * t, np.zeros(1, dtype=complex)]                   # re = 0: a tie between c and -conj(c)
    if as_set(np.conj(ops)) == as_set(ops):
        pts += [t + 0j]                                               # im = 0: a tie between c and conj(c)
    ang = rs.uniform(0, 2 * np.pi, 400)
    for r in (1.5, 4.0, 50.0, 300.0):
        pts += [r * ext * np.exp(1j * ang)]
    pts += [(rs.uniform(-1.3, 1.3, 4000) + 1j * rs.uniform(-1.3, 1.3, 4000)) * ext]
    pts += _range_points(table, cert, dtype, rs)
    if grid is not None:
        G, x0, y0, inv_h, _ = grid
        c = np.float64(x0) + (np.arange(G) + 0.5) / np.float64(inv_h)
        # (off the centre in y: the centres of the diagonal cells would sit on the symmetry axis re = im of a table such as apsk32,
        #  a tie in exact arithmetic that the rounded cosines and sines of the table turn into a gap of an ulp)
        cx_, cy_ = np.meshgrid(c, np.float64(y0) + (np.arange(G) + 0.375) / np.float64(inv_h))
        pts += [(cx_ + 1j * cy_).ravel()]
    p = operands(np.concatenate(pts), dtype)
    assert np.isfinite(p.real).all() and np.isfinite(p.imag).all()
    return p[: 12 * (p.size // 12)]                                    # whole groups of 2, 3, 4 and 6


def cell_counts(pts, grid):
    """the count byte of each point's cell, looked up as modem.hpp grid_cell does (float32 arithmetic, clamped)"""
    G, x0, y0, inv_h, cells = grid
    x, y = pts.real.astype(np.float32), pts.imag.astype(np.float32)
    ix = np.clip(np.floor((x - x0) * inv_h).astype(np.int64), 0, G - 1)
    iy = np.clip(np.floor((y - y0) * inv_h).astype(np.int64), 0, G - 1)
    return (cells[iy * G + ix] & np.uint64(0xFF)).astype(np.int64)


def length_class(n):
    """0: one candidate, 1: two to four (the lockstep steps), 2: five to seven (the long-list loop), 3: the 0xFF marker"""
    return np.where(n == 0xFF, 3, np.where(n > 4, 2, np.where(n > 1, 1, 0)))


def certified(table, cert, pts, dtype):
    """CPU statement of the table's certificate (the models of tests/test_demod_cert.py; the on-axis one restated here for both
    arithmetics): which points it vouches for.  Used to ORDER the points and to prove the orders mix -- never as the reference."""
    T = np.float32 if dtype == "f32" else np.float64
    r = pts.astype(np.complex64) if dtype == "f32" else pts
    if cert == "qam":
        return tdc.cert_model(r, table.size, dtype)[1]
    if cert == "quad":
        return tdc.quad_cert_model(r, table, T)[1]
    if cert == "psk":
        return tdc.psk_cert_model(r, table, dtype)[1]
    if cert == "axis":
        a = float(np.max(np.abs(np.concatenate([table.real, table.imag]))))
        lo, hi = T(a * (2.0 ** -15 if dtype == "f32" else 2.0 ** -30)), T(a * (8.0 if dtype == "f32" else 256.0))
        x, y = r.real.astype(T), r.imag.astype(T)
        return (np.abs(x - y) >= lo) & (np.abs(x + y) >= lo) & (np.abs(x) <= hi) & (np.abs(y) <= hi)
    return np.zeros(pts.size, dtype=bool)


def _alternate(a, b):
    m = min(a.size, b.size)
    out = np.empty(2 * m, dtype=np.int64)
    out[0::2], out[1::2] = a[:m], b[:m]
    return np.concatenate([out, a[m:], b[m:]])


def make_orders(sure, long_list, seed):
    """natural order, a seeded permutation, and an interleave: first every long-list (n > 4 or 0xFF) point next to a short-list one
    (uncertified ones first, so that the group is searched), then the rest alternating certified with uncertified"""
    n = sure.size
    lng = np.flatnonzero(long_list)
    short_u, short_c = np.flatnonzero(~long_list & ~sure), np.flatnonzero(~long_list & sure)
    partner = np.concatenate([short_u, short_c])[: lng.size]
    head = _alternate(lng, partner)
    used = np.zeros(n, dtype=bool)
    used[head] = True
    rest_c, rest_u = np.flatnonzero(~used & sure), np.flatnonzero(~used & ~sure)
    inter = np.concatenate([head, _alternate(rest_c, rest_u)])
    assert np.array_equal(np.sort(inter), np.arange(n))
    return {"natural": np.arange(n), "permuted": np.random.RandomState(seed).permutation(n), "interleaved": inter}


def group_mix(mask, order, size):
    """per group of `size` consecutive points of the order: (has a True, has a False)"""
    m = mask[order][: size * (order.size // size)].reshape(-1, size)
    return m.any(axis=1), (~m).any(axis=1)


def _exact_distance(p, c):
    dx, dy = Fraction(p.real) - Fraction(c.real), Fraction(p.imag) - Fraction(c.imag)
    return dx * dx + dy * dy


def _same_numbers(p, cs):
    """do the entries cs give one and the same floating-point distance from p, whatever the metric?  Equal coordinates up to the
    sign, and a sign that differs only in a coordinate in which p is zero"""
    return bool(np.all(np.abs(cs.real) == abs(cs.real[0])) and np.all(np.abs(cs.imag) == abs(cs.imag[0])) and
                (p.real == 0 or np.all(cs.real == cs.real[0])) and (p.imag == 0 or np.all(cs.imag == cs.imag[0])))


class Reference:
    def __init__(self, table_ops, pts, dtype):
        assert np.finfo(LD).nmant >= 63, "numpy.longdouble with a 64-bit significand"
        u = U[dtype]
        self.table, self.pts, self.dtype, self.u = table_ops, pts, dtype, u
        cx_, cy_ = table_ops.real, table_ops.imag
        self.cabs = np.abs(table_ops)
        self.half = 0.5 * self.cabs ** 2
        n = pts.size
        self.best = np.empty(n, dtype=np.int64)
        self.d_best = np.empty(n, dtype=LD)
        # exact ties for the minimum.  tie_sets: point -> the tied entries, where they are mirror images in an axis the point lies on,
        # or duplicates: their distances are then THE SAME NUMBERS in either metric and the first index must win.  Any other exact tie
        # (a bisector point that float32 rounding put on the bisector of two unrelated entries) is loose: no float metric can be
        # expected to see it, either entry is right.
        self.exact_tie, loose, self.tie_sets = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool), {}
        apart = {"literal": np.zeros(n, dtype=bool), "two_fma": np.zeros(n, dtype=bool)}
        for s in range(0, n, 8192):
            p = pts[s:s + 8192]
            rows = np.arange(p.size)
            D = (p.real[:, None] - cx_[None, :]) ** 2 + (p.imag[:, None] - cy_[None, :]) ** 2
            close = (D <= D.min(axis=1)[:, None] * (1.0 + 2.0 ** -40)).sum(axis=1) > 1

            def fill(D_, sel, exactly=False):
                b = np.argmin(D_, axis=1)                                   # first index on exact ties
                r_ = np.arange(b.size)
                same = D_ == D_[r_, b][:, None]                             # the nearest entry and whatever ties with it exactly
                if exactly:                                                 # ... which rational arithmetic says, not 64 bits
                    for i in np.flatnonzero(same.sum(axis=1) > 1):
                        js = np.flatnonzero(same[i])
                        ex = [_exact_distance(complex(p[sel[i]]), complex(table_ops[j])) for j in js]
                        keep = [int(j) for j, e in zip(js, ex) if e == min(ex)]
                        b[i], same[i] = keep[0], False
                        same[i, keep] = True
                        if len(keep) > 1:
                            self.exact_tie[s + sel[i]] = True
                            if _same_numbers(p[sel[i]], table_ops[keep]):
                                self.tie_sets[int(s + sel[i])] = frozenset(keep)
                            else:
                                loose[s + sel[i]] = True
                db = D_[r_, b]
                Dx = np.where(same, np.inf, D_)                             # every other entry
                at = s + sel
                self.best[at], self.d_best[at] = b, db
                dn = Dx.min(axis=1)
                with np.errstate(invalid="ignore"):                         # (no other entry at all: dn = inf)
                    apart["literal"][at] = np.isinf(dn) | ((dn - db) > 4.0 * u * (dn + db))      # (4 u d grows with d: the nearest other entry decides)
                if dtype == "f32":
                    B = 3.0 * u * (self.half[None, :] + np.abs(p[sel])[:, None] * self.cabs[None, :])
                    apart["two_fma"][at] = (0.5 * (Dx - db[:, None]) - (B + B[r_, b][:, None])).min(axis=1) > 0

            fill(D[~close], rows[~close])
            if close.any():
                q = p[close]
                fill((q.real.astype(LD)[:, None] - cx_.astype(LD)[None, :]) ** 2 + (q.imag.astype(LD)[:, None] - cy_.astype(LD)[None, :]) ** 2,
                     rows[close], exactly=True)
        # decided[metric]: every entry that does not tie EXACTLY with the nearest one is farther by more than the two bounds -- the
        # label must be the reference's (a clear point, or an exact tie between entries that are clear of all others: first index)
        self.tied = np.zeros(n, dtype=bool)
        self.tied[list(self.tie_sets)] = True
        self.decided = {m: v & ~loose for m, v in apart.items() if m == "literal" or dtype == "f32"}
        self.clear = {m: v & ~self.tied for m, v in self.decided.items()}

    def _bound_fma(self, idx, lab):
        return 3.0 * self.u * (self.half[lab] + np.abs(self.pts[idx]) * self.cabs[lab])

    def wrong(self, labels, metric):
        """indices of the points whose label breaks rule (a) for this metric: on a decided point the reference's label; elsewhere
        an entry whose exact distance is within the two bounds of the minimum, and where it ties exactly with the minimum, the
        first index"""
        lab = np.asarray(labels, dtype=np.int64)
        assert lab.shape == self.best.shape and lab.min() >= 0 and lab.max() < self.table.size
        must = self.decided[metric]
        bad = must & (lab != self.best)
        idx = np.flatnonzero(~must & (lab != self.best))
        if idx.size:
            p, c = self.pts[idx], self.table[lab[idx]]
            dc = (p.real.astype(LD) - c.real.astype(LD)) ** 2 + (p.imag.astype(LD) - c.imag.astype(LD)) ** 2
            db = self.d_best[idx]
            if metric == "literal":
                ok = dc - db <= 4.0 * self.u * (dc + db)
            else:
                ok = 0.5 * (dc - db) <= self._bound_fma(idx, lab[idx]) + self._bound_fma(idx, self.best[idx])
            # an entry that ties exactly with the minimum, at a later index than the first of them
            ok &= ~np.array([int(l) in self.tie_sets.get(int(i), ()) for i, l in zip(idx, lab[idx])], dtype=bool)
            bad[idx[~ok]] = True
        return np.flatnonzero(bad)

    def slicer_clear(self):
        """square QAM: both level coordinates keep the slicers' rounding off every decision boundary (module docstring)"""
        M = self.table.size
        L = int(round(np.sqrt(M)))
        sc, off = LD(np.sqrt((M - 1) * 2.0 / 3.0)) * LD(0.5), LD(L - 1) * LD(0.5)
        ok = np.ones(self.pts.size, dtype=bool)
        for x, sgn in ((self.pts.real, 1.0), (self.pts.imag, -1.0)):
            t = sgn * x.astype(LD) * sc + off
            edge = np.clip(np.floor(t) + LD(0.5), LD(0.5), LD(L) - LD(1.5))      # the nearest of the boundaries 1/2 ... L - 3/2
            ok &= np.abs(t - edge) > 4.0 * self.u * (np.abs(x.astype(LD)) * sc + off + 1.0)
        return ok


class Case:
    """everything the two test modules share about one (table, arithmetic): built once, never modified"""

    def __init__(self, name, dtype):
        self.name, self.dtype = name, dtype
        self.table, self.kind, self.cert, self.walk_form = TABLES[name]
        self.M = self.table.size
        self.grid = tdg.build(self.table)
        seed = 11 + 7 * NAMES.index(name)
        self.pts = make_points(self.table, dtype, seed, self.cert, self.grid)
        self.ops = operands(self.table, dtype)
        self.ref = Reference(self.ops, self.pts, dtype)
        self.counts = cell_counts(self.pts, self.grid)
        self.lclass = length_class(self.counts)
        self.sure = certified(self.table, self.cert, self.pts, dtype)
        self.orders = make_orders(self.sure, self.lclass >= 2, seed + 1)
        for a in (self.pts, self.ops, self.counts, self.lclass, self.sure, self.ref.best) + tuple(self.orders.values()):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case(name, dtype):
    return Case(name, dtype)
