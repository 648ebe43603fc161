"""mcle_bd_extint (WhiteningBD / EnhancedBD, csrc/bd_extint.hpp::bd_extint_lane) against the 50-digit oracle of
tests/bd_extint_oracle.py over its whole envelope: every geometry with K r <= 8, n_ext in {0, 1, r - 1, r, 8}, the input
classes of bd_extint_oracle.CLASSES, every variant (whitening; EnhancedBD with metric None, naive and fixed at every stream
count, capacity, candidates, per-user counts), at a batch of one full workgroup and a ragged one.  Everything goes through
Engine.bd_extint.

Bounds are measured, not chosen: for a predicate with error e against the 50 digits, e_gpu <= 8 max(e_np, eps scale), where
e_np is the error of the NumPy complex128 path (oracle/bd.py) on the same inputs -- for the reduction, on the kernel's own
Ms_bad (Engine.bd_extint(..., "enhanced", None, iPu = r), the same bd_solve call the lane makes).  Each test prints its worst
e_gpu / max(e_np, eps scale) per predicate before it asserts (pytest -s).  The scales (bd_extint_oracle) are each quantity's
size times its first-order sensitivity to one eps of the inputs, from the 50-digit quantities alone: ||W|| ||H_k|| ||Ms||
for whatever goes through W H_k Ms (a cancelled product on an ill-conditioned channel), lambda_max over the gap at the cut
for whatever depends on span(V[:, :ns]); NumPy's e_np often lands far below that on structured inputs (a rank-one
H_ext,k), so the floor eps scale is what keeps the bound from asking more than the arithmetic can give.

Unique cases are compared with the 50-digit solution -- the cuts of `ext_weak` included, whose gaps are 7e-9 .. 1e-6 of
lambda_max by construction and whose scale therefore carries lambda_max / gap (PM and PW of such a cut are held to about 1e-7).
Metric 3's Ns is compared with the 50-digit first maximum wherever every candidate's SINRs are unique and the best value leads
by more than the SINR bound lets two values move; a case that does not is counted and printed by name (none at the committed
seeds).  A stream cut through a repeated eigenvalue of Re_k (pe = 0, n_ext = 0,
rank(H_ext,k) < r - ns) has no unique answer and is held to bd_extint_oracle.properties() under the same kind of bound, and
its SINRs to the 50-digit SINR formula on the (MsPk, W) that metric 5 returned for the same cut.  Where noise_var = 0 and
the cut lies inside the null space of Re_k the exact SINR is infinite and the computed one is a rounding residue: only
noise_var = pe = 0 is asserted there (first candidate infinite, Ns = 1: the first maximum decides)."""
import math

import numpy as np
import pytest

import bd_extint_oracle as bo

pytestmark = pytest.mark.gpu

EPS = bo.EPS64
BOOLEAN = ("order", "phase_sign", "worder")


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class Report:
    """Collects e_gpu against 8 max(e_np, eps scale) per predicate, prints the worst ratios, asserts at the end."""

    def __init__(self, title):
        self.title, self.worst, self.fails = title, {}, []
        self.paths = {"compared": 0, "properties": 0, "ns_compared": 0, "ns_undecided": 0}
        self.undecided = []

    def check(self, where, gpu, ref):
        """gpu, ref: {name: (error, scale)} of the kernel's and of NumPy's solution."""
        for name, (e_gpu, scale) in gpu.items():
            if name in BOOLEAN:
                self.require(e_gpu == 0.0, "%s %s violated" % (where, name))
                continue
            base = max(float(ref[name][0]), EPS * float(scale))
            ratio = float(e_gpu) / base if base > 0 else (0.0 if e_gpu == 0 else float("inf"))
            self.worst[name] = max(self.worst.get(name, 0.0), ratio)
            if not ratio <= bo.FACTOR:
                self.fails.append("%s %s: e_gpu %.3g, e_np %.3g, eps*scale %.3g -> ratio %.3g"
                                  % (where, name, e_gpu, ref[name][0], EPS * scale, ratio))

    def require(self, cond, label):
        if not cond:
            self.fails.append(label)

    def finish(self):
        top = max(self.worst.values()) if self.worst else 0.0
        print("\nBDENV %s worst %.3f compared %d properties %d | %s | Ns_compared %d Ns_undecided %d %s" % (
            self.title, top, self.paths["compared"], self.paths["properties"],
            " ".join("%s=%.2f" % kv for kv in sorted(self.worst.items())),
            self.paths["ns_compared"], self.paths["ns_undecided"], "; ".join(self.undecided)))
        assert not self.fails, "%s (worst e_gpu / max(e_np, eps scale) = %.3g)\n  %s" % (self.title, top, "\n  ".join(self.fails[:40]))


def ns_mixed(K, r):
    return [1 + (k + 1) % r for k in range(K)]


def run_variants(engine, H, c):
    """Every variant of one parameter group -> {variant: result dict}."""
    K, r = c.K, c.r
    args = (K, r, c.n_ext, c.iPu, c.nv, c.pe)
    out = {}
    if c.nv > 0.0 or (c.n_ext >= r and c.pe > 0.0):          # else Re_k is singular by construction: refused or flagged
        out["whitening"] = engine.bd_extint(H, *args, "whitening")
    out["none"] = engine.bd_extint(H, *args, "enhanced", None)
    out["bad"] = engine.bd_extint(H, K, r, c.n_ext, float(r), c.nv, c.pe, "enhanced", None)
    for ns in range(1, r + 1):
        out["naive", ns] = engine.bd_extint(H, *args, "enhanced", "naive", num_streams=ns)
        out["fixed", ns] = engine.bd_extint(H, *args, "enhanced", "fixed", num_streams=ns)
        out["uni", ns] = engine.bd_extint(H, *args, "enhanced", "per_user", ns_user=[ns] * K)
    out["capacity"] = engine.bd_extint(H, *args, "enhanced", "capacity")
    out["candidates"] = engine.bd_extint(H, *args, "enhanced", "candidates")
    out["per_user"] = engine.bd_extint(H, *args, "enhanced", "per_user", ns_user=ns_mixed(K, r))
    return out


def expected_ns(variant, K, r):
    if variant in ("whitening", "none", "bad"):
        return [r] * K
    if variant == "per_user":
        return ns_mixed(K, r)
    if isinstance(variant, tuple):
        return [variant[1]] * K
    return None


def structure(rep, label, variant, res, n_unique, K, r, cls):
    """Tiled twins bit-equal, zero padding beyond Ns, flags, stream counts."""
    idx = np.arange(bo.BATCH) % n_unique
    for key in ("Ms", "W", "Ns", "skipped", "cand_sinr"):
        if res[key] is not None:
            rep.require(bits_equal(res[key], res[key][idx]), "%s %s: a tiled copy differs from its twin" % (label, key))
    Ns = res["Ns"]
    want = expected_ns(variant, K, r)
    if want is not None:
        rep.require(np.array_equal(Ns, np.tile(np.array(want, dtype=Ns.dtype), (bo.BATCH, 1))), "%s Ns %s" % (label, Ns[0]))
    rep.require(bool(np.all((Ns >= 1) & (Ns <= r))), "%s Ns out of range" % (label,))
    beyond = np.arange(r)[None, None, :] >= Ns[:, :, None]                     # [b, K, r]
    rep.require(not np.any(res["Ms"][np.broadcast_to(beyond[:, :, None, :], res["Ms"].shape)]), "%s Ms padding" % (label,))
    rep.require(not np.any(res["W"][np.broadcast_to(beyond[:, :, :, None], res["W"].shape)]), "%s W padding" % (label,))
    if res["cand_sinr"] is not None:
        upper = np.triu(np.ones((r, r), dtype=bool), 1)                        # row ns - 1 holds ns entries
        rep.require(not np.any(res["cand_sinr"][:, :, upper]), "%s cand_sinr padding" % (label,))
    flagged = cls == "singular" or (cls == "ext_dependent" and variant == "whitening")
    rep.require(bool(np.all(res["skipped"] == (1 if flagged else 0))), "%s skipped = %s" % (label, res["skipped"][:n_unique]))
    if not flagged:
        rep.require(bool(np.all(np.isfinite(res["Ms"])) and np.all(np.isfinite(res["W"]))), "%s output not finite" % (label,))


class Reducer:
    """The 50-digit and the NumPy candidates of one (case, user) on the kernel's Ms_bad, each computed once."""

    def __init__(self, c, ex, k, Msb_k):
        self.c, self.ex, self.k, self.Msb = c, ex, k, Msb_k
        self._mp, self._np = {}, {}

    @staticmethod
    def _key(rule, ns, r):
        return ("I" if (rule == "naive" or (rule == "auto" and ns == r)) else "V", ns)

    def exact(self, rule, ns):
        key = self._key(rule, ns, self.c.r)
        if key not in self._mp:
            M, W, s = bo.reduce(self.c, self.ex, self.k, self.Msb, "naive" if key[0] == "I" else "fixed", ns)
            self._mp[key] = (bo.to_ld(M), bo.to_ld(W), s)
        return self._mp[key]

    def numpy(self, rule, ns):
        key = self._key(rule, ns, self.c.r)
        if key not in self._np:
            self._np[key] = bo.np_candidate(self.c, self.k, self.Msb, "naive" if key[0] == "I" else "fixed", ns)
        return self._np[key]

    def is_cut(self, rule, ns):
        return self._key(rule, ns, self.c.r)[0] == "V"

    def unique(self, rule, ns):
        return not self.is_cut(rule, ns) or bo.cut_kind(self.ex, self.k, ns) != "degenerate"


def check_solution(rep, where, red, rule, ns, MsPk, W):
    """One reduced solution of the kernel: against the 50 digits where the cut is unique, else by its properties."""
    c, ex, k = red.c, red.ex, red.k
    M_np, W_np, _ = red.numpy(rule, ns)
    if red.unique(rule, ns):
        M_x, W_x, _ = red.exact(rule, ns)
        f = bo.cut_factor(ex, k, ns, c.r) if red.is_cut(rule, ns) else 1.0
        rep.check(where, bo.invariant_errors(ex, k, c.r, (MsPk, W), (M_x, W_x), f),
                  bo.invariant_errors(ex, k, c.r, (M_np, W_np), (M_x, W_x), f))
        rep.paths["compared"] += 1
    else:
        rep.paths["properties"] += 1
    cut = red.is_cut(rule, ns)
    rep.check(where, bo.properties(c, ex, k, red.Msb, MsPk, W, ns, cut), bo.properties(c, ex, k, red.Msb, M_np, W_np, ns, cut))


def sinr_meaningful(c, ex, k, ns, cut):
    """False where the exact SINR of the cut is infinite (noise_var = 0 and the cut inside the null space of Re_k)."""
    if c.nv > 0.0:
        return True
    return not (cut and ns <= c.r - (ex["ext_rank"][k] if c.pe > 0 else 0)) and c.pe > 0 and c.n_ext > 0


def rel(got, want, sens=1.0):
    """Largest relative error, per unit of `sens` (bd_extint_oracle.sinrs_of)."""
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    if not (np.all(np.isfinite(got)) and np.all(np.isfinite(want))):
        return float("inf")
    return float(np.max(np.abs(got - want) / np.abs(want) / sens))


@pytest.mark.parametrize("K,r,cls", bo.pairs())
def test_envelope(engine, K, r, cls):
    rep = Report("%s K=%d r=%d" % (cls, K, r))
    cs = bo.cases(cls, K, r)
    for key, members in bo.groups(cls, K, r).items():
        group = [cs[i] for i in members]
        c0 = group[0]
        res = run_variants(engine, bo.tiled(group), c0)
        for variant, out in res.items():
            structure(rep, "n_ext=%d %s" % (c0.n_ext, variant), variant, out, len(group), K, r, cls)
        for name in ("Ms", "W", "Ns"):                  # metric 4 returns metric 3's solution next to the candidates' SINRs
            rep.require(bits_equal(res["candidates"][name], res["capacity"][name]), "n_ext=%d candidates %s differs from capacity's" % (c0.n_ext, name))
        if cls == "singular":
            continue
        for j, i in enumerate(members):
            c, ex = cs[i], bo._exact_cached(cls, K, r, i)
            tag = "case %d n_ext=%d" % (i, c.n_ext)
            Ms_bad_np = bo.np_ms_bad(c)
            Ms_none_np, W_none_np, _ = bo.np_enhanced(c)
            whiten = "whitening" in res and all(R is not None for R in ex["Rinv"])
            if whiten:
                Ms_w_np, W_w_np, _ = bo.np_whitening(c)
            for k in range(K):
                u = "%s user %d" % (tag, k)
                cols = slice(k * r, (k + 1) * r)
                # the BD directions the reduction starts from
                Msb = np.ascontiguousarray(res["bad"]["Ms"][j, k])
                rep.check(u + " Ms_bad", bo.bd_validity(c, ex, k, Msb), bo.bd_validity(c, ex, k, Ms_bad_np[:, cols]))
                # metric None
                Mk, Wk = res["none"]["Ms"][j, k], res["none"]["W"][j, k]
                g = dict(bo.scaled_validity(c, ex, k, Mk))
                g.update(bo.inverse_checks(c, ex, k, Mk, Wk))
                n_ = dict(bo.scaled_validity(c, ex, k, bo.obd.canonical_columns(Ms_none_np[k])))
                n_.update(bo.inverse_checks(c, ex, k, Ms_none_np[k], W_none_np[k]))
                rep.check(u + " none", g, n_)
                rep.paths["compared"] += 1
                # whitening
                if whiten:
                    Mk, Wk = res["whitening"]["Ms"][j, k], res["whitening"]["W"][j, k]
                    keep = ("leak", "orth", "proj", "phase", "phase_sign")
                    g = {n: v for n, v in bo.scaled_validity(c, ex, k, Mk).items() if n in keep}
                    g.update(bo.whitening_checks(c, ex, k, Mk, Wk))
                    n_ = {n: v for n, v in bo.scaled_validity(c, ex, k, bo.obd.canonical_columns(Ms_w_np[k])).items() if n in keep}
                    n_.update(bo.whitening_checks(c, ex, k, Ms_w_np[k], W_w_np[k]))
                    rep.check(u + " whitening", g, n_)
                    rep.paths["compared"] += 1
                # the reduction, on the kernel's own Ms_bad
                red = Reducer(c, ex, k, Msb)
                for ns in range(1, r + 1):
                    for variant, rule in (("naive", "naive"), ("fixed", "fixed"), ("uni", "auto")):
                        o = res[variant, ns]
                        check_solution(rep, "%s %s/%d" % (u, variant, ns), red, rule, ns, o["Ms"][j, k][:, :ns], o["W"][j, k][:ns])
                ns = ns_mixed(K, r)[k]
                o = res["per_user"]
                check_solution(rep, u + " per_user", red, "auto", ns, o["Ms"][j, k][:, :ns], o["W"][j, k][:ns])
                # candidates: row ns - 1 = the SINRs with ns streams
                cand = res["candidates"]["cand_sinr"][j, k]
                all_unique, slack = True, []
                for ns in range(1, r + 1):
                    cut = red.is_cut("auto", ns)
                    row = cand[ns - 1, :ns]
                    if c.nv == 0.0 and c.pe == 0.0:
                        rep.require(ns > 1 or np.isposinf(row[0]), u + " cand: nv = pe = 0 must give an infinite first SINR")
                        all_unique = False
                    elif not sinr_meaningful(c, ex, k, ns, cut):
                        all_unique = False
                    elif bo.sinr_unique(ex, k, ns, r):
                        M_x, W_x, s_x = red.exact("auto", ns)
                        want = bo.to_ld(s_x)
                        sens = bo.sinrs_of(c, ex, k, M_x, W_x)[2] * (bo.cut_factor(ex, k, ns, r, upto=True) if cut else 1.0)
                        rep.check("%s cand/%d" % (u, ns), {"sinr": (rel(row, want, sens), 1.0)},
                                  {"sinr": (rel(red.numpy("auto", ns)[2], want, sens), 1.0)})
                        rep.paths["compared"] += 1
                        # what the bound lets sum log2(1 + sinr) move by: d log2(1 + s) = s / (1 + s) ds / s / ln 2
                        w = np.asarray(want, dtype=float)
                        slack.append(float(np.sum(w / (1.0 + w) * bo.FACTOR * EPS * sens)) / math.log(2.0))
                    else:                                   # the formula on what metric 5 returned for this cut
                        all_unique = False
                        M5, W5 = res["uni", ns]["Ms"][j, k][:, :ns], res["uni", ns]["W"][j, k][:ns]
                        want, sens, _ = bo.sinrs_of(c, ex, k, M5, W5)
                        Hred = c.big_H[k * r:(k + 1) * r, :K * r] @ M5
                        have = bo.obd.ebd_linear_sinrs(Hred, W5, np.asarray(ex["Re"][k], dtype=np.complex128))
                        rep.check("%s cand/%d (on metric 5's solution)" % (u, ns), {"sinr5": (rel(row, want, sens), 1.0)},
                                  {"sinr5": (rel(have, want, sens), 1.0)})
                        rep.paths["properties"] += 1
                # capacity: the first maximum.  Compared with the 50-digit argmax wherever every candidate's SINRs are unique
                # and the best value leads every other by more than the two may move inside the SINR bound (slack).
                o = res["capacity"]
                ns_gpu = int(o["Ns"][j, k])
                if all_unique:
                    best, vals = bo.first_max([red.exact("auto", ns)[2] for ns in range(1, r + 1)])
                    rep.require(bo.capacity_margin(vals) >= 1e-6 or r == 1, u + " capacity margin below 1e-6 (pick another seed)")
                    lead = min([float(vals[best] - vals[i]) - slack[best] - slack[i] for i in range(r) if i != best] or [1.0])
                    if lead > 0:
                        rep.require(ns_gpu == best + 1, "%s capacity Ns %d, 50 digits say %d" % (u, ns_gpu, best + 1))
                        rep.paths["ns_compared"] += 1
                    else:
                        rep.paths["ns_undecided"] += 1
                        rep.undecided.append(u)
                with np.errstate(over="ignore"):
                    own = [float(np.sum(np.log2(1.0 + cand[ns - 1, :ns]))) for ns in range(1, r + 1)]
                rep.require(ns_gpu == int(np.argmax(own)) + 1, "%s capacity Ns %d is not the first maximum of %s" % (u, ns_gpu, own))
                if c.nv == 0.0 and c.pe == 0.0:
                    rep.require(ns_gpu == 1, u + " nv = pe = 0: the first maximum is one stream")
                check_solution(rep, u + " capacity", red, "auto", ns_gpu, o["Ms"][j, k][:, :ns_gpu], o["W"][j, k][:ns_gpu])
    rep.finish()


def test_batch_independence(engine):
    """Batches of 1, 64, 65 and 70 give bit-equal rows for the same channel."""
    K, r = 2, 3
    cs = bo.cases("rayleigh", K, r)
    key, members = [(k, m) for k, m in bo.groups("rayleigh", K, r).items() if k[0] == r][0]
    c = cs[members[0]]
    rs = np.random.RandomState(77)
    H = (rs.randn(70, K * r, K * r + c.n_ext) + 1j * rs.randn(70, K * r, K * r + c.n_ext)) / math.sqrt(2.0)
    H[0] = c.big_H
    for method, metric in (("whitening", None), ("enhanced", "capacity"), ("enhanced", "candidates")):
        full = engine.bd_extint(H, K, r, c.n_ext, c.iPu, c.nv, c.pe, method, metric)
        for b in (1, 64, 65):
            part = engine.bd_extint(H[:b], K, r, c.n_ext, c.iPu, c.nv, c.pe, method, metric)
            for name in ("Ms", "W", "Ns", "skipped", "cand_sinr"):
                assert (full[name] is None and part[name] is None) or bits_equal(part[name], full[name][:b]), (method, metric, b, name)


def test_grid_stride_loop(engine):
    """K = 1, r = 1, n_ext = 0 at a batch of n_cu x 16 x 64 + 70: more lanes than the grid holds (grid_for caps it at 16
    workgroups per compute unit), so the loop takes a second trip.  The last 70 rows equal the same channels in a batch of 70
    bit for bit, and every row meets the 1 x 1 closed form Ms = sqrt(iPu), W = 1 / (h sqrt(iPu)).  Bound: the lane's chain
    from h to W is 16 roundings of at most eps / 2 each (norm, square root, two reciprocals, the scalings of the LQ and of
    the Jacobi column, the phase rotation, the power scaling, the complex product H Ms and the division by its square), so
    8 eps relative; Ms takes at most half of that chain."""
    n_cu = engine.device_info()["n_cu"]
    batch = n_cu * 16 * 64 + 70
    rs = np.random.RandomState(11)
    H = ((rs.randn(batch) + 1j * rs.randn(batch)) / math.sqrt(2.0)).reshape(batch, 1, 1)
    iPu = 1.75
    full = engine.bd_extint(H, 1, 1, 0, iPu, 0.05, 0.8, "enhanced", None)
    tail = engine.bd_extint(H[-70:], 1, 1, 0, iPu, 0.05, 0.8, "enhanced", None)
    for name in ("Ms", "W", "Ns", "skipped"):
        assert bits_equal(full[name][-70:], tail[name]), name
    assert not np.any(full["skipped"]) and np.all(full["Ns"] == 1)
    root = np.sqrt(np.longdouble(iPu))
    Ms, W = full["Ms"].reshape(batch).astype(np.clongdouble), full["W"].reshape(batch).astype(np.clongdouble)
    want_W = 1 / (H.reshape(batch).astype(np.clongdouble) * root)
    e_ms, e_w = float(np.max(np.abs(Ms - root) / root)), float(np.max(np.abs(W - want_W) / np.abs(want_W)))
    print("\nBDENV grid stride: batch %d, |Ms - sqrt(iPu)| / sqrt(iPu) = %.2f eps, |W - 1/(h sqrt(iPu))| / |W| = %.2f eps"
          % (batch, e_ms / bo.EPS64, e_w / bo.EPS64))
    assert e_ms <= 8 * bo.EPS64 and e_w <= 8 * bo.EPS64, (e_ms, e_w)


def test_pe_zero_and_n_ext_zero_keep_the_first_bd_directions(engine):
    """include/mcle.h: at pe = 0 or n_ext = 0, Re = nv I, V = I and the cut keeps the first ns BD directions -- 'fixed' and
    the per-user rule then return exactly what 'naive' returns for ns < r."""
    for cls, K, r in (("pe_zero", 2, 3), ("rayleigh", 2, 4), ("pe_zero", 1, 4)):
        cs = bo.cases(cls, K, r)
        for key, members in bo.groups(cls, K, r).items():
            c = cs[members[0]]
            if not (c.pe == 0.0 or c.n_ext == 0):
                continue
            H = np.stack([cs[i].big_H for i in members])
            args = (K, r, c.n_ext, c.iPu, c.nv, c.pe)
            for ns in range(1, r):
                naive = engine.bd_extint(H, *args, "enhanced", "naive", num_streams=ns)
                for other in (engine.bd_extint(H, *args, "enhanced", "fixed", num_streams=ns),
                              engine.bd_extint(H, *args, "enhanced", "per_user", ns_user=[ns] * K)):
                    assert bits_equal(naive["Ms"], other["Ms"]) and bits_equal(naive["W"], other["W"]), (cls, K, r, key, ns)


def test_whitening_without_noise_or_interference_is_flagged(engine):
    """include/mcle.h: WhiteningBD at noise_var = 0 is refused for n_ext < r; with n_ext >= r and pe = 0 the host cannot tell
    and the kernel flags every item (Re_k = 0), with finite output."""
    K, r = 2, 2
    rs = np.random.RandomState(5)
    H = (rs.randn(70, 4, 4 + 2) + 1j * rs.randn(70, 4, 6)) / math.sqrt(2.0)
    out = engine.bd_extint(H, K, r, 2, 1.75, 0.0, 0.0, "whitening")
    assert np.all(out["skipped"] == 1) and np.all(np.isfinite(out["Ms"])) and np.all(np.isfinite(out["W"]))
    ok = engine.bd_extint(H, K, r, 2, 1.75, 0.0, 0.8, "whitening")
    assert not np.any(ok["skipped"])


def _raw(engine, K, r, n_ext, method, metric, num_streams=0, ns_user=(0, 0, 0, 0), iPu=1.0, nv=0.1, pe=1.0, batch=1,
         cand=True, fill=None):
    """mcle_bd_extint as the C API takes it (the Python mirror refuses some of these before the library sees them)."""
    from ctypes import byref
    from pyphysim_amd import _lib
    cfg = _lib.BdExtIntCfg()
    cfg.num_users, cfg.n_ant_per_user, cfg.n_ext, cfg.method, cfg.metric, cfg.num_streams = K, r, n_ext, method, metric, num_streams
    for k in range(4):
        cfg.ns_user[k] = ns_user[k]
    cfg.iPu, cfg.noise_var, cfg.pe = iPu, nv, pe
    n = max(K * r, 1)
    rows = max(batch, 1)
    bufs = [engine.to_device(np.full(shape, fill if fill is not None else 0, dtype=dt)) for shape, dt in (
        ((rows, n, n + max(n_ext, 0)), np.complex128), ((rows, max(K, 1), n, max(r, 1)), np.complex128),
        ((rows, max(K, 1), max(r, 1), max(r, 1)), np.complex128), ((rows, max(K, 1)), np.int32),
        ((rows, max(K, 1), max(r, 1), max(r, 1)), np.float64), ((rows,), np.uint32))]
    rc = engine.lib.mcle_bd_extint(engine.ctx, byref(cfg), bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr,
                                   bufs[4].ptr if cand else None, bufs[5].ptr, batch)
    return rc, bufs


REFUSALS = {
    "K r > 8": dict(K=3, r=3, n_ext=1, method=1, metric=0),
    "K > 4": dict(K=5, r=1, n_ext=1, method=1, metric=0),
    "r > 4": dict(K=1, r=5, n_ext=1, method=1, metric=0),
    "r = 0": dict(K=2, r=0, n_ext=1, method=1, metric=0),
    "n_ext = 9": dict(K=2, r=2, n_ext=9, method=1, metric=0),
    "n_ext < 0": dict(K=2, r=2, n_ext=-1, method=1, metric=0),
    "method 2": dict(K=2, r=2, n_ext=1, method=2, metric=0),
    "metric 6": dict(K=2, r=2, n_ext=1, method=1, metric=6),
    "metric -1": dict(K=2, r=2, n_ext=1, method=1, metric=-1),
    "num_streams 0": dict(K=2, r=2, n_ext=1, method=1, metric=1, num_streams=0),
    "num_streams r + 1": dict(K=2, r=2, n_ext=1, method=1, metric=2, num_streams=3),
    "ns_user 0": dict(K=2, r=2, n_ext=1, method=1, metric=5, ns_user=(1, 0, 0, 0)),
    "ns_user r + 1": dict(K=2, r=2, n_ext=1, method=1, metric=5, ns_user=(3, 1, 0, 0)),
    "whitening, nv = 0, n_ext < r": dict(K=2, r=2, n_ext=1, method=0, metric=0, nv=0.0),
    "iPu = 0": dict(K=2, r=2, n_ext=1, method=1, metric=0, iPu=0.0),
    "nv < 0": dict(K=2, r=2, n_ext=1, method=1, metric=0, nv=-1.0),
    "pe < 0": dict(K=2, r=2, n_ext=1, method=1, metric=0, pe=-1.0),
    "metric 4 without d_cand_sinr": dict(K=2, r=2, n_ext=1, method=1, metric=4, cand=False),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(engine, name):
    rc, bufs = _raw(engine, fill=7, **REFUSALS[name])
    assert rc == -1 and engine.lib.mcle_last_error().decode()
    for b in bufs[1:]:
        assert np.all(b.get() == 7), "a refused call wrote to its outputs"


def test_refusals_reach_python_and_batch_zero_writes_nothing(engine):
    H = np.zeros((1, 9, 10), dtype=np.complex128)
    with pytest.raises(ValueError):
        engine.bd_extint(H, 3, 3, 1, 1.0, 0.1, 1.0, "enhanced", None)
    with pytest.raises(ValueError):
        engine.bd_extint(np.zeros((1, 4, 5), dtype=np.complex128), 2, 2, 1, 1.0, 0.0, 1.0, "whitening")
    with pytest.raises(ValueError):
        engine.bd_extint(np.zeros((1, 4, 5), dtype=np.complex128), 2, 2, 1, 1.0, 0.1, 1.0, "enhanced", "fixed", num_streams=3)
    rc, bufs = _raw(engine, K=2, r=2, n_ext=1, method=1, metric=4, batch=0, fill=7)
    assert rc == 0
    for b in bufs[1:]:
        assert np.all(b.get() == 7), "batch 0 wrote to its outputs"
    # a valid raw call, so that the harness above is known to reach the kernel
    rc, bufs = _raw(engine, K=1, r=1, n_ext=0, method=1, metric=0, iPu=4.0, fill=2.0)
    assert rc == 0 and abs(bufs[1].get().ravel()[0] - 2.0) <= 1e-15 and abs(bufs[2].get().ravel()[0] - 0.25) <= 1e-15
