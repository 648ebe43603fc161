"""50-digit reference of mcle_mu_link_stats (csrc/kernels_multiuser.hip: the covariance matrices and post-filter SINRs of the
K-user interference channel) and the shapes it is tested on.  TEST INFRASTRUCTURE; plain mpmath at mp.dps = 50, no
pyphysim_amd.  Restates oracle/multiuser.py (calc_Q, cov_ext_plus_noise, bkl_all_l, calc_sinr) in per-link and joint form:

    H_eff = big_H * sqrt(pathloss)                       G_j = H_kj F_j   (per link)   or   H_k[:, :sum Nt] F_j   (joint)
    Re_k  = pe X_k X_k^H + nv I                          Q_k = sum_{j != k} G_j G_j^H + Re_k
    B_kl  = sum_j G_j G_j^H + Re_k - g_kl g_kl^H         sinr_kl = |u_kl^H g_kl|^2 / |u_kl^H B_kl u_kl|

and returns with each quantity its MAGNITUDE, the same formula on absolute values (every product and sum taken without
cancellation).  Values leave as np.clongdouble / np.longdouble.

Bounds: |got - exact| <= c eps magnitude, c = the number of roundings on the longest accumulation chain of the kernel
that ends in the quantity, counted from csrc/kernels_multiuser.hip (chain()), not fitted:
    an entry of H_eff                    2 p        (square root and product; p = 1 with a path-loss matrix)
    G[r][s]   = sum_t H[r][t] F[t][s]    2 rows     (each complex multiply-add is two fused operations per component);
                                                    rows = Nt[j], or sum Nt in joint mode; plus 2 p from H_eff
    sum_s G[r][s] conj(G[c][s])          2 ns + 2 c_G        (both factors carry c_G)
    first / Q                            + K                 (one addition per transmitter)
    Re[r][c]                             2 n_ext + 4 p + 2   (products of two H_eff entries, times pe, plus nv)
    Q + Re, first + Re                   + 1
    B = (first + Re) - g g^H             + 3                 (one product, one subtraction, its operands' c_G inside c_first)
    aux = sum_r g[r] conj(u[r])          2 nr + c_G;   num = |aux|^2: 2 c_aux + 3
    den = |sum_r (sum_c B[r][c] u[c]) conj(u[r])|: c_B + 4 nr + 4
    sinr = num / den                     eps (c_num num_mag / den + num c_den den_mag / den^2) + 2 eps sinr
Each rounding is at most eps / 2 of the running magnitude, so c eps leaves a factor 2 for the two components of a complex
number."""
import mpmath as mp
import numpy as np

from mimo_ops_oracle import EPS, _H, to_ld, to_mp

mp.mp.dps = 50
EPS64 = EPS["f64"]
LD, CLD = np.longdouble, np.clongdouble


def chain(Nr, Nt, ns, n_ext, joint, has_pl, k):
    """The chain lengths for receiver k -> dict(G, Re, Q, B, num, den)."""
    K, p = len(Nr), 1 if has_pl else 0
    rows = sum(Nt) if joint else max(Nt)
    c_G = 2 * rows + 2 * p
    c_first = 2 * max(max(ns), 1) + 2 * c_G + K
    c_Re = 2 * n_ext + 4 * p + 2
    c_Q = max(c_first, c_Re) + 1
    c_B = c_Q + 3
    c_aux = 2 * Nr[k] + c_G
    return dict(G=c_G, Re=c_Re, Q=c_Q, B=c_B, num=2 * c_aux + 3, den=c_B + 4 * Nr[k] + 4)


def _blocks(Nr, Nt):
    return np.hstack([0, np.cumsum(Nr)]).astype(int), np.hstack([0, np.cumsum(Nt)]).astype(int)


def _sub(M, r0, r1, c0, c1):
    out = mp.matrix(r1 - r0, c1 - c0)
    for i in range(r0, r1):
        for j in range(c0, c1):
            out[i - r0, j - c0] = M[i, j]
    return out


def exact(big_H, Nr, Nt, F, U, nv=0.0, pe=1.0, n_ext=0, joint=False, pl=None):
    """One channel.  F[k] [rows, ns_k] (None or zero columns: no streams), U[k] [Nr_k, ns_k] or U None.
    -> list over receivers of dict(Q, Re, B [ns_k], sinr [ns_k] or None, and Q_mag, Re_mag, B_mag, sinr_err) where sinr_err is
    the propagated bound of the module docstring WITHOUT the factor eps."""
    K = len(Nr)
    cr, ct = _blocks(Nr, Nt)
    n_tx = int(ct[-1])
    big_H = np.asarray(big_H, dtype=np.complex128)
    Hm = to_mp(big_H)
    A = np.abs(big_H.astype(CLD)).astype(LD)
    if pl is not None:
        for i in range(Hm.rows):
            for j in range(Hm.cols):
                Hm[i, j] = Hm[i, j] * mp.sqrt(mp.mpf(float(pl[i, j])))
        A = A * np.sqrt(np.asarray(pl, dtype=LD))
    Fm = [None if (F is None or F[j] is None or np.asarray(F[j]).shape[-1] == 0) else to_mp(np.asarray(F[j])) for j in range(K)]
    Fa = [None if Fm[j] is None else np.abs(np.asarray(F[j]).astype(CLD)).astype(LD) for j in range(K)]
    out = []
    for k in range(K):
        nr = int(Nr[k])
        Hk = _sub(Hm, int(cr[k]), int(cr[k + 1]), 0, Hm.cols)
        Ak = A[cr[k]:cr[k + 1]]
        Re = mp.mpf(nv) * mp.eye(nr)
        Re_mag = LD(nv) * np.eye(nr, dtype=LD)
        if n_ext:
            X = _sub(Hk, 0, nr, n_tx, n_tx + n_ext)
            Re = Re + mp.mpf(pe) * (X * _H(X))
            Re_mag = Re_mag + LD(abs(pe)) * (Ak[:, n_tx:] @ Ak[:, n_tx:].T)
        first, Q = mp.zeros(nr), mp.zeros(nr)
        first_mag, Q_mag = np.zeros((nr, nr), dtype=LD), np.zeros((nr, nr), dtype=LD)
        Gk = Gk_mag = None
        for j in range(K):
            if Fm[j] is None:
                continue
            c0, c1 = (0, n_tx) if joint else (int(ct[j]), int(ct[j + 1]))
            G = _sub(Hk, 0, nr, c0, c1) * Fm[j]
            G_mag = Ak[:, c0:c1] @ Fa[j]
            GG, GG_mag = G * _H(G), G_mag @ G_mag.T
            first, first_mag = first + GG, first_mag + GG_mag
            if j != k:
                Q, Q_mag = Q + GG, Q_mag + GG_mag
            else:
                Gk, Gk_mag = G, G_mag
        res = dict(Q=to_ld(Q + Re), Q_mag=Q_mag + Re_mag, Re=to_ld(Re), Re_mag=Re_mag, B=[], B_mag=[], sinr=None, sinr_err=None)
        ns = 0 if Gk is None else Gk.cols
        ch = None
        if U is not None and ns:
            res["sinr"], res["sinr_err"] = np.zeros(ns, dtype=LD), np.zeros(ns, dtype=LD)
            Um = to_mp(np.asarray(U[k]))
            Ua = np.abs(np.asarray(U[k]).astype(CLD)).astype(LD)
            ch = chain(Nr, Nt, [0 if f is None else f.cols for f in Fm], n_ext, joint, pl is not None, k)
        for l in range(ns):
            g = _sub(Gk, 0, nr, l, l + 1)
            B = first + Re - g * _H(g)
            B_mag = first_mag + Re_mag + Gk_mag[:, l:l + 1] @ Gk_mag[:, l:l + 1].T
            res["B"].append(to_ld(B))
            res["B_mag"].append(B_mag)
            if ch is not None:
                u = _sub(Um, 0, nr, l, l + 1)
                num = abs((_H(u) * g)[0, 0]) ** 2
                den = abs((_H(u) * B * u)[0, 0])
                num_mag = (Ua[:, l] @ Gk_mag[:, l]) ** 2
                den_mag = Ua[:, l] @ B_mag @ Ua[:, l]
                s = num / den if den != 0 else mp.inf
                res["sinr"][l] = LD("inf") if s == mp.inf else to_ld([s])[0]
                num_l, den_l = to_ld([num])[0], to_ld([den])[0]
                res["sinr_err"][l] = (ch["num"] * num_mag / den_l + num_l * ch["den"] * den_mag / den_l ** 2 + 2 * res["sinr"][l]) \
                    if den != 0 else LD("inf")
        out.append(res)
    return out


# ---- the shapes ------------------------------------------------------------------------------------------------------
def _cn(rs, *shape):
    return (rs.randn(*shape) + 1j * rs.randn(*shape)) / np.sqrt(2.0)


SHAPES = {
    # name: Nr, Nt, ns, n_ext, joint, nv, pe, path loss?, batch (batch K = 1, 64, 65, 210 among them)
    "k1_one_item": dict(Nr=[2], Nt=[3], ns=[2], n_ext=0, joint=False, nv=0.1, pe=1.0, pl=False, batch=1),
    "k1_64_items": dict(Nr=[4], Nt=[1], ns=[1], n_ext=1, joint=False, nv=0.1, pe=0.7, pl=False, batch=64),
    "k1_65_items": dict(Nr=[1], Nt=[4], ns=[1], n_ext=8, joint=False, nv=0.2, pe=1.3, pl=True, batch=65),
    "k2_single_antennas_64_items": dict(Nr=[1, 3], Nt=[2, 1], ns=[1, 1], n_ext=1, joint=False, nv=0.05, pe=2.0, pl=False, batch=32),
    "k3_silent_user_210_items": dict(Nr=[2, 4, 1], Nt=[3, 1, 4], ns=[2, 0, 1], n_ext=8, joint=False, nv=0.1, pe=0.5, pl=True, batch=70),
    "k4_joint_16_tx": dict(Nr=[4, 4, 4, 4], Nt=[4, 4, 4, 4], ns=[4, 1, 2, 3], n_ext=1, joint=True, nv=0.01, pe=1.0, pl=True, batch=5),
    "k2_no_noise": dict(Nr=[2, 2], Nt=[2, 2], ns=[2, 1], n_ext=0, joint=False, nv=0.0, pe=1.0, pl=False, batch=3),
    "k2_dominant_stream": dict(Nr=[3, 3], Nt=[3, 3], ns=[2, 2], n_ext=1, joint=False, nv=0.1, pe=1.0, pl=False, batch=3),
    "k4_mixed_per_link": dict(Nr=[1, 2, 3, 4], Nt=[4, 3, 2, 1], ns=[1, 2, 2, 1], n_ext=8, joint=False, nv=0.3, pe=0.9, pl=True, batch=6),
    "k3_joint_silent": dict(Nr=[2, 1, 3], Nt=[1, 2, 2], ns=[1, 0, 2], n_ext=0, joint=True, nv=0.2, pe=1.0, pl=False, batch=4),
}
UNIQUE = 4                                       # distinct channels per shape; a batch is these tiled


def inputs(name):
    """-> dict(H [batch, ...], F list of [batch, rows, ns_k], U list of [batch, Nr_k, ns_k], pl or None, unique) for SHAPES[name].
    The path-loss matrix has one zero entry (a blocked link) and spans 1e-12 .. 1; `k2_dominant_stream` gives user 0's
    first stream 1e4 times the amplitude of everything else, so that B_0l = (sum) - g g^H cancels eight digits for l = 0."""
    sh = SHAPES[name]
    rs = np.random.RandomState(4200 + sorted(SHAPES).index(name))
    Nr, Nt, ns, K = sh["Nr"], sh["Nt"], sh["ns"], len(sh["Nr"])
    u = min(UNIQUE, sh["batch"])
    idx = np.arange(sh["batch"]) % u
    H = _cn(rs, u, sum(Nr), sum(Nt) + sh["n_ext"])
    rows = [sum(Nt) if sh["joint"] else Nt[k] for k in range(K)]
    F = [_cn(rs, u, rows[k], ns[k]) for k in range(K)]
    U = [_cn(rs, u, Nr[k], ns[k]) for k in range(K)]
    if name == "k2_dominant_stream":
        F[0][:, :, 0] *= 1e4
    pl = None
    if sh["pl"]:
        pl = 10.0 ** rs.uniform(-12, 0, size=H.shape[1:])
        pl[0, min(1, H.shape[2] - 1)] = 0.0
    return dict(H=np.ascontiguousarray(H[idx]), F=[f[idx] for f in F], U=[x[idx] for x in U], pl=pl, unique=u)


def numpy_reference(H, sh, F, U, pl):
    """oracle/multiuser.py on one channel -> per receiver (Q, Re, B list, sinr)."""
    from oracle import multiuser as omu
    Nr, Nt, K = sh["Nr"], sh["Nt"], len(sh["Nr"])
    He = omu.effective_big_H(H, pl)
    nt_rows = sum(Nt) if sh["joint"] else None
    Fz = [F[k] if F[k].shape[-1] else np.zeros((nt_rows or Nt[k], 0), dtype=complex) for k in range(K)]
    sinr = omu.calc_sinr(He, Nr, Nt, Fz, U, sh["nv"], sh["pe"], sh["joint"])
    out = []
    for k in range(K):
        Rek = omu.cov_ext_plus_noise(He, Nr, Nt, k, sh["pe"], sh["nv"])
        out.append((omu.calc_Q(He, Nr, Nt, k, Fz, sh["nv"], sh["pe"], sh["joint"]), Rek,
                    omu.bkl_all_l(He, Nr, Nt, k, Fz, Rek, sh["joint"]), sinr[k]))
    return out
