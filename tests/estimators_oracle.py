"""NumPy restatement of the LS / MMSE block-pilot estimators and of the fused estimation-error pipeline.  TEST INFRASTRUCTURE.

Written from the formulas (Fodor et al. 2014; include/mcle.h) and the draw ledger of DESIGN section 4; shares no code with
the product.  Model: Y = h s + N, Y [nr, P], s [nt, P], h [nr, nt].

    LS:    h^ = Y s^H (s s^H)^-1
    MMSE:  h^ = (noise_power I + P C)^-1 C (Y s^H) P / |s|^2                      (nt = 1)

Ledger (mcle-philox-v1, oracle/philox.py), realization r of `seed`:
    pilot phase of (t, p), random pilots:  uniform t P + p of stream 3;  s = sqrt(pilot_power) e^{2 pi j u}
    w[a][t]:                               CN sample t nr + a of stream 2;  h = alpha L w
    noise of (antenna a, pilot p):         CN sample 2 ceil(P / 2) a + p of stream 1, times sqrt(noise_power)
"""
import numpy as np

from oracle import philox


def ls_estimate(Y, s):
    """Y [..., nr, P]; s [nt, P] or [..., nt, P] -> [..., nr, nt]"""
    Y, s = np.asarray(Y, dtype=np.complex128), np.asarray(s, dtype=np.complex128)
    sh = np.conj(np.swapaxes(s, -1, -2))
    return (Y @ sh) @ np.linalg.inv(s @ sh)


def mmse_matrix(n_pilots, noise_power, C):
    C = np.asarray(C, dtype=np.complex128)
    return np.linalg.solve(noise_power * np.eye(C.shape[0]) + n_pilots * C, C)


def mmse_estimate(Y, s, noise_power, C):
    """Y [..., nr, P]; s [1, P] or [..., 1, P] -> [..., nr, 1]"""
    Y, s = np.asarray(Y, dtype=np.complex128), np.asarray(s, dtype=np.complex128)
    P = Y.shape[-1]
    sh = np.conj(np.swapaxes(s, -1, -2))
    return mmse_matrix(P, noise_power, C) @ (Y @ sh) * (P / np.real(s @ sh))


def theoretical_ls_mse(nr, noise_power, alpha, pilot_power, n_pilots):
    return nr * noise_power / (alpha ** 2 * pilot_power * n_pilots)


def theoretical_mmse_mse(nr, noise_power, alpha, pilot_power, n_pilots, C):
    C = np.asarray(C, dtype=np.complex128)
    return np.trace(C @ np.linalg.inv(np.eye(nr) + (alpha ** 2 * pilot_power * n_pilots / noise_power) * C))


# ---- ledger, vectorised over realizations ----------------------------------------------------------------
def _words(seed, reals, stream, n_blocks):
    """float64 words [R, n_blocks, 4]"""
    reals = np.asarray(reals, dtype=np.uint64).reshape(-1, 1)
    return philox.blocks(seed, reals, stream, np.arange(n_blocks, dtype=np.uint64).reshape(1, -1)).astype(np.float64)


def cn_samples(seed, reals, stream, n):
    """CN(0, 1) samples 0 .. n-1 of every realization: [R, n]"""
    w = _words(seed, reals, stream, (n + 1) // 2)
    x0 = w[:, :, [0, 2]].reshape(len(w), -1)[:, :n]
    x1 = w[:, :, [1, 3]].reshape(len(w), -1)[:, :n]
    rad = np.sqrt(-np.log((x0 + 0.5) * 2.0 ** -32))
    ang = 2.0 * np.pi * (x1 * 2.0 ** -32)
    return rad * (np.cos(ang) + 1j * np.sin(ang))


def uniform_samples(seed, reals, stream, n):
    w = _words(seed, reals, stream, (n + 3) // 4)
    return w.reshape(len(w), -1)[:, :n] * 2.0 ** -32


def default_cfg(**kw):
    cfg = dict(nr=3, nt=1, n_pilots=10, pilot_power=1.0, noise_power=0.5, alpha=1.0, pilots=None, L=None, cov=None)
    cfg.update(kw)
    return cfg


def pilot_mse(seed, reals, cfg):
    """The pipeline's realizations `reals` of `seed`: dict of s [R, nt, P], h [R, nr, nt], Y [R, nr, P], est_ls, est_mmse
    (None without cfg['cov']), and the outputs err_ls, err_mmse, pow [R]."""
    reals = np.atleast_1d(np.asarray(reals, dtype=np.uint64))
    R, nr, nt, P = len(reals), cfg["nr"], cfg["nt"], cfg["n_pilots"]
    if cfg["pilots"] is None:
        u = uniform_samples(seed, reals, philox.STREAM_PHASE, nt * P).reshape(R, nt, P)
        s = np.sqrt(cfg["pilot_power"]) * np.exp(2j * np.pi * u)
    else:
        s = np.broadcast_to(np.asarray(cfg["pilots"], dtype=np.complex128).reshape(1, nt, P), (R, nt, P))
    w = np.swapaxes(cn_samples(seed, reals, philox.STREAM_CHAN, nt * nr).reshape(R, nt, nr), 1, 2)
    L = np.eye(nr) if cfg["L"] is None else np.asarray(cfg["L"], dtype=np.complex128)
    h = cfg["alpha"] * (L @ w)
    Y = h @ s
    if cfg["noise_power"] != 0:
        half = (P + 1) // 2
        n = cn_samples(seed, reals, philox.STREAM_NOISE, 2 * half * nr).reshape(R, nr, 2 * half)[:, :, :P]
        Y = Y + np.sqrt(cfg["noise_power"]) * n
    est_ls = ls_estimate(Y, s)
    out = dict(s=s, h=h, Y=Y, est_ls=est_ls, est_mmse=None, err_mmse=None,
               err_ls=np.sum(np.abs(est_ls - h) ** 2, axis=(1, 2)), pow=np.sum(np.abs(h) ** 2, axis=(1, 2)))
    if cfg["cov"] is not None:
        out["est_mmse"] = mmse_estimate(Y, s, cfg["noise_power"], cfg["cov"])
        out["err_mmse"] = np.sum(np.abs(out["est_mmse"] - h) ** 2, axis=(1, 2))
    return out


def pilot_mse_realization(seed, r, cfg):
    """One realization: the dict of pilot_mse with the leading axis dropped."""
    return {k: (None if v is None else v[0]) for k, v in pilot_mse(seed, [r], cfg).items()}


# ---- exact moments (nt = 1) ------------------------------------------------------------------------------
def mmse_error_moments(cfg):
    """(mean, variance) of err_mmse: with B = P (noise_power I + P cov)^-1 cov and C_h = alpha^2 L L^H, the error B h + B n' - h
    (n' of covariance noise_power / (P pilot_power) I) is circular Gaussian of covariance
    S = (B - I) C_h (B - I)^H + noise_power / (P pilot_power) B B^H; mean = tr S, variance = tr S^2."""
    nr, P = cfg["nr"], cfg["n_pilots"]
    L = np.eye(nr) if cfg["L"] is None else np.asarray(cfg["L"], dtype=np.complex128)
    Ch = cfg["alpha"] ** 2 * (L @ L.conj().T)
    B = P * mmse_matrix(P, cfg["noise_power"], cfg["cov"])
    D = B - np.eye(nr)
    S = D @ Ch @ D.conj().T + cfg["noise_power"] / (P * cfg["pilot_power"]) * (B @ B.conj().T)
    return float(np.real(np.trace(S))), float(np.real(np.trace(S @ S)))


def ls_error_moments(cfg):
    """(mean, variance) of err_ls at nt = 1: nr i.i.d. exponentials of mean noise_power / (P pilot_power)"""
    mean = cfg["nr"] * cfg["noise_power"] / (cfg["n_pilots"] * cfg["pilot_power"])
    return mean, mean ** 2 / cfg["nr"]


def toeplitz_cov(nr, rho, scale=1.0):
    d = np.arange(nr)[:, None] - np.arange(nr)[None, :]
    return scale * (float(rho) ** np.abs(d) if rho else (d == 0).astype(float)) * np.exp(0.3j * d)


def ledger_case(name):
    """Cases A and B of the ledger statistic: nt = 1, pilot_power 1.5, noise_power 0.5, alpha 0.7, random pilots"""
    base = dict(nt=1, pilot_power=1.5, noise_power=0.5, alpha=0.7)
    if name == "A":
        return default_cfg(nr=3, n_pilots=10, L=None, cov=0.49 * np.eye(3), **base)
    C0 = toeplitz_cov(16, 0.9)
    return default_cfg(nr=16, n_pilots=8, L=np.linalg.cholesky(C0), cov=0.49 * C0, **base)
