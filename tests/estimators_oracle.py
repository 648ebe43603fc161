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


# ---- the shape envelope of the pipeline (tests/test_estimators_envelope_cpu.py, tests/test_gpu_estimators_envelope.py) ----
ENVELOPE_SEED = 20261018
ENVELOPE_COUNT = 37                     # tiles of 16: two and a tail of 5; of 8, 4 and 2: a tail of 5, 1 and 1
ENVELOPE_FIRSTS = (0, 2 ** 32 - 5)      # the second range crosses 2^32 after five realizations


def envelope_reals(first):
    return np.arange(ENVELOPE_COUNT, dtype=np.uint64) + np.uint64(first)


def dft_pilots(nt, P, power):
    """The first nt rows of the P-point DFT matrix times sqrt(power): s s^H = P power I"""
    return np.sqrt(power) * np.exp(-2j * np.pi * np.outer(np.arange(nt), np.arange(P)) / P)


def random_phase_pilots(nt, P, power, seed=3):
    return np.sqrt(power) * np.exp(2j * np.pi * np.random.RandomState(seed).rand(nt, P))


def _envelope_case(nr, nt, P, pilots, rho_L, cov, noise_power):
    """pilots: None (drawn), 'dft' or 'phases'; rho_L: the rho of L = chol(toeplitz_cov(nr, rho)), or None; cov: None, 'eye'
    (0.49 I) or the rho of 0.49 toeplitz_cov(nr, rho)"""
    s = None if pilots is None else (dft_pilots if pilots == "dft" else random_phase_pilots)(nt, P, 1.5)
    L = None if rho_L is None else np.linalg.cholesky(toeplitz_cov(nr, rho_L))
    C = None if cov is None else 0.49 * (np.eye(nr) if cov == "eye" else toeplitz_cov(nr, cov))
    return default_cfg(nr=nr, nt=nt, n_pilots=P, pilot_power=1.5, noise_power=noise_power, alpha=0.7, pilots=s, L=L, cov=C)


ENVELOPE_CASES = {
    "a": _envelope_case(1, 1, 1, None, None, "eye", 2.0),         # smallest shape, 15 padded rows
    "b": _envelope_case(15, 1, 2, None, 0.9, 0.9, 0.5),           # one padded row
    "c": _envelope_case(17, 1, 9, "phases", 0.9, 0.9, 0.5),       # second row tile nearly empty, odd P
    "d": _envelope_case(32, 1, 255, None, None, "eye", 16.0),     # largest odd P; complex128 above the default LDS limit
    "e": _envelope_case(113, 1, 16, None, 0.7, 0.7, 1.0),         # first nr whose complex128 LDS passes 63 KiB
    "f": _envelope_case(128, 1, 256, None, 0.7, 0.7, 16.0),       # the nt = 1 maximum: above the limit in both arithmetics
    "g": _envelope_case(128, 8, 256, None, 0.7, None, 16.0),      # the overall LDS maximum; L with nt = 8
    "h": _envelope_case(5, 4, 4, "dft", 0.9, None, 0.5),          # NTP = 4 unpadded, P = nt, L with nt > 1
    "i": _envelope_case(33, 5, 12, None, 0.9, None, 0.5),         # NTP = 8 with 3 padded columns, L
    "j": _envelope_case(16, 6, 7, "phases", None, None, 0.5),     # fixed pilots with nt > 1, nr = nrp
    "k": _envelope_case(64, 7, 64, None, 0.7, None, 4.0),         # NTP = 8 with 1 padded column, L, four row tiles
    "l": _envelope_case(3, 2, 3, "phases", 0.9, None, 0.5),       # 8 realizations per wavefront, L
}
LDS_BUDGET = 160 * 1024
LDS_ATTRIBUTE_ABOVE = 63 * 1024         # a launch above this raises the kernel's dynamic-LDS limit first
MAX_NR, MAX_NT, MAX_PIPELINE_PILOTS = 128, 8, 256


def ntp_of(nt):
    """nt rounded up to a power of two: the kernel instance, 16 / ntp realizations per wavefront"""
    ntp = 1
    while ntp < nt:
        ntp *= 2
    return ntp


def pilot_mse_lds(nr, nt, P, random_pilots, real_bytes):
    """Restatement of the launcher's LDS size per wavefront: the inverse Gram matrices (complex f64), four [nrp][16] real
    planes, the pilots"""
    nrp = (nr + 15) // 16 * 16
    ng = 16 // ntp_of(nt) if random_pilots else 1
    return ng * nt * nt * 16 + 4 * nrp * 16 * real_bytes + ng * nt * P * 2 * real_bytes


def envelope_lds(cfg, dtype):
    return pilot_mse_lds(cfg["nr"], cfg["nt"], cfg["n_pilots"], cfg["pilots"] is None, 8 if dtype == "f64" else 4)


def envelope_kernel_name(cfg, dtype):
    return "pilot_mse %s b%d %s%s" % (dtype, 16 // ntp_of(cfg["nt"]), "ls+mmse" if cfg["cov"] is not None else "ls",
                                      " gl" if cfg["L"] is not None else "")


def pilot_mse_per_trip(cfg, dtype, n_cu):
    """Realizations one pass of the pipeline's grid takes with grid_oversub = 1: min(8, 160 KiB / LDS) one-wavefront
    workgroups per compute unit, 16 / ntp realizations each"""
    per_cu = max(1, min(8, LDS_BUDGET // envelope_lds(cfg, dtype)))
    return n_cu * per_cu * (16 // ntp_of(cfg["nt"]))
