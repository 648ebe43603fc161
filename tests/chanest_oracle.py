"""NumPy restatement of the CAZAC-based channel estimators and of one realization of the fused
estimation-error pipeline.  TEST INFRASTRUCTURE: written from the formulas, shares no code with the
product (pyphysim_amd/channel_estimation.py, csrc/kernels_chanest.hip).

    estimate          FFT_{m Ne}( IFFT_{Ne}(conj(r) y)[0 : K + 1] ), times Ne for a normalised sequence
                      -- the literal np.fft form (the depth oracle)
    estimate_pruned   the same as the two pruned DFTs the kernel evaluates
    estimate_occ      mean over the cover-code axis of cover[c] y[c], then `estimate` with m = 1
    chanest_realization(seed, r, cfg)
                      realization r under the draw ledger of DESIGN section 4 (oracle/philox.py)
"""
import numpy as np

from oracle import philox


def estimate(ref_seq, y, num_taps_to_keep, size_multiplier=2, normalized=False):
    """ref_seq [Ne]; y [..., Ne] -> [..., m Ne]."""
    r = np.asarray(ref_seq)
    ne = r.size
    h = np.fft.ifft(np.conj(r) * np.asarray(y), ne, axis=-1)[..., :num_taps_to_keep + 1]
    H = np.fft.fft(h, size_multiplier * ne, axis=-1)
    return H * ne if normalized else H


def estimate_pruned(ref_seq, y, num_taps_to_keep, size_multiplier=2, normalized=False):
    r = np.asarray(ref_seq)
    ne, m = r.size, size_multiplier
    n, t, k = np.arange(ne), np.arange(num_taps_to_keep + 1), np.arange(m * ne)
    z = np.conj(r) * np.asarray(y)
    h = (z[..., None, :] * np.exp(2j * np.pi * np.outer(t, n) / ne)).sum(-1) / ne
    H = (h[..., None, :] * np.exp(-2j * np.pi * np.outer(k, t) / (m * ne))).sum(-1)
    return H * ne if normalized else H


def estimate_occ(ref_seq_2d, cover, y, num_taps_to_keep, normalized=False):
    """ref_seq_2d [Nc, Ne] (row c = plain sequence times cover[c]); y [..., Nc, Ne] -> [..., Ne]."""
    cover = np.asarray(cover)
    r = np.asarray(ref_seq_2d)[0] * cover[0]
    y_mean = np.mean(np.asarray(y) * cover[:, None], axis=-2)
    return estimate(r, y_mean, num_taps_to_keep, 1, normalized)


def chanest_draws(seed, r, cfg):
    """(taps [n_users, n_rx, n_taps], noise [n_rx, Ne]) of realization r.
    cfg: dict(ref_seqs [n_users, Ne], n_rx, size_multiplier, num_taps_to_keep, noise_var, tap_power, tap_delay)."""
    seqs = np.atleast_2d(cfg["ref_seqs"])
    n_users, ne = seqs.shape
    n_rx, L = cfg["n_rx"], len(cfg["tap_delay"])
    power = np.asarray(cfg["tap_power"], dtype=float)
    power = power / power.sum()
    # taps: CN sample (u n_rx + a) L + i of the channel stream, times sqrt(p_i)
    taps = philox.cnormal(seed, r, n_users * n_rx * L, philox.STREAM_CHAN).reshape(n_users, n_rx, L) * np.sqrt(power)
    # noise: CN sample 2 ceil(Ne / 2) a + n of the noise stream, times sqrt(noise_var)
    half = (ne + 1) // 2
    noise = philox.cnormal(seed, r, n_rx * 2 * half, philox.STREAM_NOISE).reshape(n_rx, 2 * half)[:, :ne]
    return taps, noise * np.sqrt(cfg["noise_var"])


def chanest_channels(taps, noise, cfg):
    """True responses H [n_users, n_rx, m Ne] and the received comb Y [n_rx, Ne]."""
    seqs = np.atleast_2d(cfg["ref_seqs"])
    ne, m = seqs.shape[1], cfg["size_multiplier"]
    N = m * ne
    d = np.asarray(cfg["tap_delay"])
    H = taps @ np.exp(-2j * np.pi * np.outer(d, np.arange(N)) / N)           # [n_users, n_rx, N]
    Y = (H[:, :, ::m] * seqs[:, None, :]).sum(0) + noise
    return H, Y


def chanest_realization(seed, r, cfg):
    """-> (err [n_users], pow [n_users]): sum over antennas and subcarriers of |H^ - H|^2 and |H|^2."""
    seqs = np.atleast_2d(cfg["ref_seqs"])
    taps, noise = chanest_draws(seed, r, cfg)
    H, Y = chanest_channels(taps, noise, cfg)
    err, pw = np.empty(seqs.shape[0]), np.empty(seqs.shape[0])
    for u in range(seqs.shape[0]):
        est = estimate(seqs[u], Y, cfg["num_taps_to_keep"], cfg["size_multiplier"], cfg.get("normalized", False))
        err[u] = (np.abs(est - H[u]) ** 2).sum()
        pw[u] = (np.abs(H[u]) ** 2).sum()
    return err, pw
