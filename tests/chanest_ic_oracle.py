"""NumPy restatement of one realization of the estimation-error pipeline with a gain per user and interference
cancellation (direct-link removal, ordered successive cancellation).  TEST INFRASTRUCTURE: written from the formulas of
include/mcle.h at mcle_run_chanest_ic, shares no code with the product; the draws and the plain estimator come from
tests/chanest_oracle.py, the transforms are np.fft.

    ic_estimates(seqs, Y, K, m, direct, mode, order=None, normalized=False) -> (est [n_users, n_rx, m Ne], order, margin)
    ic_realization(seed, r, cfg, gains, direct, mode, order=None)           -> (err [n_users], pow [n_users], order, margin)
"""
import numpy as np

import chanest_oracle as co


def fixed_order(n_users, direct, mode):
    """The order of the final estimates where no norm decides it."""
    if mode == 0:
        return list(range(n_users))
    return [direct] + [u for u in range(n_users) if u != direct]


def ic_estimates(seqs, Y, K, m, direct, mode, order=None, normalized=False):
    """seqs [n_users, Ne]; Y [n_rx, Ne].  order=None decides by the literal Frobenius norms of the first estimates (a tie:
    the higher index counts as stronger); a given order (direct user first) forces that sequence.  margin: the smallest
    norm[i] / norm[i + 1] - 1 over adjacent members of the literal ordering (inf where nothing is ordered)."""
    seqs = np.atleast_2d(seqs)
    n_users = seqs.shape[0]
    if mode == 0:
        est = np.stack([co.estimate(seqs[u], Y, K, m, normalized) for u in range(n_users)])
        return est, fixed_order(n_users, direct, 0), np.inf
    est = [None] * n_users
    est[direct] = co.estimate(seqs[direct], Y, K, m, normalized)
    R = Y - est[direct][:, ::m] * seqs[direct]
    others = [u for u in range(n_users) if u != direct]
    for u in others:
        est[u] = co.estimate(seqs[u], R, K, m, normalized)
    if mode == 1:
        return np.stack(est), fixed_order(n_users, direct, 1), np.inf
    norms = {u: np.linalg.norm(est[u]) for u in others}
    literal = sorted(others, key=lambda u: (-norms[u], -u))
    margin = min([norms[a] / norms[b] - 1.0 for a, b in zip(literal[:-1], literal[1:])], default=np.inf)
    seq = literal if order is None else [int(u) for u in order[1:]]
    assert sorted(seq) == others and (order is None or int(order[0]) == direct)
    for prev, u in zip(seq[:-1], seq[1:]):
        R = R - est[prev][:, ::m] * seqs[prev]
        est[u] = co.estimate(seqs[u], R, K, m, normalized)
    return np.stack(est), [direct] + seq, margin


def ic_realization(seed, r, cfg, gains, direct, mode, order=None):
    """cfg as chanest_oracle.chanest_draws takes it; gains: linear power gain per user."""
    seqs = np.atleast_2d(cfg["ref_seqs"])
    taps, noise = co.chanest_draws(seed, r, cfg)
    taps = taps * np.sqrt(np.asarray(gains, dtype=float))[:, None, None]
    H, Y = co.chanest_channels(taps, noise, cfg)
    est, order, margin = ic_estimates(seqs, Y, cfg["num_taps_to_keep"], cfg["size_multiplier"], direct, mode, order,
                                      cfg.get("normalized", False))
    err = np.array([(np.abs(est[u] - H[u]) ** 2).sum() for u in range(seqs.shape[0])])
    pw = np.array([(np.abs(H[u]) ** 2).sum() for u in range(seqs.shape[0])])
    return err, pw, order, margin
