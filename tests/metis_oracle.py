"""NumPy restatement of the indoor system-level entry points (include/mcle.h: mcle_indoor_sinr, mcle_run_indoor_drops) --
TEST INFRASTRUCTURE, float64, written from the header's contract and the reference's
apps/metis_scenarios/simulate_metis_scenario.py / simulate_metis_scenario2.py; shares no code with pyphysim_amd.  The Philox
positions come from oracle/philox.py, so the file needs nothing outside the repository.

A configuration is a dict: n (rooms per side), dec, L (side length), wall_dB, model 'none' | 'general' | 'metis_ps7',
pl_n / pl_C / dist_scale (general), fc_MHz (PS7), tx, noise (linear), assoc 0 closest | 1 best channel, active 0 | 1.
"""
import os

import numpy as np

from oracle import philox

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g8_metis.npz")
DECIMATIONS = (1, 2, 4, 9)
MODEL_CODES = {"none": 0, "general": 1, "metis_ps7": 2}
# the heat map's four models in the fixture's order (3GPP and free space take km: dist_scale 1e-3 on metres)
FREE_SPACE_C = 10 * 2.0 * (np.log10(900.0 * 1e6) - 4.377911390697565)
HEAT_MODELS = (dict(model="none"), dict(model="general", pl_n=3.76, pl_C=128.1, dist_scale=1e-3),
               dict(model="general", pl_n=2.0, pl_C=float(FREE_SPACE_C), dist_scale=1e-3), dict(model="metis_ps7", fc_MHz=900.0))
# Philox cases of the GPU tests: (rooms per side, decimation, side, users, drops), 130 / 8 drops from first = 7
PHILOX_SEED, PHILOX_FIRST = 20261020, 7
PHILOX_CASES = [(4, 4, 10.0, 64, 130), (12, 1, 10.0, 100, 8)]
GAP_CAP = 0.05                # at most this share of a case's drops may be left out by the gap rule
ROOM_EDGE = 1e-9              # a user within ROOM_EDGE * L of a room boundary is left out


def load_fixture():
    return np.load(GOLDEN, allow_pickle=False)


def base_cfg(n, dec, L, wall_dB=5.0, tx=0.1, noise=1e-13, assoc=1, active=1, **model):
    cfg = dict(n=int(n), dec=int(dec), L=float(L), wall_dB=float(wall_dB), tx=float(tx), noise=float(noise), assoc=assoc,
               active=active, model="metis_ps7", pl_n=3.76, pl_C=128.1, dist_scale=1e-3, fc_MHz=900.0)
    cfg.update(model)
    return cfg


def cfg_from_row(row, **kw):
    """heat<i>_cfg / drop<i>_cfg of the fixture -> configuration (powers from dBm)."""
    n, dec, L, wall_dB, pt_dBm, noise_dBm = row[:6]
    return base_cfg(n, dec, L, wall_dB, tx=10.0 ** (pt_dBm / 10.0) / 1000.0, noise=10.0 ** (noise_dBm / 10.0) / 1000.0, **kw)


def engine_kwargs(cfg):
    """The configuration as keyword arguments of Engine.indoor_sinr / run_indoor_drops (active is the drops' own)."""
    return dict(rooms_per_side=cfg["n"], side_length=cfg["L"], ap_decimation=cfg["dec"], model=cfg["model"],
                assoc=cfg["assoc"], wall_loss_dB=cfg["wall_dB"], tx_power=cfg["tx"], noise_power=cfg["noise"],
                pl_n=cfg["pl_n"], pl_C=cfg["pl_C"], dist_scale=cfg["dist_scale"], fc_MHz=cfg["fc_MHz"])


# ---- geometry ----------------------------------------------------------------------------------------------------------
def axis_centres(L, n):
    shift = L * (n - 1) // 2
    return (L * (np.arange(n) - 0.5) - shift) + L / 2.0


def rooms(L, n):
    """complex [n, n], row 0 on top"""
    a = axis_centres(L, n)
    return a[None, :] + 1j * a[::-1, None]


def ap_rooms(n, dec):
    """(row, column) [A, 2] of the rooms with an AP, row-major"""
    r, c = np.indices((n, n))
    mask = {1: np.ones((n, n), bool), 2: (r + c) % 2 == 1, 4: (r % 2 == 1) & (c % 2 == 1), 9: (r % 3 == 1) & (c % 3 == 1)}[dec]
    return np.argwhere(mask)


def walls_reference(L, n, dec):
    """round(|Re| + |Im|) of (room - 1.0001 AP) / L, int [n n, A]"""
    rm = rooms(L, n)
    rc = ap_rooms(n, dec)
    aps = rm[rc[:, 0], rc[:, 1]]
    off = (rm.reshape(-1, 1) - 1.0001 * aps.reshape(1, -1)) / L
    return np.round(np.abs(off.real) + np.abs(off.imag)).astype(int)


def walls_manhattan(n, dec):
    r, c = np.indices((n, n))
    rc = ap_rooms(n, dec)
    return np.abs(r.reshape(-1, 1) - rc[None, :, 0]) + np.abs(c.reshape(-1, 1) - rc[None, :, 1])


def point_rooms(cfg, pos):
    """flat room index of every point (nearest centre, lowest index on a tie) and its margin: how much farther the
    second-nearest centre is (metres; twice the distance to the room boundary for a point near one)"""
    d = np.abs(rooms(cfg["L"], cfg["n"]).reshape(-1, 1) - np.reshape(pos, (1, -1)))
    idx = np.argmin(d, axis=0)
    if d.shape[0] == 1:
        return idx, np.full(idx.shape, np.inf)
    two = np.partition(d, 1, axis=0)[:2]
    return idx, two[1] - two[0]


# ---- gains ---------------------------------------------------------------------------------------------------------------
def path_loss_dB(cfg, d, walls):
    with np.errstate(divide="ignore"):
        if cfg["model"] == "none":
            pl = np.zeros_like(d)
        elif cfg["model"] == "general":
            pl = 10 * cfg["pl_n"] * np.log10(d * cfg["dist_scale"]) + cfg["pl_C"]
        else:
            f = 20 * np.log10(cfg["fc_MHz"] / 1e3 / 5.0)
            pl = np.where(walls == 0, 18.7 * np.log10(d) + 46.8 + f, 36.8 * np.log10(d) + 43.8 + f + 5 * (walls - 1))
    return np.maximum(pl, 0.0)


def gains(cfg, pos):
    """-> (g [P, A], distance [P, A]) for complex positions [P]"""
    pos = np.reshape(pos, -1)
    rm = rooms(cfg["L"], cfg["n"])
    rc = ap_rooms(cfg["n"], cfg["dec"])
    aps = rm[rc[:, 0], rc[:, 1]]
    d = np.abs(pos[:, None] - aps[None, :])
    walls = walls_manhattan(cfg["n"], cfg["dec"])[point_rooms(cfg, pos)[0]]
    g = 10.0 ** (-path_loss_dB(cfg, d, walls) / 10.0) * 10.0 ** (-walls * cfg["wall_dB"] / 10.0)
    return g, d


def associate(cfg, g, d):
    return np.argmax(g, axis=1) if cfg["assoc"] else np.argmin(d, axis=1)


def sinr_of(cfg, g, assoc, transmitting):
    """linear SINR [P]: transmitting = bool [A]"""
    rows = np.arange(g.shape[0])
    others = np.where(transmitting[None, :], g, 0.0)
    others[rows, assoc] = 0.0
    return cfg["tx"] * g[rows, assoc] / (cfg["tx"] * others.sum(axis=1) + cfg["noise"])


def gain_gap(g):
    """relative gap between the best and the second-best gain of every point (inf with one AP)"""
    if g.shape[1] == 1:
        return np.full(g.shape[0], np.inf)
    top = np.sort(g, axis=1)[:, -2:]
    return (top[:, 1] - top[:, 0]) / top[:, 1]


def heat_map(cfg, pos):
    """mcle_indoor_sinr: -> (sinr linear, assoc), shaped like pos"""
    g, d = gains(cfg, pos)
    a = associate(cfg, g, d)
    s = sinr_of(cfg, g, a, np.ones(g.shape[1], bool))
    return s.reshape(np.shape(pos)), a.reshape(np.shape(pos))


def heat_points(L, n, per_room=15):
    t = np.linspace(-(1.0 - 1.0 / per_room), 1.0 - 1.0 / per_room, per_room)
    off = (t[None, :] + 1j * t[::-1, None]) * L / 2.0
    return rooms(L, n)[:, :, None, None] + off[None, None]


# ---- drops ---------------------------------------------------------------------------------------------------------------
def philox_positions(seed, first, count, U, n, L):
    """complex [count, U]: user u of drop r takes uniforms 2 u and 2 u + 1 of STREAM_CHAN of realization first + r"""
    out = np.empty((count, U), dtype=complex)
    for r in range(count):
        u = philox.uniforms(seed, first + r, 2 * U, stream=philox.STREAM_CHAN)
        out[r] = (n * L) * (u[0::2] - 0.5) + 1j * ((n * L) * (u[1::2] - 0.5))
    return out


def drop(cfg, pos):
    """One drop (positions [U]) of mcle_run_indoor_drops -> dict: assoc, sinr (linear), sinr_dB, capacity, active_aps, load
    (users per AP [A]), gap (gain_gap), margin (point_rooms)."""
    g, d = gains(cfg, pos)
    a = associate(cfg, g, d)
    load = np.bincount(a, minlength=g.shape[1])
    on = load > 0 if cfg["active"] else np.ones(g.shape[1], bool)
    s = sinr_of(cfg, g, a, on)
    with np.errstate(divide="ignore"):
        db = 10.0 * np.log10(s)
    return dict(assoc=a, sinr=s, sinr_dB=db, capacity=np.log2(1.0 + s) / load[a], active_aps=int(on.sum()), load=load,
                gap=gain_gap(g) if cfg["assoc"] else gain_gap(1.0 / np.maximum(d, 1e-300) ** 2),
                margin=point_rooms(cfg, pos)[1])


def hist_slots(sinr_dB, lo, step, bins):
    """d_hist's slot of every value: 0 below lo, bins + 1 at or above the top, 1 + floor((s - lo) / step) otherwise"""
    s = np.asarray(sinr_dB, dtype=float).reshape(-1)
    with np.errstate(invalid="ignore"):
        t = np.floor((s - lo) / step) if bins else np.zeros_like(s)
    slot = np.where(t < bins, 1 + np.where(np.isfinite(t), t, 0).astype(np.int64), bins + 1)
    return np.where(s < lo, 0, slot)
