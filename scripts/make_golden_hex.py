#!/usr/bin/env python3
"""Writes tests/golden/g9_hex.npz: the reference's own results for the hexagonal cluster geometry and the 'Random' / 'Symmetric
Far Away' user positioning of apps/comp_BD/simulate_comp.py -- what tests/test_hex_cpu.py, tests/test_gpu_hex.py,
tests/test_gpu_comp_drops.py and tests/hex_oracle.py are held to.

Drives the reference (darcamo/pyphysim v0.7.2) the way scripts/make_golden_metis.py does -- the stub modules of oracle/ref_shim
on sys.path, PYPHYSIM_REFERENCE naming its checkout, matplotlib on the Agg backend -- and holds none of it.  Arrays only.

Contents:
  geo_cells [7], geo_radii [2]; geo<k>_<i>_centres [K], geo<k>_<i>_vfirst / _vlast [6], geo<k>_<i>_radii = (cluster radius,
      external radius, cell height) for cluster size geo_cells[k] and cell radius geo_radii[i];
  wrap<i>_pos, wrap<i>_start [20]: the 19-cell cluster's per-cell position lists after create_wrap_around_cells, flattened;
  powers = (tx, noise, ext) linear;
  place<c>_cfg = (cells, users per cell, min_dist_ratio, cell radius, seeds), place<c>_seeds [S], and per seed:
      _attempts [S, K U]: candidates each user consumed; _uniforms: the uniforms the reference consumed, all seeds in a row
      (found by re-seeding and drawing up to the uniform the reference draws next; every user's position must be the last
      candidate of its run of pairs, bit for bit); _pos [S, K U] (complex); _dist [S, K U, K]
      (calc_dist_all_users_to_each_cell); _dcentre [S, K U]; _pl3gpp [S, K U, K], _plint3gpp [S, K U] (PathLoss3GPP1, linear,
      handle_small_distances_bool set; the app's pathloss and pathlossInt); for the small cases _plfree / _plintfree
      (PathLossFreeSpace); _sinr, _capacity [S, K U]: served by the user's own cell; _assoc [S, K U]: the cell of the largest
      3GPP gain, _assoc_ok: the two largest differ by more than 1e-3 relative; _sinr_best: served by _assoc.
      A seed is taken only if every candidate it consumed lies more than 1e-9 radii from every edge line and from the
      min-distance circle; the generator fails if more than 1 % of the seeds are rejected.
  border_app_pos [3] and its _dist, _dcentre, _pl3gpp, _plint3gpp: add_border_users([1, 2, 3], [210, -30, 90], 0.7) on the
      three-cell cluster of radius 1; border_more_cfg [n, 4] = (cells, cell id, angle, ratio), border_more_pos [n].

usage: PYPHYSIM_REFERENCE=/path/to/pyphysim python scripts/make_golden_hex.py
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("PYPHYSIM_REFERENCE")
OUT = os.path.join(REPO, "tests", "golden", "g9_hex.npz")

GEO_CELLS = [1, 2, 3, 4, 7, 13, 19]
GEO_RADII = [1.0, 0.35]
# (cells, users per cell, min_dist_ratio, cell radius, seeds)
PLACE_CASES = [(1, 1, 0.0, 1.0, 6), (3, 1, 0.0, 1.0, 8), (3, 1, 0.7, 1.0, 6), (3, 2, 0.3, 0.35, 5), (7, 1, 0.7, 0.35, 5),
               (7, 5, 0.0, 1.0, 4), (19, 1, 0.0, 1.0, 3), (19, 5, 0.7, 1.0, 2), (19, 13, 0.0, 0.35, 1)]
FREE_MAX_USERS = 35
EDGE, GAP = 1e-9, 1e-3
TX, NOISE, EXT = 2.9e-2, 10.0 ** (-116.4 / 10.0) / 1000.0, 1e-8
BORDER_MORE = [(1, 1, 0.0, 1.0), (1, 1, 90.0, 1.0), (1, 1, 180.0, 0.5), (1, 1, 270.0, 0.9), (1, 1, 30.0, 1.0), (1, 1, 45.0, 0.3),
               (7, 4, 135.0, 0.8), (7, 7, 200.0, 0.7), (7, 2, 300.0, 1.0), (7, 5, 355.0, 0.25), (3, 2, -30.0, 0.7), (3, 3, 61.0, 0.0)]


def build_fixture():
    if not REF:
        raise SystemExit("set PYPHYSIM_REFERENCE to a checkout of the reference")
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, os.path.join(REPO, "oracle", "ref_shim"))
    sys.path.insert(0, REF)
    sys.path.insert(0, REPO)
    np.int = int
    from pyphysim.cell import cell
    from pyphysim.channels import pathloss

    out = {"geo_cells": np.array(GEO_CELLS), "geo_radii": np.array(GEO_RADII), "powers": np.array([TX, NOISE, EXT])}
    for k, K in enumerate(GEO_CELLS):
        for i, r in enumerate(GEO_RADII):
            cl = cell.Cluster(cell_radius=r, num_cells=K)
            cells = list(cl)
            key = "geo%d_%d_" % (k, i)
            out[key + "centres"] = np.array([c.pos for c in cells])
            out[key + "vfirst"], out[key + "vlast"] = np.array(cells[0].vertices), np.array(cells[-1].vertices)
            out[key + "radii"] = np.array([cl.radius, cl.external_radius, cl.cell_height])
    for i, r in enumerate(GEO_RADII):
        cl = cell.Cluster(cell_radius=r, num_cells=19)
        cl.create_wrap_around_cells()
        lists = [np.atleast_1d(np.asarray(p, dtype=complex)) for p in cl._cell_pos]
        out["wrap%d_pos" % i] = np.concatenate(lists)
        out["wrap%d_start" % i] = np.concatenate([[0], np.cumsum([len(p) for p in lists])]).astype(np.int64)

    g3, fs = pathloss.PathLoss3GPP1(), pathloss.PathLossFreeSpace()
    g3.handle_small_distances_bool = fs.handle_small_distances_bool = True

    def scenario(cl):
        """The app's _create_users_channels up to the path loss (:192-213), for both models."""
        users = cl.get_all_users()
        dists = cl.calc_dist_all_users_to_each_cell()
        dcentre = np.array([cl.calc_dist(u) for u in users])
        res = dict(pos=np.array([u.pos for u in users]), dist=dists, dcentre=dcentre)
        for name, model in (("3gpp", g3), ("free", fs)):
            res["pl" + name] = model.calc_path_loss(dists.copy())
            res["plint" + name] = model.calc_path_loss(cl.external_radius - dcentre)
        return res

    def sinr(pl, plint, serving):
        n, K = pl.shape
        own = pl[np.arange(n), serving]
        other = np.array([sum(pl[q, c] for c in range(K) if c != serving[q]) for q in range(n)], dtype=float)
        return TX * own / (TX * other + EXT * plint + NOISE)

    def edge_margin(offset, r, ratio):
        """Distance, in radii, from a candidate (as an offset from the cell centre) to the nearest edge line of the hexagon or
        to the min-distance circle."""
        h = np.sqrt(3.0) * r / 2.0
        ax, ay = abs(offset.real), abs(offset.imag)
        margin = min(abs(h - ay), abs(2.0 * h - (np.sqrt(3.0) * ax + ay)) / 2.0)
        if ratio > 0:
            margin = min(margin, abs(abs(offset) - ratio * r))
        return margin / r

    seed, tried, rejected = 20261100, 0, 0
    for c, (K, U, ratio, r, n_seeds) in enumerate(PLACE_CASES):
        cl = cell.Cluster(cell_radius=r, num_cells=K)
        centres = [x.pos for x in cl]
        rows = []
        while len(rows) < n_seeds:
            seed += 1
            tried += 1
            np.random.seed(seed)
            cl.delete_all_users()
            cl.add_random_users(np.arange(1, K + 1), int(U), None, float(ratio))
            marker = np.random.random_sample()
            sc = scenario(cl)
            # which uniforms did it consume?  Re-seed and draw until the uniform the reference drew next; every pair is a
            # candidate, and a user's position is the first candidate of its run that the reference kept
            np.random.seed(seed)
            stream = np.random.random_sample(2 * 4096 * K * U)
            n_used = int(np.flatnonzero(stream == marker)[0])
            assert n_used % 2 == 0
            used = stream[:n_used]
            attempts, worst, i = [], np.inf, 0
            for q in range(K * U):
                t = 0
                while True:
                    cand = centres[q // U] + complex(2 * (used[2 * i] - 0.5) * r, 2 * (used[2 * i + 1] - 0.5) * r)
                    worst, i, t = min(worst, edge_margin(cand - centres[q // U], r, ratio)), i + 1, t + 1
                    if cand == sc["pos"][q]:
                        break
                attempts.append(t)
            assert 2 * i == n_used
            if worst <= EDGE:
                rejected += 1
                continue
            rows.append((seed, np.array(attempts), np.array(used), sc))
        key = "place%d_" % c
        out[key + "cfg"] = np.array([K, U, ratio, r, n_seeds])
        out[key + "seeds"] = np.array([x[0] for x in rows], dtype=np.int64)
        out[key + "attempts"] = np.stack([x[1] for x in rows]).astype(np.int32)
        out[key + "uniforms"] = np.concatenate([x[2] for x in rows])
        names = ["pos", "dist", "dcentre", "pl3gpp", "plint3gpp"] + (["plfree", "plintfree"] if K * U <= FREE_MAX_USERS else [])
        for name in names:
            out[key + name] = np.stack([x[3][name] for x in rows])
        own = np.arange(K * U) // U
        s = np.stack([sinr(x[3]["pl3gpp"], x[3]["plint3gpp"], own) for x in rows])
        out[key + "sinr"], out[key + "capacity"] = s, np.log2(1.0 + s)
        best = np.stack([np.argmax(x[3]["pl3gpp"], axis=1) for x in rows])
        out[key + "assoc"] = best.astype(np.int64)
        if K > 1:
            top = np.stack([np.sort(x[3]["pl3gpp"], axis=1)[:, -2:] for x in rows])
            out[key + "assoc_ok"] = top[..., 1] - top[..., 0] > GAP * top[..., 1]
        else:
            out[key + "assoc_ok"] = np.ones(best.shape, dtype=bool)
        out[key + "sinr_best"] = np.stack([sinr(x[3]["pl3gpp"], x[3]["plint3gpp"], b) for x, b in zip(rows, best)])
    assert rejected <= 0.01 * tried, "%d of %d seeds rejected by the edge rule" % (rejected, tried)
    print("seeds: %d tried, %d rejected by the %g edge rule" % (tried, rejected, EDGE))

    # the app's 'Symmetric Far Away' users (:172-185) through Grid, as the app builds its cluster
    grid = cell.Grid()
    grid.create_clusters(1, 3, 1.0)
    cl = grid.get_cluster_from_index(0)
    cl.delete_all_users()
    cl.add_border_users(np.arange(1, 4), np.array([210, -30, 90]), 0.7)
    sc = scenario(cl)
    for name in ("pos", "dist", "dcentre", "pl3gpp", "plint3gpp"):
        out["border_app_" + name] = sc[name]
    pts = []
    for K, cid, angle, ratio in BORDER_MORE:
        cl = cell.Cluster(cell_radius=0.35 if K == 7 else 1.0, num_cells=K)
        cl.add_border_users(int(cid), float(angle), float(ratio))
        pts.append(cl.get_all_users()[0].pos)
    out["border_more_cfg"] = np.array(BORDER_MORE)
    out["border_more_pos"] = np.array(pts)
    return out


if __name__ == "__main__":
    fixture = build_fixture()
    np.savez_compressed(OUT, **fixture)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(fixture), os.path.getsize(OUT)))
