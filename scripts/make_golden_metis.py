#!/usr/bin/env python3
"""Writes tests/golden/g8_metis.npz: the reference's own results for the indoor scenario of apps/metis_scenarios/ -- what
tests/test_metis_cpu.py, tests/test_gpu_metis.py and tests/metis_oracle.py are held to.

Drives the reference (darcamo/pyphysim v0.7.2) the way scripts/make_golden_quant_ia.py does -- the stub modules of
oracle/ref_shim on sys.path, PYPHYSIM_REFERENCE naming its checkout, matplotlib on the Agg backend -- and holds none of it.
Arrays only.

Contents:
  heat<i>_cfg = (rooms per side, ap_decimation, side_length, wall loss dB, Pt dBm, noise dBm), heat<i>_sinr [4, n, n, 15, 15]:
      perform_simulation_SINR_heatmap (no path loss, 3GPP, free space, METIS PS7);
  drop<i>_cfg = (rooms per side, ap_decimation, side_length, wall loss dB, Pt dBm, noise dBm, users, drops),
  drop<i>_seeds [drops], drop<i>_positions [drops, U] (complex), drop<i>_assoc, drop<i>_sinr_dB, drop<i>_capacity [drops, U]:
      simulate_metis_scenario2.perform_simulation fixes 100 users and returns no positions, so a drop is made from here: the
      users and their rooms and distances by tests/metis_oracle.py under np.random.seed, walls, path loss, association, SINR
      and capacity by the app's and the library's own functions; with 100 users the app's own call is checked to return
      the same two arrays.  A seed is taken only if every user's best and second-best gain differ by more than 1e-3
      relative (the next seed is tried otherwise), so comparing the association needs no gap rule;
  pl_*: path loss tables of PathLoss3GPP1, PathLossFreeSpace and PathLossMetisPS7 with handle_small_distances_bool set;
  noise_args [k, 2], noise_dBm [k]: calc_thermal_noise_power_dBm;
  geo_*: calc_room_positions_square, get_ap_positions, calc_num_walls, prepare_sinr_array_for_color_plot.

usage: PYPHYSIM_REFERENCE=/path/to/pyphysim python scripts/make_golden_metis.py
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("PYPHYSIM_REFERENCE", "/root/reference")
OUT = os.path.join(REPO, "tests", "golden", "g8_metis.npz")

WALL_DB, PT_DBM = 5.0, 20.0
HEAT_CASES = [(2, 1, 10.0), (4, 2, 10.0), (4, 4, 10.0), (3, 9, 10.0), (4, 1, 7.5)]          # (rooms per side, decimation, side)
DROP_CASES = [(12, 1, 10.0, 100, 1), (12, 4, 10.0, 100, 2), (5, 2, 7.0, 37, 2), (4, 4, 10.0, 64, 2), (3, 9, 10.0, 5, 1),
              (16, 1, 10.0, 256, 1), (2, 1, 10.0, 1, 1)]                                     # (..., users, drops)
GAP = 1e-3
PS7_LOS_D = [0.0, 0.01, 0.0196, 0.0197, 0.02, 0.5, 1.0, 7.0, 10.0, 150.0]


def build_fixture():
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, os.path.join(REPO, "oracle", "ref_shim"))
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, REPO)
    import metis_oracle as mo
    np.int = int
    from apps.metis_scenarios import simulate_metis_scenario as heat_app
    from apps.metis_scenarios import simulate_metis_scenario2 as drop_app
    from pyphysim.channels import pathloss
    from pyphysim.channels.noise import calc_thermal_noise_power_dBm
    from pyphysim.util.conversion import dB2Linear, dBm2Linear

    noise_dBm = calc_thermal_noise_power_dBm(25, 5e6)
    power = {"Pt_dBm": PT_DBM, "noise_power_dBm": noise_dBm}
    out = {}

    for i, (n, dec, L) in enumerate(HEAT_CASES):
        scen = {"side_length": L, "single_wall_loss_dB": WALL_DB, "num_rooms_per_side": n, "ap_decimation": dec}
        with np.errstate(divide="ignore"):
            maps = heat_app.perform_simulation_SINR_heatmap(scen, power)
        out["heat%d_cfg" % i] = np.array([n, dec, L, WALL_DB, PT_DBM, noise_dBm])
        out["heat%d_sinr" % i] = np.stack(maps)

    def one_drop(n, dec, L, U):
        """One drop of U users through the reference's own functions -> positions, gains [U, APs], association, SINR (dB),
        capacity.  The geometry that feeds them (users from two blocks of U uniforms, real parts first; the user's room;
        the distances) is the restatement's, tests/metis_oracle.py; with 100 users the app's own entry point must agree."""
        cfg = mo.base_cfg(n, dec, L)
        u = np.random.random_sample((2, U))
        pos = (n * L) * (u[0] - 0.5) + 1j * ((n * L) * (u[1] - 0.5))
        rooms = heat_app.calc_room_positions_square(L, n * n).reshape(n, n)
        aps = heat_app.get_ap_positions(rooms, dec)
        walls = heat_app.calc_num_walls(L, rooms, aps)[mo.point_rooms(cfg, pos)[0]]
        model = pathloss.PathLossMetisPS7()
        model.handle_small_distances_bool = True
        gains = model.calc_path_loss(np.abs(np.subtract.outer(pos, aps)), num_walls=walls) * dB2Linear(-walls * WALL_DB)
        assoc = drop_app.find_ap_assoc_best_channel(gains)
        tx_aps = np.unique(assoc)
        sinr_dB, cap = drop_app.simulate_for_a_given_ap_assoc(gains.take(tx_aps, axis=1), assoc, tx_aps,
                                                              dBm2Linear(PT_DBM), dBm2Linear(noise_dBm))
        return pos, gains, assoc, sinr_dB, cap

    seed = 20261020
    for i, (n, dec, L, U, drops) in enumerate(DROP_CASES):
        scen = {"side_length": L, "single_wall_loss_dB": WALL_DB, "num_rooms_per_side": n, "ap_decimation": dec}
        rows = []
        while len(rows) < drops:
            seed += 1
            np.random.seed(seed)
            pos, gains, assoc, sinr_dB, cap = one_drop(n, dec, L, U)
            if gains.shape[1] > 1:
                top = np.sort(gains, axis=1)[:, -2:]
                if np.any(top[:, 1] - top[:, 0] <= GAP * top[:, 1]):
                    continue
            if U == 100:                      # the app's own entry point draws the same users and returns the same figures
                np.random.seed(seed)
                app_sinr, app_cap = drop_app.perform_simulation(scen, power, plot_results_bool=False)
                assert np.array_equal(app_sinr, sinr_dB) and np.array_equal(app_cap, cap)
            rows.append((seed, pos, assoc, sinr_dB, cap))
        out["drop%d_cfg" % i] = np.array([n, dec, L, WALL_DB, PT_DBM, noise_dBm, U, drops])
        out["drop%d_seeds" % i] = np.array([r[0] for r in rows], dtype=np.int64)
        out["drop%d_positions" % i] = np.stack([r[1] for r in rows])
        out["drop%d_assoc" % i] = np.stack([r[2] for r in rows]).astype(np.int64)
        out["drop%d_sinr_dB" % i] = np.stack([r[3] for r in rows])
        out["drop%d_capacity" % i] = np.stack([r[4] for r in rows])

    # path loss tables (the small-distance rule set)
    g3, fs, fs2, ps7, ps7b = (pathloss.PathLoss3GPP1(), pathloss.PathLossFreeSpace(), pathloss.PathLossFreeSpace(),
                              pathloss.PathLossMetisPS7(), pathloss.PathLossMetisPS7())
    fs2.n, fs2.fc = 2.5, 2000.0
    ps7b.fc = 2600.0
    for m in (g3, fs, fs2, ps7, ps7b):
        m.handle_small_distances_bool = True
    d_km = np.array([0.0, 1e-5, 1e-4, 3.9e-4, 4e-4, 1e-3, 0.01, 0.1, 1.0, 10.0])
    with np.errstate(divide="ignore"):
        out["pl_d_km"] = d_km
        out["pl_3gpp_dB"] = g3.calc_path_loss_dB(d_km.copy())
        out["pl_3gpp_lin"] = g3.calc_path_loss(d_km.copy())
        out["pl_free_dB"] = fs.calc_path_loss_dB(d_km.copy())
        out["pl_free2_dB"] = fs2.calc_path_loss_dB(d_km.copy())
        out["pl_free_C"] = np.array([fs._C, fs2._C])
        out["pl_ps7_d"] = np.array(PS7_LOS_D)
        out["pl_ps7_los_dB"] = ps7.calc_path_loss_dB(np.array(PS7_LOS_D), num_walls=0)
        out["pl_ps7_los_lin"] = ps7.calc_path_loss(np.array(PS7_LOS_D), num_walls=0)
        walls = np.array([0, 1, 2, 5, 11])
        out["pl_ps7_walls"] = walls
        out["pl_ps7_grid_dB"] = ps7.calc_path_loss_dB(np.array(PS7_LOS_D)[:, np.newaxis] * np.ones((1, walls.size)),
                                                       num_walls=walls[np.newaxis, :])
        out["pl_ps7_2600_dB"] = np.stack([ps7b.calc_path_loss_dB(np.array(PS7_LOS_D), num_walls=int(w)) for w in (0, 3)])
    out["pl_3gpp_scalar_dB"] = np.array([g3.calc_path_loss_dB(float(d)) for d in d_km[1:]])
    out["pl_ps7_scalar_dB"] = np.array([ps7.calc_path_loss_dB(float(d), num_walls=2) for d in PS7_LOS_D[1:]])

    args = np.array([[25.0, 5e6], [0.0, 1e6], [-10.0, 20e6]])
    out["noise_args"] = args
    out["noise_dBm"] = np.array([calc_thermal_noise_power_dBm(t, bw) for t, bw in args])

    for j, (L, n) in enumerate([(7.5, 4), (10.0, 12), (7.0, 5), (10.0, 1)]):
        out["geo_rooms%d_cfg" % j] = np.array([L, n])
        out["geo_rooms%d" % j] = heat_app.calc_room_positions_square(L, n * n)
    rooms = heat_app.calc_room_positions_square(10.0, 49).reshape(7, 7)
    for dec in (1, 2, 4, 9):
        aps = heat_app.get_ap_positions(rooms, dec)
        out["geo_aps_dec%d" % dec] = aps
        out["geo_walls_dec%d" % dec] = heat_app.calc_num_walls(10.0, rooms, aps).astype(np.int64)
    img = np.arange(2 * 2 * 3 * 3, dtype=float).reshape(2, 2, 3, 3)
    out["geo_plot_in"] = img
    out["geo_plot_out"] = heat_app.prepare_sinr_array_for_color_plot(img, 2, 3)
    return out


if __name__ == "__main__":
    fixture = build_fixture()
    np.savez_compressed(OUT, **fixture)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(fixture), os.path.getsize(OUT)))
