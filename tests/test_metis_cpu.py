"""CPU: the host side of the indoor scenario against the reference's own results (tests/golden/g8_metis.npz, written by
scripts/make_golden_metis.py) -- the path loss classes and the thermal noise of pyphysim_amd, the geometry helpers of
pyphysim_amd/metis.py, the wall count as a Manhattan distance over the whole envelope of the GPU path, and the NumPy
restatement tests/metis_oracle.py (what the GPU tests compare the kernels with) on every heat-map and drop case.  No GPU."""
import numpy as np
import pytest

import metis_oracle as mo
from pyphysim_amd import metis
from pyphysim_amd.noise import calc_thermal_noise_power_dBm
from pyphysim_amd.pathloss import PathLoss3GPP1, PathLossFreeSpace, PathLossGeneral, PathLossMetisPS7

# the restatement against the reference: both are float64 NumPy, a gain is one log10 and one power of ten with an exponent
# below 30 in magnitude, a sum has at most 256 terms
ORACLE_RTOL = 1e-12


@pytest.fixture(scope="module")
def fx():
    return mo.load_fixture()


def small(model):
    model.handle_small_distances_bool = True
    return model


# ---- path loss and noise ---------------------------------------------------------------------------------------------------
def test_general_and_free_space_tables(fx):
    d = fx["pl_d_km"]
    g3, fs, fs2 = small(PathLoss3GPP1()), small(PathLossFreeSpace()), small(PathLossFreeSpace())
    fs2.n, fs2.fc = 2.5, 2000.0
    assert np.array_equal(g3.calc_path_loss_dB(d), fx["pl_3gpp_dB"])
    assert np.array_equal(g3.calc_path_loss(d), fx["pl_3gpp_lin"])
    assert np.array_equal(fs.calc_path_loss_dB(d), fx["pl_free_dB"])
    assert np.array_equal(fs2.calc_path_loss_dB(d), fx["pl_free2_dB"])
    assert [fs.C, fs2.C] == list(fx["pl_free_C"]) and (fs.n, fs.fc, fs2.n, fs2.fc) == (2.0, 900.0, 2.5, 2000.0)
    assert [g3.calc_path_loss_dB(float(x)) for x in d[1:]] == list(fx["pl_3gpp_scalar_dB"])
    # the clamp is on the path: 3GPP is negative below 0.39 m, and d = 0 gives 0 dB
    assert fx["pl_3gpp_dB"][0] == 0.0 and fx["pl_3gpp_dB"][3] == 0.0 and fx["pl_3gpp_dB"][4] > 0.0
    assert g3.calc_path_loss_dB(0.0) == 0.0 and g3.calc_path_loss(0.0) == 1.0


def test_metis_ps7_tables(fx):
    d, walls = fx["pl_ps7_d"], fx["pl_ps7_walls"]
    ps7, ps7b = small(PathLossMetisPS7()), small(PathLossMetisPS7(fc=2600.0))
    assert np.array_equal(ps7.calc_path_loss_dB(d, num_walls=0), fx["pl_ps7_los_dB"])
    assert np.array_equal(ps7.calc_path_loss(d, num_walls=0), fx["pl_ps7_los_lin"])
    assert np.array_equal(ps7.calc_path_loss_dB(d[:, None], num_walls=walls[None, :]), fx["pl_ps7_grid_dB"])
    assert np.array_equal(np.stack([ps7b.calc_path_loss_dB(d, num_walls=w) for w in (0, 3)]), fx["pl_ps7_2600_dB"])
    assert [ps7.calc_path_loss_dB(float(x), num_walls=2) for x in d[1:]] == list(fx["pl_ps7_scalar_dB"])
    # either side of the line-of-sight clamp at 900 MHz: 0.0196 m is clamped, 0.0197 m is not
    los = dict(zip(d.tolist(), fx["pl_ps7_los_dB"].tolist()))
    assert los[0.0] == los[0.01] == los[0.0196] == 0.0 and 0.0 < los[0.0197] < los[0.02]
    assert ps7.calc_path_loss_dB(0.0) == 0.0


def test_small_distances_and_negative_walls_are_errors():
    for model in (PathLoss3GPP1(), PathLossFreeSpace(), PathLossGeneral(2.0, 30.0)):
        with pytest.raises(RuntimeError):
            model.calc_path_loss_dB(1e-6)
        with pytest.raises(RuntimeError):
            model.calc_path_loss_dB(np.array([1.0, 1e-6]))
    ps7 = PathLossMetisPS7()
    with pytest.raises(RuntimeError):
        ps7.calc_path_loss_dB(0.01)
    with pytest.raises(RuntimeError):
        ps7.calc_path_loss_dB(np.array([5.0, 0.0]), num_walls=np.array([1, 0]))
    for walls in (-1, np.array([0, -2])):
        with pytest.raises(ValueError):
            ps7.calc_path_loss_dB(np.array([5.0, 6.0]), num_walls=walls)


def test_thermal_noise(fx):
    assert [calc_thermal_noise_power_dBm(t, bw) for t, bw in fx["noise_args"]] == list(fx["noise_dBm"])


# ---- geometry --------------------------------------------------------------------------------------------------------------
def test_geometry_helpers(fx):
    for j in range(4):
        L, n = fx["geo_rooms%d_cfg" % j]
        assert np.array_equal(metis.calc_room_positions_square(L, int(n) ** 2), fx["geo_rooms%d" % j])
    assert np.array_equal(metis.calc_room_positions_square(7.5, 16).real[:4], [-11.0, -3.5, 4.0, 11.5])     # the lopsided grid
    with pytest.raises(ValueError):
        metis.calc_room_positions_square(10.0, 12)
    rooms = metis.calc_room_positions_square(10.0, 49).reshape(7, 7)
    for dec in metis.AP_DECIMATIONS:
        aps = metis.get_ap_positions(rooms, dec)
        assert np.array_equal(aps, fx["geo_aps_dec%d" % dec])
        assert np.array_equal(metis.calc_num_walls(10.0, rooms, aps), fx["geo_walls_dec%d" % dec])
    with pytest.raises(ValueError):
        metis.get_ap_positions(rooms, 3)
    assert np.array_equal(metis.prepare_sinr_array_for_color_plot(fx["geo_plot_in"], 2, 3), fx["geo_plot_out"])


@pytest.mark.parametrize("L", [7.0, 7.5, 10.0])
def test_walls_are_the_manhattan_distance_over_the_envelope(L):
    """The kernel counts walls as |row - row_ap| + |col - col_ap|; the reference rounds offsets in units of the side length."""
    layouts = 0
    for n in range(1, 17):
        for dec in mo.DECIMATIONS:
            if len(mo.ap_rooms(n, dec)) == 0:
                continue
            layouts += 1
            want = mo.walls_reference(L, n, dec)
            assert np.array_equal(want, mo.walls_manhattan(n, dec)), (n, dec)
            rooms = metis.calc_room_positions_square(L, n * n).reshape(n, n)
            assert np.array_equal(metis.calc_num_walls(L, rooms, metis.get_ap_positions(rooms, dec)), want)
    assert layouts == 16 + 15 + 15 + 15          # one room per side holds an AP only with decimation 1


# ---- the restatement against the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(5))
def test_oracle_heat_maps(fx, case):
    row = fx["heat%d_cfg" % case]
    n, L = int(row[0]), float(row[2])
    pts = mo.heat_points(L, n)
    assert np.array_equal(pts, metis.heatmap_points(L, n))
    worst = 0.0
    for m, model in enumerate(mo.HEAT_MODELS):
        sinr, _ = mo.heat_map(mo.cfg_from_row(row, assoc=0, **model), pts)
        want = 10.0 ** (fx["heat%d_sinr" % case][m] / 10.0)
        worst = max(worst, float(np.max(np.abs(sinr - want) / want)))
    print("heat map %d: largest relative error of the linear SINR %.3g" % (case, worst))
    assert worst <= ORACLE_RTOL


@pytest.mark.parametrize("case", range(7))
def test_oracle_drops(fx, case):
    row = fx["drop%d_cfg" % case]
    cfg = mo.cfg_from_row(row, assoc=1, active=1)
    worst = 0.0
    for r, pos in enumerate(fx["drop%d_positions" % case]):
        out = mo.drop(cfg, pos)
        assert np.array_equal(out["assoc"], fx["drop%d_assoc" % case][r])
        assert out["active_aps"] == np.unique(fx["drop%d_assoc" % case][r]).size
        assert np.all(out["gap"] > 1e-3)                                   # the fixture's seeds were chosen for this
        want = 10.0 ** (fx["drop%d_sinr_dB" % case][r] / 10.0)
        worst = max(worst, float(np.max(np.abs(out["sinr"] - want) / want)),
                    float(np.max(np.abs(out["capacity"] - fx["drop%d_capacity" % case][r]) / fx["drop%d_capacity" % case][r])))
    print("drop case %d: largest relative error of SINR and capacity %.3g" % (case, worst))
    assert worst <= ORACLE_RTOL


def test_philox_positions_are_on_the_floor_and_reproducible():
    for n, dec, L, U, drops in mo.PHILOX_CASES:
        pos = mo.philox_positions(mo.PHILOX_SEED, mo.PHILOX_FIRST, 3, U, n, L)
        assert pos.shape == (3, U) and np.all(np.abs(pos.real) <= n * L / 2) and np.all(np.abs(pos.imag) <= n * L / 2)
        assert np.array_equal(pos[2], mo.philox_positions(mo.PHILOX_SEED, mo.PHILOX_FIRST + 2, 1, U, n, L)[0])
        assert len(np.unique(pos)) == pos.size


def test_hist_slots():
    s = np.array([-np.inf, -10.1, -10.0, -9.5, 0.0, 9.99, 10.0, 55.0])
    assert mo.hist_slots(s, -10.0, 0.5, 40).tolist() == [0, 0, 1, 2, 21, 40, 41, 41]
    assert mo.hist_slots(s, 0.0, 1.0, 0).tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
