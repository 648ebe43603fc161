"""The indoor scenario of the reference's apps/metis_scenarios/ (a much simplified METIS test case 2): one floor of n x n square
rooms, access points (APs) in room centres, users anywhere on the floor.

The geometry helpers are plain NumPy with the reference's names and results; positions are complex (x + 1j y, metres), room
(row, column) counts rows from the TOP of the floor.  The two simulations run on the GPU (Engine.indoor_sinr,
Engine.run_indoor_drops; csrc/pipeline_indoor.hip):

    perform_simulation_SINR_heatmap(scenario_params, power_params)      simulate_metis_scenario.py: 15 x 15 points per room,
                                                                        closest AP, every AP on, four path loss models
    perform_simulation(scenario_params, power_params, num_users, seed)  simulate_metis_scenario2.py: one random drop, best
                                                                        channel, unused APs off, METIS PS7

scenario_params: 'side_length', 'single_wall_loss_dB', 'num_rooms_per_side', 'ap_decimation'; power_params: 'Pt_dBm',
'noise_power_dBm'.  simulators.MetisDropSimulator is the Monte Carlo over drops.
"""
import math

import numpy as np

from .pathloss import PathLoss3GPP1, PathLossFreeSpace
from .util import dBm2Linear

POINTS_PER_ROOM = 15          # the heat map's discrete positions per room and axis


def _axis_centres(side_length, n):
    """Centre coordinate of room index 0 .. n-1 along one axis.  The shift is a FLOOR division, as in the reference: the grid
    is centred on the origin only when side_length (n - 1) / 2 is whole (side_length 7.5, n = 4: -11, -3.5, 4, 11.5)."""
    shift = side_length * (n - 1) // 2
    return (side_length * (np.arange(n) - 0.5) - shift) + side_length / 2.0


def calc_room_positions_square(side_length, num_rooms):
    """Centres of num_rooms (a perfect square) square rooms, row-major from the top-left room, as a flat complex array."""
    n = int(math.sqrt(num_rooms))
    if n * n != num_rooms:
        raise ValueError("num_rooms must be a perfect square number")
    axis = _axis_centres(side_length, n)
    return (axis[np.newaxis, :] + 1j * axis[::-1, np.newaxis]).reshape(-1)


AP_DECIMATIONS = (1, 2, 4, 9)


def ap_mask(n, decimation):
    """Boolean [n, n]: the rooms that hold an AP.  1: every room; 2: a checkerboard (row + column odd); 4: odd rows and odd
    columns; 9: rows and columns 1, 4, 7, ..."""
    r, c = np.indices((n, n))
    if decimation == 1:
        return np.ones((n, n), dtype=bool)
    if decimation == 2:
        return (r + c) % 2 == 1
    if decimation == 4:
        return (r % 2 == 1) & (c % 2 == 1)
    if decimation == 9:
        return (r % 3 == 1) & (c % 3 == 1)
    raise ValueError("Invalid decimation value: {0}".format(decimation))


def get_ap_positions(room_positions, decimation=1):
    """AP positions (flat, row-major order of their rooms) for room_positions [n, n]."""
    room_positions = np.asarray(room_positions)
    return room_positions[ap_mask(room_positions.shape[0], decimation)]


def calc_num_walls(side_length, room_positions, ap_positions):
    """Walls between every room and every AP, int [rooms, APs]: the real and imaginary room offsets in units of the side
    length, added and rounded.  The APs are pulled out by 1.0001 as in the reference; over the whole envelope of the GPU path
    the result is the Manhattan distance of the room indices (tests/test_metis_cpu.py)."""
    offset = (np.reshape(room_positions, (-1, 1)) - 1.0001 * np.reshape(ap_positions, (1, -1))) / side_length
    return np.round(np.abs(offset.real) + np.abs(offset.imag)).astype(int)


def prepare_sinr_array_for_color_plot(sinr_array, num_rooms_per_side, num_discrete_positions_per_room):
    """(n, n, d, d) -> the (n d, n d) image: room rows and point rows interleaved."""
    side = num_rooms_per_side * num_discrete_positions_per_room
    return np.swapaxes(sinr_array, 1, 2).reshape(side, side)


def heatmap_points(side_length, num_rooms_per_side, points_per_room=POINTS_PER_ROOM):
    """The heat map's user positions, complex [n, n, d, d]: in every room a d x d grid that stays 1 / d of the half side away
    from the walls, point rows from the top."""
    n, d = int(num_rooms_per_side), int(points_per_room)
    rooms = calc_room_positions_square(side_length, n * n).reshape(n, n)
    t = np.linspace(-(1.0 - 1.0 / d), 1.0 - 1.0 / d, d)
    offset = (t[np.newaxis, :] + 1j * t[::-1, np.newaxis]) * side_length / 2.0
    return rooms[:, :, np.newaxis, np.newaxis] + offset[np.newaxis, np.newaxis, :, :]


def heatmap_models():
    """The four path loss models of the heat map, in the order the reference returns them, as Engine keyword arguments (the
    two outdoor models take km: dist_scale 1e-3 on metres)."""
    fs, g3 = PathLossFreeSpace(), PathLoss3GPP1()
    return (dict(model="none"),
            dict(model="general", pl_n=g3.n, pl_C=g3.C, dist_scale=1e-3),
            dict(model="general", pl_n=fs.n, pl_C=fs.C, dist_scale=1e-3),
            dict(model="metis_ps7", fc_MHz=900.0))


def _engine_args(scenario_params, power_params):
    return dict(rooms_per_side=int(scenario_params["num_rooms_per_side"]), side_length=float(scenario_params["side_length"]),
                ap_decimation=int(scenario_params["ap_decimation"]),
                wall_loss_dB=float(scenario_params["single_wall_loss_dB"]),
                tx_power=float(dBm2Linear(power_params["Pt_dBm"])),
                noise_power=float(dBm2Linear(power_params["noise_power_dBm"])))


def perform_simulation_SINR_heatmap(scenario_params, power_params, engine=None, dtype="f64"):
    """SINR (dB) at 15 x 15 points of every room, each point served by its closest AP, every AP transmitting.  Returns four
    arrays (n, n, 15, 15): no path loss, 3GPP, free space, METIS PS7 (the wall losses apply to all four)."""
    from .engine import get_engine
    eng = engine if engine is not None else get_engine()
    args = _engine_args(scenario_params, power_params)
    points = heatmap_points(args["side_length"], args["rooms_per_side"])
    return tuple(eng.indoor_sinr(points, assoc="closest", dtype=dtype, **args, **m) for m in heatmap_models())


def perform_simulation(scenario_params, power_params, num_users=100, seed=0, drop=0, engine=None, dtype="f64"):
    """One drop of num_users users (realization `drop` of `seed`): best-channel association, the unused APs switched off, METIS
    PS7.  Returns (sinr_dB [num_users], capacity [num_users]); the capacity of an AP is shared equally among its users."""
    from .engine import get_engine
    eng = engine if engine is not None else get_engine()
    out = eng.run_indoor_drops(n_users=num_users, seed=seed, first=drop, count=1, model="metis_ps7", assoc="best_channel",
                               active=True, dtype=dtype, per_user=True, **_engine_args(scenario_params, power_params))
    return out["sinr_dB"][0], out["capacity"][0]
