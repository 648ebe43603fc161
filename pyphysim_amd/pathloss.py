"""Host-only path loss models (reference channels/pathloss.py:669-816 PathLossGeneral, :818-975 PathLossFreeSpace, :977-1020
PathLoss3GPP1, :1022-1342 PathLossMetisPS7): what the CoMP application's power rule needs (apps/comp_BD/simulate_comp.py:629-659
-- the loss at the cell border fixes the transmit power for a wanted SNR there) and what the indoor scenario of
apps/metis_scenarios/ evaluates per (user, access point) pair (pyphysim_amd/metis.py; on the GPU csrc/pipeline_indoor.hip).
The distances come from the user, or from the hexagonal cluster of pyphysim_amd/cell.py (on the GPU csrc/pipeline_hex.hip).

    >>> pl = PathLoss3GPP1()
    >>> pl.calc_path_loss(1)
    1.5488166189124858e-13
    >>> pl.calc_path_loss_dB(1)
    128.1
    >>> pl.which_distance_dB(130)
    1.1233935211892188
    >>> PathLossMetisPS7().calc_path_loss_dB(10.0, num_walls=2)
    70.70545010206611
"""
import math

import numpy as np


def _clamp_small_distances(PL, allowed):
    """A negative loss in dB means the distance is too small for the model: 0 dB when `allowed`, an error otherwise."""
    if np.ndim(PL) == 0:
        if PL < 0:
            if not allowed:
                raise RuntimeError("The distance is too small to calculate a valid path loss.")
            return 0.0
        return PL
    if np.any(PL < 0):
        if not allowed:
            raise RuntimeError("The distance is too small to calculate a valid path loss.")
        PL[PL < 0] = 0.0
    return PL


def _log10(d):
    """log10 of a scalar or an array; d = 0 gives -inf (the clamp then makes it 0 dB) instead of math.log10's error."""
    if isinstance(d, (list, tuple, np.ndarray)):
        with np.errstate(divide="ignore"):
            return np.log10(np.asarray(d, dtype=float))
    return -math.inf if d == 0 else math.log10(d)


class PathLossGeneral:
    """PL [dB] = 10 n log10(d) + C, d in km.  A negative loss (a distance too small for the model) is an error unless
    handle_small_distances_bool is set, in which case it is taken as 0 dB (d = 0 included).  No shadowing."""

    def __init__(self, n, C):
        self.n = float(n)
        self.C = float(C)
        self.handle_small_distances_bool = False

    def calc_path_loss_dB(self, d):
        """Loss in dB (positive) at distance d (km; scalar or array)."""
        return _clamp_small_distances(10 * self.n * _log10(d) + self.C, self.handle_small_distances_bool)

    def calc_path_loss(self, d):
        """Loss in linear scale (a power gain below one) at distance d (km)."""
        return 10.0 ** (-self.calc_path_loss_dB(d) / 10.0)

    def which_distance_dB(self, PL):
        """Distance (km) at which the loss is PL dB."""
        if isinstance(PL, (list, tuple, np.ndarray)):
            PL = np.asarray(PL, dtype=float)
        return 10.0 ** ((PL - self.C) / (10.0 * self.n))

    def which_distance(self, pl):
        """Distance (km) at which the linear loss is pl."""
        return self.which_distance_dB(-10.0 * np.log10(pl))


class PathLoss3GPP1(PathLossGeneral):
    """3GPP scenario 1 (LTE assumptions at 2 GHz): PL = 128.1 + 37.6 log10(d), d in km."""

    def __init__(self):
        super().__init__(n=3.76, C=128.1)


class PathLossFreeSpace(PathLossGeneral):
    """Free space: 10 n log10(d) + C with C = 10 n (log10(fc 1e6) - 4.377911390697565), d in km, fc in MHz (n = 2: the Friis
    loss 20 log10(d) + 20 log10(fc) + 32.45).  Setting n or fc recomputes C."""

    def __init__(self, n=2.0, fc=900.0):
        self._n, self._fc = float(n), float(fc)
        self.handle_small_distances_bool = False

    n = property(lambda self: self._n)
    fc = property(lambda self: self._fc)

    @n.setter
    def n(self, value):
        self._n = float(value)

    @fc.setter
    def fc(self, value):
        self._fc = float(value)

    @property
    def C(self):
        return 10.0 * self._n * (math.log10(self._fc * 1e6) - 4.377911390697565)


class PathLossMetisPS7:
    """METIS propagation scenario 7 (indoor office, one floor), d in METRES, fc in MHz:
        line of sight (num_walls == 0):  18.7 log10 d + 46.8 + 20 log10(fc_GHz / 5)
        otherwise:                       36.8 log10 d + 43.8 + 20 log10(fc_GHz / 5) + 5 (num_walls - 1)
    num_walls is a scalar or broadcasts against d; a negative value is a ValueError.  The small-distance rule is that of
    PathLossGeneral.  The wall loss itself (num_walls x a loss per wall) is the scenario's, not the model's: metis.py."""

    LOS, NLOS = (18.7, 46.8), (36.8, 43.8)

    def __init__(self, fc=900.0):
        self.fc = float(fc)
        self.handle_small_distances_bool = False

    def calc_path_loss_dB(self, d, num_walls=0):
        walls = np.asarray(num_walls)
        if np.any(walls < 0):
            raise ValueError("num_walls cannot be negative")
        if walls.ndim == 0 and not isinstance(d, (list, tuple, np.ndarray)):
            # a scalar goes through the math module, an array through NumPy, as in the reference: the two log10 can
            # differ in the last place
            A, B = self.NLOS if walls > 0 else self.LOS
            PL = A * _log10(d) + B + 20 * math.log10(self.fc / 1e3 / 5.0) + (5 * (int(walls) - 1) if walls > 0 else 0)
            return _clamp_small_distances(PL, self.handle_small_distances_bool)
        d_arr, walls = np.broadcast_arrays(np.asarray(d, dtype=float), walls)
        with np.errstate(divide="ignore"):
            logd = np.log10(d_arr)
        freq = 20 * np.log10(self.fc / 1e3 / 5.0)
        los = self.LOS[0] * logd + self.LOS[1] + freq
        nlos = self.NLOS[0] * logd + self.NLOS[1] + freq + 5 * (walls - 1)
        return _clamp_small_distances(np.where(walls == 0, los, nlos), self.handle_small_distances_bool)

    def calc_path_loss(self, d, num_walls=0):
        """Loss in linear scale (a power gain below one) at distance d (metres)."""
        return 10.0 ** (-self.calc_path_loss_dB(d, num_walls) / 10.0)


def calc_transmit_power(SNR_dB, N0_dBm, cell_radius, path_loss_obj):
    """simulate_comp.py:629-659 _calc_transmit_power: the power (linear, W) that gives a mean SNR of SNR_dB at the cell border."""
    return transmit_power_for_border_loss(SNR_dB, N0_dBm, path_loss_obj.calc_path_loss(cell_radius))


def transmit_power_for_border_loss(SNR_dB, N0_dBm, path_loss_border):
    snr = 10.0 ** (float(SNR_dB) / 10.0)
    return snr * (10.0 ** (float(N0_dBm) / 10.0) / 1000.0) / path_loss_border
