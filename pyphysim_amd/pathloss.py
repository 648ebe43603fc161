"""Host-only path loss models (reference channels/pathloss.py:669-816 PathLossGeneral, :977-1020 PathLoss3GPP1): what
the CoMP application's power rule needs (apps/comp_BD/simulate_comp.py:629-659) -- the loss at the cell border fixes the
transmit power for a wanted SNR there.  Cell geometry is out of scope: the distances come from the user.

    >>> pl = PathLoss3GPP1()
    >>> pl.calc_path_loss(1)
    1.5488166189124858e-13
    >>> pl.calc_path_loss_dB(1)
    128.1
    >>> pl.which_distance_dB(130)
    1.1233935211892188
"""
import math

import numpy as np


class PathLossGeneral:
    """PL [dB] = 10 n log10(d) + C, d in km.  A negative loss (a distance too small for the model) is an error unless
    handle_small_distances_bool is set, in which case it is taken as 0 dB.  No shadowing."""

    def __init__(self, n, C):
        self.n = float(n)
        self.C = float(C)
        self.handle_small_distances_bool = False

    def calc_path_loss_dB(self, d):
        """Loss in dB (positive) at distance d (km; scalar or array)."""
        if isinstance(d, (list, tuple, np.ndarray)):
            PL = 10 * self.n * np.log10(np.asarray(d, dtype=float)) + self.C
            if np.any(PL < 0):
                if not self.handle_small_distances_bool:
                    raise RuntimeError("The distance is too small to calculate a valid path loss.")
                PL[PL < 0] = 0.0
            return PL
        PL = 10 * self.n * math.log10(d) + self.C
        if PL < 0:
            if not self.handle_small_distances_bool:
                raise RuntimeError("The distance is too small to calculate a valid path loss.")
            PL = 0.0
        return PL

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


def calc_transmit_power(SNR_dB, N0_dBm, cell_radius, path_loss_obj):
    """simulate_comp.py:629-659 _calc_transmit_power: the power (linear, W) that gives a mean SNR of SNR_dB at the cell border."""
    return transmit_power_for_border_loss(SNR_dB, N0_dBm, path_loss_obj.calc_path_loss(cell_radius))


def transmit_power_for_border_loss(SNR_dB, N0_dBm, path_loss_border):
    snr = 10.0 ** (float(SNR_dB) / 10.0)
    return snr * (10.0 ** (float(N0_dBm) / 10.0) / 1000.0) / path_loss_border
