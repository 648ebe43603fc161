"""Thermal noise (reference channels/noise.py:11-33)."""
from .util import linear2dBm

BOLTZMANN = 1.380649e-23      # J / K (exact since the 2019 SI; scipy.constants.Boltzmann)


def calc_thermal_noise_power_dBm(T, delta_f):
    """Noise power in dBm of a bandwidth delta_f (Hz) at room temperature T (degrees Celsius): k (T + 273) delta_f.

        >>> calc_thermal_noise_power_dBm(25, 5e6)
        -106.86782148578291
    """
    return float(linear2dBm(BOLTZMANN * (T + 273.0) * delta_f))
