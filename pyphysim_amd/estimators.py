"""LS and MMSE block-pilot channel estimators on the GPU.

Function names, signatures and array shapes are those of the reference's ``channel_estimation.estimators`` module
(Fodor et al. 2014, "Performance analysis of block and comb type channel estimation for massive MIMO systems"), so
its users' code runs unchanged.  The model is ``Y_p = h s + N`` with ``Y_p`` ``[Nr, num_pilots]``, ``s``
``[Nt, num_pilots]`` and ``h`` of covariance ``C`` across the receive antennas:

    LS:    h^ = Y_p s^H (s s^H)^-1
    MMSE:  h^ = (noise_power I + num_pilots C)^-1 C (Y_p s^H) num_pilots / |s|^2          (Nt = 1)

A 3-D ``Y_p`` ``[num_realizations, Nr, num_pilots]``, with a 2-D ``s`` shared by all realizations or a 3-D one, is ONE
kernel launch (``mcle_ls_estimate`` / ``mcle_mmse_estimate``, csrc/kernels_estimators.hip), not a loop.  NumPy in, NumPy
out; a :class:`pyphysim_amd.engine.DeviceArray` stays on the device.  The two ``compute_theoretical_*`` functions are
host scalars.  The fused Monte Carlo of both estimators is ``Engine.run_pilot_mse``
(:class:`pyphysim_amd.simulators.PilotEstimationSimulator`).
"""
import numpy as np

from .engine import DeviceArray, get_engine

__all__ = ["compute_ls_estimation", "compute_mmse_estimation", "compute_theoretical_ls_MSE",
           "compute_theoretical_mmse_MSE"]


def _as_array(x):
    return x if isinstance(x, DeviceArray) else np.asarray(x)


def _batched(Y_p, s):
    """-> (Y [batch, Nr, P], s, whether Y_p was 2-D)"""
    Y_p, s = _as_array(Y_p), _as_array(s)
    if len(Y_p.shape) == 2:
        if len(s.shape) != 2:
            raise ValueError("a 2-D Y_p takes a 2-D s (got %s)" % (tuple(s.shape),))
        return Y_p.reshape((1,) + tuple(Y_p.shape)), s, True
    if len(Y_p.shape) != 3 or len(s.shape) not in (2, 3):
        raise ValueError("Y_p must be [Nr, num_pilots] or [num_realizations, Nr, num_pilots] and s [Nt, num_pilots] or "
                         "[num_realizations, Nt, num_pilots] (got %s, %s)" % (tuple(Y_p.shape), tuple(s.shape)))
    return Y_p, s, False


def _first(out):
    return out.reshape(tuple(out.shape[1:])) if isinstance(out, DeviceArray) else out[0]


def compute_ls_estimation(Y_p, s, engine=None, dtype=None):
    """The LS estimate of the channel from the received pilots.

    Y_p: `Nr x num_pilots` or `num_realizations x Nr x num_pilots`; s: `Nt x num_pilots` (the same pilots in every
    realization) or `num_realizations x Nt x num_pilots`, Nt <= 8 and Nt <= num_pilots.  Returns `Nr x Nt` or
    `num_realizations x Nr x Nt`.  The reference raises on a singular s s^H; here the values are then unspecified.
    engine, dtype: where and in which arithmetic ('f64' / 'f32') to run; default: the process-wide engine and its default."""
    Y, s, single = _batched(Y_p, s)
    out = (get_engine() if engine is None else engine).ls_estimate(Y, s, dtype=dtype)
    return _first(out) if single else out


def compute_mmse_estimation(Y_p, s, noise_power, C, engine=None, dtype=None):
    """The MMSE estimate of a SIMO channel (Nt = 1) of covariance C (`Nr x Nr`; a path loss belongs in it) from the
    received pilots.  Shapes as compute_ls_estimation; returns `Nr x 1` or `num_realizations x Nr x 1`."""
    Y, s, single = _batched(Y_p, s)
    out = (get_engine() if engine is None else engine).mmse_estimate(Y, s, noise_power, C, dtype=dtype)
    return _first(out) if single else out


def compute_theoretical_ls_MSE(Nr, noise_power, alpha, pilot_power, num_pilots):
    """The MSE of the LS estimator, normalised by the path loss alpha^2: Nr noise_power / (alpha^2 pilot_power num_pilots)."""
    return Nr * noise_power / ((alpha ** 2) * pilot_power * num_pilots)


def compute_theoretical_mmse_MSE(Nr, noise_power, alpha, pilot_power, num_pilots, C):
    """The MSE of the MMSE estimator: tr( C (I + alpha^2 pilot_power num_pilots / noise_power C)^-1 )."""
    C = np.asarray(C)
    return np.trace(C @ np.linalg.inv(np.eye(Nr) + alpha ** 2 * pilot_power * num_pilots / noise_power * C))
