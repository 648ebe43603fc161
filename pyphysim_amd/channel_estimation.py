"""Pilot-based channel estimation from CAZAC reference signals on the GPU.

Class names, constructor and method signatures and array shapes are those of the reference's
``reference_signals.channel_estimation`` module, so its users' code runs unchanged; what is new is a
leading batch axis of realizations.  Everything goes through ONE kernel launch per call
(``mcle_cazac_estimate``: a wavefront per (realization, receive antenna) row, csrc/kernels_chanest.hip):

    H^ = FFT_{m Ne}( IFFT_{Ne}(conj(r) * y)[0 .. K] )          K = num_taps_to_keep, m = size_multiplier

times Ne when the sequence has unit norm.  NumPy in, NumPy out; a
:class:`pyphysim_amd.engine.DeviceArray` stays on the device.

:func:`estimate_with_interference_cancellation` is the staged form of the reference's apps/simple_precoded_srs.py rules
(direct-link removal, ordered successive cancellation) for a received signal the caller brings: ``mcle_cazac_estimate`` and
``mcle_cazac_cancel`` launches with the ordering done on the host.  The fused Monte Carlo is ``Engine.run_chanest_ic``.
"""
import numpy as np

from . import _lib
from .engine import DeviceArray, get_engine
from .reference_signals import UeSequence

__all__ = ["CazacBasedChannelEstimator", "CazacBasedWithOCCChannelEstimator", "estimate_with_interference_cancellation"]


def _as_array(x):
    return x if isinstance(x, DeviceArray) else np.asarray(x)


class CazacBasedChannelEstimator:
    """Least-squares estimate of an uplink channel from the CAZAC reference sequence (SRS or DMRS) of one user,
    truncated to the first delay taps and interpolated to `size_multiplier` times as many subcarriers
    (2: an SRS comb on every other subcarrier; 1: DMRS).

    ue_ref_seq: a :class:`~pyphysim_amd.reference_signals.UeSequence` (its `normalized` flag is honoured) or a
    plain array.  engine, dtype: where and in which arithmetic ('f64' / 'f32') to run; default: the
    process-wide engine and its default.
    """

    _INPUT_RANKS = (1, 2, 3)

    def __init__(self, ue_ref_seq, size_multiplier=2, engine=None, dtype=None):
        self._unit_norm = bool(ue_ref_seq.normalized) if isinstance(ue_ref_seq, UeSequence) else False
        self._seq = np.asarray(ue_ref_seq.seq_array() if isinstance(ue_ref_seq, UeSequence) else ue_ref_seq)
        self._m = int(size_multiplier)
        self._engine, self._dtype = engine, dtype

    @property
    def engine(self):
        if self._engine is None:
            self._engine = get_engine()
        return self._engine

    @property
    def ue_ref_seq(self):
        """The user's sequence, as an array."""
        return self._seq

    def _launch(self, rows, num_taps_to_keep, cover=None):
        return self.engine.cazac_estimate(self._seq, rows, num_taps_to_keep, size_multiplier=self._m,
                                          normalized=self._unit_norm, cover=cover, dtype=self._dtype)

    def estimate_channel_freq_domain(self, received_signal, num_taps_to_keep):
        """received_signal (frequency domain, the comb's positions): [Ne], [Nr, Ne] or [B, Nr, Ne] for B realizations
        of Nr receive antennas.  Delay taps 0 .. num_taps_to_keep are kept -- one more than the name suggests, as in
        the reference.  Returns [..., size_multiplier * Ne]."""
        rx = _as_array(received_signal)
        if len(rx.shape) not in self._INPUT_RANKS:
            raise ValueError("received_signal has %d axes; expected [Ne], [Nr, Ne] or [B, Nr, Ne]" % len(rx.shape))
        return self._launch(rx, num_taps_to_keep)


class CazacBasedWithOCCChannelEstimator(CazacBasedChannelEstimator):
    """The estimator for a DMRS sequence sent under an orthogonal cover code: Nc slots, slot c multiplied by
    cover_code[c].  The code is undone and the slots averaged (inside the kernel's staging) before the estimation;
    size_multiplier is 1."""

    def __init__(self, ue_ref_seq, engine=None, dtype=None):
        cover = ue_ref_seq.cover_code
        super().__init__(ue_ref_seq.seq_array()[0] * cover[0], size_multiplier=1, engine=engine, dtype=dtype)
        self._unit_norm = bool(ue_ref_seq.normalized)
        self._cover = cover

    @property
    def cover_code(self):
        """The user's cover code."""
        return self._cover

    def estimate_channel_freq_domain(self, received_signal, num_taps_to_keep, extra_dimension=True):
        """received_signal: with extra_dimension=True the cover-code axis comes before the element axis,
        [Nc, Ne], [Nr, Nc, Ne] or [B, Nr, Nc, Ne]; with extra_dimension=False the slots are laid end to end on the last
        axis, [Nc*Ne], [Nr, Nc*Ne] or [B, Nr, Nc*Ne].  RuntimeError for any other number of axes.  Returns [..., Ne]."""
        rx = _as_array(received_signal)
        nc, rank = int(self._cover.size), len(rx.shape)
        if rank not in ((2, 3, 4) if extra_dimension else (1, 2, 3)):
            raise RuntimeError("received_signal has %d axes, which extra_dimension=%s does not take" % (rank, extra_dimension))
        if not extra_dimension:
            rx = rx.reshape(tuple(rx.shape[:-1]) + (nc, rx.shape[-1] // nc))
        return self._launch(rx, num_taps_to_keep, cover=np.real(self._cover))


def estimate_with_interference_cancellation(ref_seqs, rx, num_taps_to_keep, size_multiplier, direct_user, mode, engine=None,
                                            dtype=None):
    """Estimates of every user on one comb at the receiver of `direct_user`, with interference cancellation.

    ref_seqs [n_users, Ne]; rx [..., Nr, Ne] (NumPy): the received comb of Nr antennas per realization.  mode 0 / 'none':
    every user from rx; 1 / 'direct': the direct user is estimated from rx and its contribution est[::m] * ref subtracted,
    the others are estimated from that residual; 2 / 'sic': then the others are ordered by the norm of their first estimates
    over the antennas and subcarriers, descending (a tie: the higher index first), and each one after the strongest is
    estimated again from the residual left by the final estimates of all stronger ones.  Returns [..., Nr, n_users, m Ne]:
    rx's leading axes, then the user, then the subcarrier.
    The order is decided per realization on the host; realizations that share an order share their launches."""
    mode = int(_lib.CHANEST_IC_MODES.get(mode, mode))
    seqs = np.atleast_2d(np.asarray(ref_seqs))
    n_users, ne = seqs.shape
    rx = np.asarray(rx)
    if mode not in (0, 1, 2) or not 0 <= int(direct_user) < n_users:
        raise ValueError("mode must be 0, 1 or 2 and direct_user one of the %d users" % n_users)
    if rx.ndim < 2 or rx.shape[-1] != ne:
        raise ValueError("rx must be [..., Nr, Ne = %d] (got %s)" % (ne, rx.shape))
    lead, nr, m, d = rx.shape[:-2], rx.shape[-2], int(size_multiplier), int(direct_user)
    eng = get_engine() if engine is None else engine
    y = rx.reshape((-1, nr, ne))

    def estimate(u, rows):
        return eng.cazac_estimate(seqs[u], rows, num_taps_to_keep, size_multiplier=m, dtype=dtype)

    first = d if mode else 0
    est = [None] * n_users
    est[first] = estimate(first, y)
    others = [u for u in range(n_users) if u != first]
    if mode:
        y = eng.cazac_cancel(seqs[d], y, est[d], size_multiplier=m, dtype=dtype)
    for u in others:
        est[u] = estimate(u, y)
    if mode == 2 and len(others) > 1:
        norms = np.stack([np.linalg.norm(est[u].reshape(len(y), -1).astype(np.complex128), axis=1) for u in others], axis=1)
        # descending; on a tie the higher index first: sort by (-norm, -index)
        idx = np.asarray(others)
        orders = np.stack([idx[np.lexsort((-idx, -row))] for row in norms]) if len(y) else np.zeros((0, len(others)), int)
        for order in {tuple(o) for o in orders.tolist()}:
            rows = np.flatnonzero((orders == np.asarray(order)).all(axis=1))
            res = y[rows]
            for s in range(1, len(order)):
                res = eng.cazac_cancel(seqs[order[s - 1]], res, est[order[s - 1]][rows], size_multiplier=m, dtype=dtype)
                est[order[s]][rows] = estimate(order[s], res)
    out = np.stack(est, axis=2)                                   # [B, Nr, n_users, m Ne]
    return out.reshape(tuple(lead) + out.shape[1:])
