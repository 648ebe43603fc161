#!/usr/bin/env python3
"""Writes tests/golden/g1_chanest.npz: the reference's own reference-signal sequences and channel-estimator outputs
for the cases of tests/test_chanest_cpu.py and tests/test_gpu_chanest.py.

Drives the reference (darcamo/pyphysim v0.7.2, reference_signals/) the way oracle/make_golden.py does -- the stub modules
of oracle/ref_shim on sys.path, PYPHYSIM_REFERENCE naming its checkout, the numpy.int alias it still uses -- and holds
none of it.  Received arrays come from a seeded RandomState.  Arrays only.

usage: PYPHYSIM_REFERENCE=/path/to/pyphysim python scripts/make_golden_chanest.py
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("PYPHYSIM_REFERENCE", "/root/reference")
OUT = os.path.join(REPO, "tests", "golden", "g1_chanest.npz")

# estimator cases: name -> (Ne, root index, cyclic shift, K, m, rows, normalize); rows = 0: 1-D input
EST_CASES = {
    "ne36": (36, 5, 0, 3, 2, 0, False),            # smallest extended Zadoff-Chu size; a lane tail in both passes
    "ne37_all": (37, 36, 1, 36, 2, 2, False),      # prime size, every tap kept
    "ne64_m1": (64, 1, 2, 8, 1, 3, False),
    "ne150": (150, 25, 3, 15, 2, 4, False),
    "ne150_k70": (150, 25, 5, 70, 2, 2, False),    # K + 1 > 64
    "ne139_norm": (139, 17, 7, 40, 2, 2, True),
    "k0": (48, 7, 2, 0, 2, 2, False),
    "ne2048": (2048, 101, 4, 15, 2, 0, False),     # the table limit
    "rows67": (48, 7, 5, 5, 2, 67, False),
}
# The reference's list of primes ends at 1009, so beyond that it would not pick the largest prime <= size: named here
NZC = {"ne2048": 2039}
OCC_CASE = (48, 15, 4, 5, 3)                       # Ne, root index, cyclic shift, K, antennas; cover code [1, -1]


def build_fixture():
    sys.path.insert(0, os.path.join(REPO, "oracle", "ref_shim"))
    sys.path.insert(0, REF)
    np.int = int
    from pyphysim.reference_signals.channel_estimation import (CazacBasedChannelEstimator,
                                                               CazacBasedWithOCCChannelEstimator)
    from pyphysim.reference_signals.dmrs import DmrsUeSequence
    from pyphysim.reference_signals.root_sequence import RootSequence
    from pyphysim.reference_signals.srs import SrsUeSequence
    from pyphysim.reference_signals.zadoffchu import calcBaseZC

    out = {}
    # ---- sequences
    out["seq_zc139_u25"] = calcBaseZC(139, 25)
    root150 = RootSequence(root_index=25, size=150)
    out["seq_root150_u25"] = root150.seq_array()
    out["seq_root75_nzc31_u7"] = RootSequence(root_index=7, size=75, Nzc=31).seq_array()
    out["seq_srs150_cs0"] = SrsUeSequence(root150, 0).seq_array()
    out["seq_srs150_cs7"] = SrsUeSequence(root150, 7).seq_array()
    out["seq_dmrs150_cs11_occ"] = DmrsUeSequence(root150, 11, cover_code=np.array([1, -1])).seq_array()
    out["seq_srs139_cs3_norm"] = SrsUeSequence(RootSequence(root_index=25, Nzc=139), 3, normalize=True).seq_array()
    # ---- estimator
    rng = np.random.RandomState(20261018)
    for name, (ne, u, ncs, K, m, rows, norm) in EST_CASES.items():
        ue = SrsUeSequence(RootSequence(root_index=u, size=ne, Nzc=NZC.get(name)), ncs, normalize=norm)
        shape = (rows, ne) if rows else (ne,)
        rx = rng.randn(*shape) + 1j * rng.randn(*shape)
        if norm:
            rx = rx / np.sqrt(ne)
        out["est_%s_ref" % name] = ue.seq_array()
        out["est_%s_rx" % name] = rx
        out["est_%s_out" % name] = CazacBasedChannelEstimator(ue, size_multiplier=m).estimate_channel_freq_domain(rx, K)
    ne, u, ncs, K, nr = OCC_CASE
    ue = DmrsUeSequence(RootSequence(root_index=u, size=ne), ncs, cover_code=np.array([1, -1]))
    rx = rng.randn(nr, 2, ne) + 1j * rng.randn(nr, 2, ne)
    est = CazacBasedWithOCCChannelEstimator(ue)
    out["occ_ref"] = ue.seq_array()
    out["occ_rx"] = rx
    out["occ_out"] = est.estimate_channel_freq_domain(rx, K)
    out["occ_out_flat"] = est.estimate_channel_freq_domain(rx.reshape(nr, 2 * ne).copy(), K, extra_dimension=False)
    out["occ_out_1ant"] = est.estimate_channel_freq_domain(rx[0].copy(), K)
    return out


if __name__ == "__main__":
    fixture = build_fixture()
    np.savez(OUT, **fixture)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(fixture), os.path.getsize(OUT)))
