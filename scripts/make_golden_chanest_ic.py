#!/usr/bin/env python3
"""Writes tests/golden/g2_chanest_ic.npz: what the reference's own interference-cancellation rules return on seeded random
inputs, for tests/test_chanest_ic_cpu.py and tests/test_gpu_chanest_ic.py.

The rules are the two functions estimate_channels_remove_only_direct and estimate_channels_remove_direct_and_perform_SIC of
the reference's apps/simple_precoded_srs.py (darcamo/pyphysim v0.7.2).  That app cannot be imported where its plotting
library is absent, and the functions need NumPy only: this script reads the app's source at run time, takes the two function
definitions out of it with `ast` and runs them.  It holds none of the app's text, and only arrays are written.

Inputs, all from one seeded RandomState: Nsc = 48 subcarriers (a comb of Ne = 24), two antennas, three receivers; three
unit-modulus sequences of random phases (the rules do not need them to be CAZAC, and 24 elements is a size of the standard's
tabulated sequences, which this package does not carry); received combs in which receiver i hears user i strongest.  The app
keeps 11 delay taps (num_taps_to_keep = 10).  Arrays are stored antenna-major, as this package lays them out:
    ref [3, 24], rx [3 receivers, 2, 24], direct / sic [3 receivers, 3 users, 2, 48].

usage: PYPHYSIM_REFERENCE=/path/to/pyphysim python scripts/make_golden_chanest_ic.py
"""
import ast
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("PYPHYSIM_REFERENCE", "")
OUT = os.path.join(REPO, "tests", "golden", "g2_chanest_ic.npz")
APP = os.path.join("apps", "simple_precoded_srs.py")
RULES = ("estimate_channels_remove_only_direct", "estimate_channels_remove_direct_and_perform_SIC")
NSC, N_ANT, TAPS_KEPT = 48, 2, 10
GAINS = np.array([[1.0, 0.2, 0.03], [0.05, 1.0, 0.3], [0.3, 0.3, 1.0]])      # [receiver, user]: amplitude of the user's part


def reference_rules():
    tree = ast.parse(open(os.path.join(REF, APP)).read())
    keep = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in RULES]
    assert sorted(node.name for node in keep) == sorted(RULES)
    scope = {"np": np}
    exec(compile(ast.Module(body=keep, type_ignores=[]), APP, "exec"), scope)
    return [scope[name] for name in RULES]


def build_fixture():
    ne = NSC // 2
    rng = np.random.RandomState(20261018)
    ref = np.exp(2j * np.pi * rng.rand(3, ne))
    # receiver i: sum_u g[i, u] * (a short random channel of user u) * r_u + noise, [Ne, antennas] as the app lays it out
    rx = []
    for i in range(3):
        y = 0.05 * (rng.randn(ne, N_ANT) + 1j * rng.randn(ne, N_ANT))
        for u in range(3):
            h = np.zeros((NSC, N_ANT), dtype=complex)
            h[:4] = (rng.randn(4, N_ANT) + 1j * rng.randn(4, N_ANT)) * GAINS[i, u]
            y = y + np.fft.fft(h, axis=0)[::2] * ref[u][:, None]
        rx.append(y)
    out = {"ref": ref, "rx": np.stack([y.T for y in rx])}
    comb = np.arange(0, NSC, 2)
    for name, rule in zip(("direct", "sic"), reference_rules()):
        got = rule(rx[0].copy(), rx[1].copy(), rx[2].copy(), ref[0], ref[1], ref[2], NSC, comb)
        # the rules return uH11, uH12, uH13, uH21, ...: receiver-major, each [Nsc, antennas]
        out[name] = np.stack([np.stack([got[3 * i + u].T for u in range(3)]) for i in range(3)])
    return out


if __name__ == "__main__":
    if not os.path.isfile(os.path.join(REF, APP)):
        raise SystemExit("PYPHYSIM_REFERENCE must name a checkout of the reference (no %s under '%s')" % (APP, REF))
    fixture = build_fixture()
    np.savez(OUT, **fixture)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(fixture), os.path.getsize(OUT)))
