"""CPU: the 50-digit oracle of mcle_mu_link_stats (tests/mu_stats_oracle.py) held to oracle/multiuser.py on the reference's own
fixture (tests/golden/a14b_multiuser_stats.npz) and on the envelope shapes; its magnitudes dominate its values; NumPy in
complex128 meets the chain bound the GPU test uses."""
import numpy as np
import pytest

import mu_stats_oracle as mu
from helpers import GOLDEN, relerr
from oracle import multiuser as omu


def test_oracle_against_the_reference_fixture():
    z = np.load(GOLDEN + "/a14b_multiuser_stats.npz", allow_pickle=False)
    n = 0
    for ci in range(int(z["n_cases"])):
        pre = "case%d_" % ci
        Nr, Nt, ext = [int(v) for v in z[pre + "Nr"]], [int(v) for v in z[pre + "Nt"]], z[pre + "ext"]
        nv, pe = [float(v) for v in z[pre + "par"]]
        nv = None if nv < 0 else nv
        pl = z[pre + "pl"] if pre + "pl" in z.files else None
        pl_ext = z[pre + "pl_ext"] if pre + "pl_ext" in z.files else None
        full_Nt = np.hstack([Nt, ext]) if ext.size else Nt
        pl_big = None if pl is None else omu.pathloss_big(pl if pl_ext is None else np.hstack([pl, pl_ext]), Nr, full_Nt)
        n_ext = int(np.sum(ext)) if ext.size else 0
        for joint in (False, True):
            tag = pre + ("jp_" if joint else "")
            K = len(Nr)
            F = [z[tag + "F%d" % k] for k in range(K)]
            U = [z[tag + "U%d" % k] for k in range(K)]
            got = mu.exact(z[pre + "big_H"], Nr, Nt, F, U, nv or 0.0, pe if n_ext else 0.0, n_ext, joint, pl_big)
            for k in range(K):
                assert relerr(np.asarray(got[k]["sinr"], dtype=float), z[tag + "sinr%d" % k]) <= 1e-11
                assert relerr(np.asarray(got[k]["Q"], dtype=complex), z[tag + "Q%d" % k]) <= 1e-13
                n += 1
    assert n == 2 * (3 + 3 + 2 + 3 + 2 + 4)


@pytest.mark.parametrize("name", sorted(mu.SHAPES))
def test_numpy_meets_the_chain_bound_on_the_envelope_shapes(name):
    sh, inp = mu.SHAPES[name], mu.inputs(name)
    K = len(sh["Nr"])
    assert inp["H"].shape[0] == sh["batch"]
    for b in range(inp["unique"]):
        F, U = [f[b] for f in inp["F"]], [u[b] for u in inp["U"]]
        ex = mu.exact(inp["H"][b], sh["Nr"], sh["Nt"], F, U, sh["nv"], sh["pe"], sh["n_ext"], sh["joint"], inp["pl"])
        ref = mu.numpy_reference(inp["H"][b], sh, F, U, inp["pl"])
        for k in range(K):
            ch = mu.chain(sh["Nr"], sh["Nt"], sh["ns"], sh["n_ext"], sh["joint"], inp["pl"] is not None, k)
            e, (Q, Re, B, sinr) = ex[k], ref[k]
            assert np.all(np.abs(e["Q"]) <= e["Q_mag"] * (1 + 1e-15)) and np.all(np.abs(e["Re"]) <= e["Re_mag"] * (1 + 1e-15))
            assert np.all(np.abs(Q - e["Q"]) <= ch["Q"] * mu.EPS64 * e["Q_mag"])
            assert np.all(np.abs(Re - e["Re"]) <= ch["Re"] * mu.EPS64 * e["Re_mag"])
            assert len(B) == sh["ns"][k] == len(e["B"])
            for l in range(sh["ns"][k]):
                assert np.all(np.abs(B[l] - e["B"][l]) <= ch["B"] * mu.EPS64 * e["B_mag"][l])
                assert abs(sinr[l] - e["sinr"][l]) <= mu.EPS64 * e["sinr_err"][l]
    if name == "k2_dominant_stream":            # the cancellation is there: B_00 is eight digits below its magnitude
        assert float(np.max(np.abs(ex[0]["B"][0])) / np.max(ex[0]["B_mag"][0])) <= 1e-6


def test_item_counts_cover_the_workgroup_edges():
    items = {sh["batch"] * len(sh["Nr"]) for sh in mu.SHAPES.values()}
    assert {1, 64, 65, 210} <= items


def test_chain_lengths_are_counted_not_fitted():
    ch = mu.chain([4, 4, 4, 4], [4, 4, 4, 4], [4, 1, 2, 3], 8, True, True, 0)
    assert ch == dict(G=34, Re=22, Q=2 * 4 + 2 * 34 + 4 + 1, B=2 * 4 + 2 * 34 + 4 + 4, num=2 * (8 + 34) + 3, den=84 + 16 + 4)
    ch = mu.chain([1], [1], [1], 0, False, False, 0)
    assert ch == dict(G=2, Re=2, Q=8, B=11, num=11, den=19)
