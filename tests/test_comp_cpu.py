"""CPU: the CoMP link oracle (tests/comp_oracle.py) against the reference's own realizations (tests/golden/g5_comp.npz,
minted by scripts/make_golden_comp.py), the host-only path loss models, the C ABI of mcle_run_comp, and the gap-rule
precondition of tests/test_gpu_comp.py shown with the oracle alone."""
import ctypes
import os
import re

import numpy as np
import pytest

import comp_oracle as co
from helpers import GOLDEN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(GOLDEN + "/g5_comp.npz", allow_pickle=False)
K, R, EXT, M, PACKET = [int(v) for v in Z["cfg"]]


@pytest.mark.parametrize("variant", co.VARIANTS)
@pytest.mark.parametrize("i", range(4))
def test_oracle_link_reproduces_the_reference(i, variant):
    """Fed the fixture's own MsPk, W and draws, the oracle's link gives the reference's decisions and per-stream counts
    exactly, per / spec_effic to 1e-12 and calc_JP_SINR (pe = 1) to 1e-10."""
    tag = "r%d_%s_" % (i, variant)
    Ns = [int(v) for v in Z[tag + "Ns"]]
    MsPk, W = [Z[tag + "MsPk%d" % k] for k in range(K)], [Z[tag + "W%d" % k] for k in range(K)]
    assert all(MsPk[k].shape == (K * R, Ns[k]) and W[k].shape == (Ns[k], R) for k in range(K))
    data = Z[tag + "input_data"]
    out = co.link(Z[tag + "big_H"], MsPk, W, data, Z[tag + "ext_data"], Z[tag + "noise"], co.table_for("psk", M))
    assert np.max(np.abs(out["received"] - Z[tag + "received"])) <= 1e-12 * np.max(np.abs(Z[tag + "received"]))
    assert np.array_equal(out["decisions"], Z[tag + "decoded"])
    assert np.array_equal(out["sym_err"], Z[tag + "sym_err"]) and np.array_equal(out["bit_err"], Z[tag + "bit_err"])
    res = co.stream_results(out["sym_err"], out["bit_err"], data.shape[1], co.omodem.level2bits(M), PACKET)
    ser, ber, per, se = Z[tag + "results"]
    assert res["ser"][0] / res["ser"][1] == ser and res["ber"][0] / res["ber"][1] == ber
    assert abs(res["per"][0] / res["per"][1] - per) <= 1e-12 and abs(res["spec_effic"][0] - se) <= 1e-12
    sinr = np.concatenate(co.jp_sinr(Z[tag + "big_H"], K, R, MsPk, W, float(Z["noise_var"]), pe=1.0))
    assert np.all(np.abs(sinr - Z[tag + "sinr"]) <= 1e-10 * np.abs(Z[tag + "sinr"]))
    # slots: 0 on an inactive stream
    slots = co.to_slots(out["sym_err"], Ns, R)
    assert slots.shape == (K * R,) and slots.sum() == out["sym_err"].sum()
    if variant in ("naive", "fixed"):
        assert Ns == [1] * K and np.all(slots[1::R] == 0)


def test_oracle_selection_follows_the_reference():
    """The oracle's stream counts are the reference's on the fixture's channels (LAPACK phases on both sides), and the stream
    counts really vary at this point."""
    snr, pe_dbm = Z["single_point"]
    iPu, pe, nv = float(Z["transmit_power"][0]), float(Z["single_pe"]), float(Z["noise_var"])
    for i in range(4):
        for variant in co.VARIANTS:
            tag = "r%d_%s_" % (i, variant)
            _, _, Ns = co.solve(Z[tag + "big_H"], K, R, iPu, nv, pe, variant, 1, "psk", M, PACKET)
            assert Ns == [int(v) for v in Z[tag + "Ns"]], tag
    hist = Z["ref_p0_ns_hist"]                      # [variant, stream count]
    eff = list(co.VARIANTS).index("effec_throughput")
    assert hist[eff, 1] > 0.1 * hist[eff].sum() and hist[eff, 2] > 0.1 * hist[eff].sum()


def test_pathloss_known_answers():
    from pyphysim_amd.pathloss import PathLoss3GPP1, PathLossGeneral, calc_transmit_power
    pl = PathLoss3GPP1()
    assert pl.calc_path_loss(1) == 1.5488166189124858e-13
    assert pl.calc_path_loss_dB(1) == 128.1
    assert pl.which_distance_dB(130) == 1.1233935211892188
    d = np.array([0.5, 1.0, 2.0])
    assert np.allclose(pl.which_distance_dB(pl.calc_path_loss_dB(d)), d, rtol=1e-14)
    assert np.allclose(pl.which_distance(pl.calc_path_loss(d)), d, rtol=1e-12)
    g = PathLossGeneral(2.0, 10.0)
    assert g.calc_path_loss_dB(10.0) == 30.0
    with pytest.raises(RuntimeError):
        g.calc_path_loss_dB(0.01)
    g.handle_small_distances_bool = True
    assert g.calc_path_loss_dB(0.01) == 0.0 and np.array_equal(g.calc_path_loss_dB(np.array([0.01, 10.0])), [0.0, 30.0])
    # the fixture's transmit power (the app's rule: the wanted SNR at the cell border, 1 km)
    assert abs(pl.calc_path_loss(1.0) - float(Z["path_loss_border"])) <= 1e-12 * float(Z["path_loss_border"])
    for (snr, _), want in zip(Z["ref_points"], Z["transmit_power"]):
        got = calc_transmit_power(float(snr), -116.4, 1.0, pl)
        assert abs(got - want) <= 1e-12 * want


def test_header_and_binding_declare_run_comp():
    from pyphysim_amd import _lib
    text = open(os.path.join(REPO, "include", "mcle.h")).read()
    assert re.search(r"\bint\s+mcle_run_comp\s*\(", text)
    body = re.search(r"typedef struct mcle_comp_cfg \{(.*?)\} mcle_comp_cfg;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[.*\]", "", n).strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == [n for n, _ in _lib.CompCfg._fields_]
    assert ctypes.sizeof(_lib.CompCfg) == 10 * 4 + 4 * 8 + 16 * 8 + 32 * 8
    assert _lib.CompCfg.iPu.offset == 40 and _lib.CompCfg.pathloss.offset == 72 and _lib.CompCfg.pathloss_ext.offset == 200
    assert "mcle_run_comp" in _lib.exported_symbols()
    assert _lib.COMP_VARIANTS["effec_throughput"] == (1, 4) and _lib.COMP_VARIANTS["Whitening"][0] == 0


GAP_SHAPES = [(3, 2, 1), (2, 2, 1), (2, 3, 2)]


@pytest.mark.parametrize("shape", GAP_SHAPES, ids=lambda s: "K%dr%de%d" % s)
def test_gap_rule_precondition(shape):
    """On the selection inputs of tests/test_gpu_comp.py the share of realizations the gap rule leaves out is within its cap of
    5 %: with 300 realizations at SNR 5 / 15 dB and Pe -10 / 10 dBm, none under 'capacity' and at most 7 of 300 (measured;
    the cap allows 15) under 'effective_throughput'.  At (5 dB, 10 dBm) about half the realizations reduce a stream."""
    Kk, r, E = shape
    PLB = 10 ** -12.81
    nv = 10.0 ** (-116.4 / 10.0) / 1000.0
    pl, ple = PLB * (2.0 * np.ones((Kk, Kk)) + 6.0 * np.eye(Kk)), 1.5 * PLB * np.ones((Kk, E))
    H = [co.draw_big_H(7, 37 + i, Kk, r, E, pl, ple) for i in range(300)]
    for snr in (5.0, 15.0):
        for pe_dbm in (-10.0, 10.0):
            iPu, pe = 10.0 ** (snr / 10.0) * nv / PLB, 10.0 ** (pe_dbm / 10.0) / 1000.0
            out_cap = out_eff = reduced = 0
            for Hi in H:
                cand = co.candidate_sinrs(Hi, Kk, r, iPu, nv, pe)
                v_eff = co.candidate_values(cand, "effec_throughput", "psk", 4, 60)
                out_cap += co.near_tie(co.candidate_values(cand, "capacity", None, None, None))
                out_eff += co.near_tie(v_eff)
                reduced += bool(np.any(np.argmax(v_eff, axis=1) + 1 < r))
            print(shape, snr, pe_dbm, "left out: capacity %d, effective_throughput %d; reduced %d" % (out_cap, out_eff, reduced))
            assert out_cap == 0 and out_eff <= 0.05 * 300
            if (snr, pe_dbm) == (5.0, 10.0):
                assert 0.3 * 300 <= reduced <= 0.7 * 300
