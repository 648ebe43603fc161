"""CPU: the conditions that make the GPU comparisons of tests/test_gpu_pilot_link.py meaningful, on the NumPy restatement alone
(tests/pilot_link_oracle.py): its perfect-CSI half is the chain that is already pinned to the reference, no decision of either
half sits on a decision border, the estimate does not depend on how it is formed, and estimated and perfect CSI do give
different counts -- a kernel that used H twice would be noticed."""
import numpy as np
import pytest

from oracle import chains

import pilot_link_oracle as po

GAP_FLOOR = 1e-9           # every realization's smallest decision gap
ROUTE_SHARE = 1e-3         # the estimate by a second route moves no est by more than this share of the gap


@pytest.mark.parametrize("name", sorted(po.PARITY_CASES))
def test_perfect_csi_half_is_the_blast_chain(name):
    cfg, ref = po.PARITY_CASES[name], po.reference(name)
    assert cfg["L"] is None and cfg["alpha"] == 1.0
    for i, r in enumerate(range(po.FIRST, po.FIRST + po.COUNT)):
        out = chains.chain_mimo_scheme(chains.PhiloxRng(po.SEED, r), "blast", mod="qam", M=16, nt=cfg["nt"], nr=cfg["nr"],
                                       NSymbs=cfg["n_symbols"], snr_db=cfg["snr_db"], mmse=cfg["mmse"])
        assert out["noise_var"] == cfg["noise_var"]
        assert (out["symbol_errors"], out["bit_errors"]) == (ref["se"][1, i], ref["be"][1, i]), (name, r)
        assert (out["num_symbols"], out["num_bits"]) == (ref["n_symbols"], ref["n_bits"])


@pytest.mark.parametrize("name", sorted(po.ALL_CASES))
def test_no_realization_is_near_a_decision_border(name):
    """The cap on realizations left out of the exact comparison is zero: every one has to meet both conditions."""
    ref = po.reference(name)
    print(name, "smallest gap %.3g, largest route move %.3g, largest Gram condition %.3g"
          % (ref["gap"].min(), ref["route"].max(), ref["gram_cond"].max()))
    assert ref["gap"].shape == (po.COUNT,)
    assert np.all(ref["gap"] >= GAP_FLOOR), int(np.sum(ref["gap"] < GAP_FLOOR))
    assert np.all(ref["route"] <= ROUTE_SHARE * ref["gap"]), int(np.sum(ref["route"] > ROUTE_SHARE * ref["gap"]))


@pytest.mark.parametrize("name", sorted(po.ALL_CASES))
def test_estimated_and_perfect_csi_give_different_counts(name):
    cfg, ref = po.ALL_CASES[name], po.reference(name)
    assert cfg["noise_var"] > 0
    print(name, "symbol errors estimated %d perfect %d" % (ref["se"][0].sum(), ref["se"][1].sum()))
    assert ref["se"][0].sum() != ref["se"][1].sum() and ref["be"][0].sum() != ref["be"][1].sum()
    assert np.min(ref["err"] / ref["pow"]) > 0


@pytest.mark.parametrize("name", sorted(po.ALL_CASES))
def test_the_error_bar_is_above_the_rounding_of_the_subtraction(name):
    """|H^ - H|^2 is held at 1e-11 relative on the GPU.  tests/test_gpu_pilot_mse.py guards its bar by err / pow > 1e-2; at this
    link's SNRs no case meets that in every realization (the smallest ratios are 1.8e-5 .. 6.9e-3), so the guard here is the
    rounding model itself: what f64 can move err by stays below half the bar in every realization."""
    cfg, ref = po.ALL_CASES[name], po.reference(name)
    bound = po.err_rounding_bound(cfg, ref)
    print(name, "smallest err / pow %.3g, modelled rounding of err %.3g" % (np.min(ref["err"] / ref["pow"]), bound))
    assert bound <= 0.5e-11


def test_noise_free_estimate_is_the_channel():
    cfg = po.make_case(3, 4, 7, 6, 16.0, 1.5, noise_var=0.0)
    ref = po.run(cfg, 0, 8)
    assert np.all(ref["err"] / ref["pow"] <= 1e-24) and not ref["se"].any() and not ref["be"].any()


def test_stream_four_is_its_own_stream():
    """The pilot noise comes from stream 4: it is neither the data noise nor the channel's draw."""
    from oracle import philox
    z = [philox.cnormal(po.SEED, 3, 8, s) for s in (philox.STREAM_NOISE, philox.STREAM_CHAN, philox.STREAM_PHASE, po.STREAM_PILOT)]
    for i in range(4):
        for j in range(i):
            assert not np.any(z[i] == z[j])
