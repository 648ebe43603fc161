"""CPU: the case table of the estimators' shape envelope (tests/estimators_oracle.py ENVELOPE_CASES, run on the GPU by
tests/test_gpu_estimators_envelope.py), on the NumPy restatement alone and for both index ranges (realizations 0 .. 36 and
2^32 - 5 .. 2^32 + 31 of the envelope seed): every compared error is large enough for a relative comparison to mean
something, no Gram matrix is worse conditioned than in a case the suite already holds to the operator tolerance, the LDS
sizes are those the table was chosen for, and no shape inside the argument rules exceeds the LDS budget."""
import itertools

import numpy as np
import pytest

import estimators_oracle as eo

CASES = sorted(eo.ENVELOPE_CASES)
# complex128 / complex64 bytes of LDS per wavefront where a case was chosen for them
TABLE_LDS = {"d": (81920, None), "e": (69888, None), "f": (131328, 65792), "g": (133120, None)}

_WANT = {}


def envelope_want(case, first):
    """The restatement of the 37 realizations from `first` of a case, computed once and left unchanged."""
    if (case, first) not in _WANT:
        out = eo.pilot_mse(eo.ENVELOPE_SEED, eo.envelope_reals(first), eo.ENVELOPE_CASES[case])
        for v in out.values():
            if v is not None:
                v.setflags(write=False)
        _WANT[case, first] = out
    return _WANT[case, first]


def gram_cond(s):
    return float(np.max(np.linalg.cond(s @ np.conj(np.swapaxes(s, -1, -2)))))


def held_cond():
    """The worst cond(s s^H) of test_parity_of_the_ls_estimator_with_several_transmit_antennas at nt = 8 (P = 11,
    realizations 0 .. 12), which the GPU suite holds to the operator tolerance."""
    if "held" not in _WANT:
        cfg = eo.default_cfg(nr=5, nt=8, n_pilots=11, noise_power=0.5, pilot_power=1.5, alpha=0.7)
        _WANT["held"] = gram_cond(eo.pilot_mse(eo.ENVELOPE_SEED, np.arange(13), cfg)["s"])
    return _WANT["held"]


def test_table_is_the_one_the_issue_states():
    assert CASES == list("abcdefghijkl") and eo.ENVELOPE_COUNT == 37 and eo.ENVELOPE_FIRSTS == (0, 2 ** 32 - 5)
    shapes = {k: (c["nr"], c["nt"], c["n_pilots"], c["noise_power"]) for k, c in eo.ENVELOPE_CASES.items()}
    assert shapes == {"a": (1, 1, 1, 2.0), "b": (15, 1, 2, 0.5), "c": (17, 1, 9, 0.5), "d": (32, 1, 255, 16.0),
                      "e": (113, 1, 16, 1.0), "f": (128, 1, 256, 16.0), "g": (128, 8, 256, 16.0), "h": (5, 4, 4, 0.5),
                      "i": (33, 5, 12, 0.5), "j": (16, 6, 7, 0.5), "k": (64, 7, 64, 4.0), "l": (3, 2, 3, 0.5)}
    for k, cfg in eo.ENVELOPE_CASES.items():
        assert cfg["pilot_power"] == 1.5 and cfg["alpha"] == 0.7
        assert (cfg["pilots"] is not None) == (k in "chjl") and (cfg["L"] is not None) == (k in "bcefghikl")
        assert (cfg["cov"] is not None) == (k in "abcdef") and (cfg["cov"] is None or cfg["nt"] == 1)
        if cfg["L"] is not None and cfg["cov"] is not None:                   # cov = alpha^2 L L^H
            assert np.allclose(0.49 * cfg["L"] @ cfg["L"].conj().T, cfg["cov"], rtol=0, atol=1e-13)
        if cfg["pilots"] is not None:
            assert np.allclose(np.abs(cfg["pilots"]) ** 2, 1.5, rtol=1e-14)
    h = eo.ENVELOPE_CASES["h"]["pilots"]
    assert np.allclose(h @ h.conj().T, 4 * 1.5 * np.eye(4), rtol=0, atol=1e-13)
    assert np.array_equal(eo.ENVELOPE_CASES["c"]["pilots"],
                          np.sqrt(1.5) * np.exp(2j * np.pi * np.random.RandomState(3).rand(1, 9)))


@pytest.mark.parametrize("first", eo.ENVELOPE_FIRSTS)
@pytest.mark.parametrize("case", CASES)
def test_errors_are_large_enough_for_a_relative_comparison(case, first):
    want = envelope_want(case, first)
    keys = ["err_ls"] + (["err_mmse"] if want["err_mmse"] is not None else [])
    ratios = {k: float(np.min(want[k] / want["pow"])) for k in keys}
    print(case, first, " ".join("%s/pow >= %.4g" % kv for kv in ratios.items()))
    assert want["pow"].shape == (37,) and np.all(want["pow"] > 0)
    assert min(ratios.values()) > 1e-2, ratios


@pytest.mark.parametrize("first", eo.ENVELOPE_FIRSTS)
@pytest.mark.parametrize("case", CASES)
def test_no_gram_matrix_is_worse_conditioned_than_one_already_held(case, first):
    cond = gram_cond(envelope_want(case, first)["s"])
    print(case, first, "cond(s s^H) %.4g against %.4g" % (cond, held_cond()))
    assert cond <= held_cond()


def test_the_two_ranges_are_different_realizations():
    """Realization 2^32 + r is not realization r: the high word of the index reaches the restatement's generator."""
    for case in ("b", "i", "l"):
        lo, hi = envelope_want(case, 0), envelope_want(case, eo.ENVELOPE_FIRSTS[1])
        assert not np.any(np.isin(hi["pow"], lo["pow"])), case
        again = eo.pilot_mse(eo.ENVELOPE_SEED, [2 ** 32 + 31], eo.ENVELOPE_CASES[case])
        assert again["pow"][0] == hi["pow"][36] and again["err_ls"][0] == hi["err_ls"][36]


def test_lds_sizes_are_those_the_table_was_chosen_for():
    for case, (f64, f32) in TABLE_LDS.items():
        cfg = eo.ENVELOPE_CASES[case]
        assert eo.envelope_lds(cfg, "f64") == f64, case
        assert f32 is None or eo.envelope_lds(cfg, "f32") == f32, case
    above = {c: tuple(eo.envelope_lds(eo.ENVELOPE_CASES[c], d) > eo.LDS_ATTRIBUTE_ABOVE for d in ("f64", "f32")) for c in CASES}
    assert {c for c in CASES if above[c][0]} == set("defg") and {c for c in CASES if above[c][1]} == set("fg")
    # e is the first nr that passes 63 KiB in complex128 at its P; complex64 stays below
    e = eo.ENVELOPE_CASES["e"]
    assert eo.pilot_mse_lds(112, 1, 16, True, 8) <= eo.LDS_ATTRIBUTE_ABOVE < eo.envelope_lds(e, "f64")
    # every complex128 shape with nr >= 113 is above it, whatever nt, P and the pilot mode
    assert eo.pilot_mse_lds(113, 1, 1, False, 8) > eo.LDS_ATTRIBUTE_ABOVE
    # workgroups per compute unit the launcher's grid assumes in complex128: two at d (exactly half the budget) and e, one
    # at f and g
    assert [eo.LDS_BUDGET // eo.envelope_lds(eo.ENVELOPE_CASES[c], "f64") for c in "defg"] == [2, 2, 1, 1]
    assert eo.LDS_BUDGET // eo.envelope_lds(eo.ENVELOPE_CASES["g"], "f32") == 2


def test_no_admissible_shape_exceeds_the_lds_budget():
    """The size grows with nr (in steps of 16) and with P, so the maximum is at nr = 128, P = 256; there every nt and both pilot
    modes and arithmetics are walked: 133 120 bytes at nt = 8, drawn pilots, complex128."""
    sizes = {(nt, rp, rb): eo.pilot_mse_lds(eo.MAX_NR, nt, eo.MAX_PIPELINE_PILOTS, rp, rb)
             for nt, rp, rb in itertools.product(range(1, eo.MAX_NT + 1), (False, True), (4, 8))}
    worst = max(sizes, key=sizes.get)
    assert worst == (8, True, 8) and sizes[worst] == 133120 <= eo.LDS_BUDGET
    for (nt, rp, rb), top in sizes.items():                     # monotone in nr and P: the corner is the maximum
        for nr, P in ((112, 256), (128, 255), (1, nt)):
            assert eo.pilot_mse_lds(nr, nt, P, rp, rb) <= top
