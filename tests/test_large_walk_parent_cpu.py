"""No GPU: tests/golden/large_walk_parent.npz (the parent commit's results that tests/test_gpu_large_walk_parent.py holds the
kernels to bit for bit) is a recording of the RIGHT thing: its complex128 counts are the NumPy references' exactly, every case
that is not skipped makes symbol errors, the two blocks of every pilot case differ, the rank-deficient case is skipped throughout,
and the two halves of the split calls concatenate to the whole."""
import re

import numpy as np
import pytest

import large_pilot_cases as lp
import mimo_large_cases as ml
import pilot_link_oracle as po
from conftest import load_golden
from large_walk_cases import COUNT, COUNTER_KEYS, DTYPES, EDGE_COLUMNS, SKIP, SMALL, large_calls, pilot_calls

IDX = {k: i for i, k in enumerate(COUNTER_KEYS)}


@pytest.fixture(scope="module")
def z():
    return load_golden("large_walk_parent")


def test_it_holds_every_case_and_names_its_commit(z):
    assert re.fullmatch(r"[0-9a-f]{40}", str(z["parent_commit"])) and tuple(z["counter_keys"]) == COUNTER_KEYS
    want = {"%s/%s/%s" % (k, dt, f) for k in large_calls() for dt in DTYPES for f in ("cnt", "se", "be")}
    want |= {"%s/%s/%s" % (k, dt, f) for k in pilot_calls() for dt in DTYPES for f in ("cnt0", "cnt1", "se", "be", "err", "pow")}
    assert set(z.files) == want | {"parent_commit", "counter_keys"}
    assert len(large_calls()) == 2 * len(ml.CASES) + len(EDGE_COLUMNS) + 2 and len(pilot_calls()) == len(lp.CASES) + 2 * len(SMALL) + 4
    for k in want:
        field = k.rsplit("/", 1)[1]
        assert z[k].dtype == (np.int64 if field.startswith("cnt") else np.uint32 if field in ("se", "be") else np.float64), k


def test_complex128_counts_are_the_references(z):
    for key, (nt, nr, mmse, snr, ns, mname, first, count) in large_calls().items():
        if key.startswith("split/"):
            continue
        ref = ml.reference(nt, nr, mmse, snr, ns)
        assert np.array_equal(z[key + "/f64/se"], ref["se"]) and np.array_equal(z[key + "/f64/be"], ref["be"]), key
    for name in lp.NAMES:
        ref = lp.reference(name)
        assert np.array_equal(z["lpilot/%s/f64/se" % name], ref["se"]) and np.array_equal(z["lpilot/%s/f64/be" % name], ref["be"]), name
    for name in SMALL:
        ref = po.run(po.ALL_CASES[name], lp.FIRST, COUNT)
        for entry in ("lpilot", "pilot"):
            pre = "%s/%s/f64/" % (entry, name)
            assert np.array_equal(z[pre + "se"], ref["se"]) and np.array_equal(z[pre + "be"], ref["be"]), pre


def test_counter_blocks_are_the_sums_of_the_arrays(z):
    for key in list(large_calls()) + list(pilot_calls()):
        for dt in DTYPES:
            pre = "%s/%s/" % (key, dt)
            se, be = z[pre + "se"].astype(np.int64), z[pre + "be"].astype(np.int64)
            blocks = [(z[pre + "cnt"], se, be)] if pre + "cnt" in z.files else [(z[pre + "cnt%d" % b], se[b], be[b]) for b in (0, 1)]
            for cnt, s, b in blocks:
                if key.startswith("rank/"):
                    assert np.all(s == SKIP) and np.all(b == SKIP) and s.shape == (9,)
                    assert cnt[IDX["n_realizations"]] == 0 and cnt[IDX["n_skipped"]] == 9
                    assert cnt[IDX["sym_errors"]] == 0 and cnt[IDX["bit_errors"]] == 0
                    continue
                assert cnt[IDX["n_realizations"]] == len(s) and cnt[IDX["n_skipped"]] == 0 and not np.any(s == SKIP), pre
                assert cnt[IDX["sym_errors"]] == s.sum() > 0 and cnt[IDX["bit_errors"]] == b.sum() > 0, pre
                assert cnt[IDX["sym_errors_sq"]] == (s ** 2).sum() and cnt[IDX["bit_errors_sq"]] == (b ** 2).sum(), pre


def test_the_two_blocks_of_a_pilot_case_differ(z):
    for key in pilot_calls():
        if key.startswith("rank/"):
            continue
        for dt in DTYPES:
            pre = "%s/%s/" % (key, dt)
            assert z[pre + "cnt0"][IDX["sym_errors"]] != z[pre + "cnt1"][IDX["sym_errors"]], pre
            assert not np.array_equal(z[pre + "se"][0], z[pre + "se"][1]), pre
            assert np.all(z[pre + "err"] > 0) and np.all(z[pre + "pow"] > 0), pre


def test_the_halves_of_a_split_call_are_the_whole(z):
    for dt in DTYPES:
        a, b, whole = "split/large/a/%s/" % dt, "split/large/b/%s/" % dt, "large/7x9-zf-18dB-34/mindist/%s/" % dt
        for f in ("se", "be"):
            assert np.array_equal(np.concatenate([z[a + f], z[b + f]]), z[whole + f]), (dt, f)
        a, b, whole = "split/lpilot/a/%s/" % dt, "split/lpilot/b/%s/" % dt, "lpilot/7x9-p12/%s/" % dt
        for f in ("se", "be"):
            assert np.array_equal(np.concatenate([z[a + f], z[b + f]], axis=1), z[whole + f]), (dt, f)
        for f in ("err", "pow"):
            assert np.array_equal(np.concatenate([z[a + f], z[b + f]]), z[whole + f]), (dt, f)
        assert z[a + "se"].shape == (2, 37) and z[b + "se"].shape == (2, 33)
