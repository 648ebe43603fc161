"""CPU: the conditions under which tests/test_gpu_decide_forms.py means something, asserted with the reference and the host grid
builder alone (tests/decide_points.py says how the tables, points, orders, reference and rounding bounds are made):
  * every table's candidate grid is well formed (mcle_build_demod_grid, the shipped host code): 8 / 16 / 32 cells per axis, lists of
    1 ... 7 ascending indices below M or the BARE 0xFF marker (demod_grid4_multi_search reads candidate bytes of a marker word
    before it looks at the count and relies on their being zero), and marker32 does carry the marker;
  * per (table, metric) at most 25 % of the complex64 points are unclear, and no complex128 point is unclear outside exact ties -- a
    looser bound cannot quietly empty the comparison on the device;
  * the point set reaches every list-length class the grid has (1, 2-4, 5-7, 0xFF);
  * for every group size the interleaved order has a group that mixes a certified with an uncertified point (tables with a
    certificate) and one that mixes a short with a long list (tables whose grid has long lists), and the natural order has a wholly
    certified group (the early return of demod_multi_cert).  BPSK, the irregular tables and marker32 have no certificate, and BPSK
    no list longer than 2: there is nothing to mix there."""
import numpy as np
import pytest

import decide_points as dp
import test_demod_grid as tdg


@pytest.mark.parametrize("name", dp.NAMES)
def test_every_table_has_a_well_formed_grid(name):
    table = dp.TABLES[name][0]
    G, x0, y0, inv_h, cells = tdg.build(table)
    assert G in (8, 16, 32) and cells.size == G * G
    n = (cells & np.uint64(0xFF)).astype(np.int64)
    marker = n == 0xFF
    assert np.all(cells[marker] == np.uint64(0xFF))                         # bare: every candidate byte of a marker word is 0
    assert np.all((n[~marker] >= 1) & (n[~marker] <= 7))
    cand = np.stack([((cells >> np.uint64(8 * (j + 1))) & np.uint64(0xFF)).astype(np.int64) for j in range(7)], axis=1)
    live = (np.arange(7)[None, :] < n[:, None]) & ~marker[:, None]
    assert np.all(cand[live] < table.size) and np.all(cand[~live] == 0)
    both = live[:, 1:] & live[:, :-1]
    assert np.all((cand[:, 1:] > cand[:, :-1])[both])                        # ascending: list order is index order (first minimum)
    if name == "marker32":
        assert marker.any()
    if name == "duplicates8":                                                # a duplicate pair is listed together, lower index first
        assert np.all([(1 not in c[:k]) or (0 in c[:k]) for c, k in zip(cand[~marker], n[~marker])])


@pytest.mark.parametrize("dtype", dp.DTYPES)
@pytest.mark.parametrize("name", dp.NAMES)
def test_the_point_set_can_hold_the_device_to_something(name, dtype):
    c = dp.case(name, dtype)
    n = c.pts.size
    assert 6000 <= n <= 80000 and n % 12 == 0
    # (b) the unclear share, by the reference alone
    for metric, decided in c.ref.decided.items():
        unclear = ~decided & ~c.ref.exact_tie
        print("%s %s %s: %d points, %.2f %% not decided by the reference, %d exact ties" % (name, dtype, metric, n, 100.0 * (~decided).mean(), c.ref.exact_tie.sum()))
        if dtype == "f64":
            assert not unclear.any(), c.pts[unclear][:5]
        assert (~decided).mean() <= dp.UNCLEAR_CAP
    if c.kind == dp._lib.CONST_QAM:
        assert c.ref.slicer_clear().mean() >= 1.0 - dp.UNCLEAR_CAP                # (the tie lines ARE slicer boundaries)
    # every list-length class of the grid is reached
    cells = c.grid[4]
    have = set(dp.length_class((cells & np.uint64(0xFF)).astype(np.int64)).tolist())
    reached = set(c.lclass.tolist())
    print("%s %s: list-length classes %s" % (name, dtype, sorted(reached)))
    assert reached == have
    long_list = c.lclass >= 2
    for size in (2, 3, 4, 6):
        if c.cert is not None:
            assert c.sure.any() and not c.sure.all()
            t, f = dp.group_mix(c.sure, c.orders["interleaved"], size)
            assert (t & f).any()
            t, f = dp.group_mix(c.sure, c.orders["natural"], size)
            assert (~f).any()                                                # wholly certified: the early return
        if long_list.any():
            t, f = dp.group_mix(long_list, c.orders["interleaved"], size)
            assert (t & f).any()
            # ... and with an uncertified point in it, so that the group is searched at all
            if c.cert is not None:
                t2, f2 = dp.group_mix(c.sure, c.orders["interleaved"], size)
                assert (t & f & f2).any()
    if name != "bpsk":
        assert len(have) >= 2
    for order in c.orders.values():
        assert np.array_equal(np.sort(order), np.arange(n))


def test_marker_grid_decides_like_the_sweep():
    """the NumPy statement of the device lookup (tests/test_demod_grid.py) on marker32, built to carry 0xFF cells (the PSK tables have them at the origin too)"""
    c = dp.case("marker32", "f32")
    G, x0, y0, inv_h, cells = c.grid
    r = c.pts.astype(np.complex64)
    tab = c.table.astype(np.complex64)
    for metric_fn in (tdg.metric_literal, tdg.metric_two_fma):
        metric = metric_fn(tab, r)
        got, n = tdg.grid_decide(cells, G, x0, y0, inv_h, metric)(r)
        assert np.array_equal(got, np.argmin(metric, axis=1))
        assert (n == 0xFF).any() and (n <= 4).any()


@pytest.mark.parametrize("name", ["qam256", "psk16", "irregular64", "duplicates8", "marker32"])
def test_the_rules_accept_a_correct_search_and_refuse_a_wrong_one(name):
    """rule (a) is neither unsatisfiable nor empty: the float32 NumPy statements of the two metrics (tests/test_demod_grid.py) pass it
    on every point; the same labels with the LAST index on exact ties, or with the runner-up on a handful of clear points, do not"""
    c = dp.case(name, "f32")
    r, tab = c.pts.astype(np.complex64), c.table.astype(np.complex64)
    for metric, fn in (("literal", tdg.metric_literal), ("two_fma", tdg.metric_two_fma)):
        m = fn(tab, r)
        lab = np.argmin(m, axis=1)
        assert c.ref.wrong(lab, metric).size == 0
        clear = np.flatnonzero(c.ref.clear[metric])[::97]
        off = lab.copy()
        off[clear] = np.argsort(m[clear], axis=1)[:, 1]
        assert np.array_equal(c.ref.wrong(off, metric), clear)
        if c.ref.tied.sum() > 100:                                           # mirror images / duplicates
            last = m.shape[1] - 1 - np.argmin(m[:, ::-1], axis=1)
            assert c.ref.wrong(last, metric).size > 0
