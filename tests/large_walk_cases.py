"""What tests/golden/large_walk_parent.npz records of the two large-array Blast links and the 4 x 4 pilot link
(csrc/pipeline_mimo_large.hip, pipeline_mimo_large_pilot.hip, pipeline_mimo_pilot.hip), shared by scripts/make_golden_large_walk.py
(records it from a build of the parent commit), tests/test_gpu_large_walk_parent.py (the kernels of this tree must reproduce it bit
for bit in BOTH arithmetics) and tests/test_large_walk_parent_cpu.py (keeps the fixture honest without a GPU).  TEST INFRASTRUCTURE.

The inputs are the existing ones and no larger: realizations 3 .. 72, 16-QAM.
    large/<case>/<method>       every case of mimo_large_cases.CASES, min-distance and slicer
    edge/<columns>              5 x 6 at 1, 31, 32 and 33 columns (mimo_large_cases.EDGE_COLUMNS)
    lpilot/<case>               every case of large_pilot_cases.CASES
    lpilot/<case>, pilot/<case> the three cases up to 4 x 4 through BOTH pilot entry points
    rank/lpilot, rank/pilot     two equal fixed pilot rows at 2 x 2: every realization skipped, realizations 0 .. 8
    split/...                   7 x 9 in two calls, 3 .. 39 and 40 .. 72
Key of an array: <case key>/<f32|f64>/<field>; fields: cnt (large link) or cnt0, cnt1 (pilot links: estimated, perfect CSI) with the
counter block in the order of COUNTER_KEYS, se, be, and for the pilot links err, pow (float64, compared bitwise)."""
import numpy as np

import pilot_link_oracle as po
from helpers import FLAT_COUNT, FLAT_FIRST, SEED
from oracle import modem as omodem
from pyphysim_amd import _lib

import large_pilot_cases as lp
import mimo_large_cases as ml

FIRST, COUNT, SPLIT_AT = FLAT_FIRST, FLAT_COUNT, 40
DTYPES = ("f32", "f64")
METHODS = {"mindist": _lib.DEMOD_MINDIST, "slicer": _lib.DEMOD_QAM_SLICER}
COUNTER_KEYS = ("n_realizations", "n_skipped", "n_symbols", "n_bits", "sym_errors", "sym_errors_sq", "bit_errors", "bit_errors_sq")
EDGE_COLUMNS = (1, 31, 32, 33)
SMALL = ("1x4-p3", "4x4-p9", "mmse-est-1x4")
SKIP = 0xFFFFFFFF
assert set(EDGE_COLUMNS) <= set(ml.EDGE_COLUMNS) and (5, 6) in ml.EDGE_SHAPES and (FIRST, COUNT) == (lp.FIRST, lp.COUNT)

_row = np.exp(2j * np.pi * np.array([0.0, 0.3, 0.55]))
RANK_CASE = dict(po.make_case(2, 2, 3, 6, 16.0), pilots=np.stack([_row, _row]))


def large_calls():
    """key -> (nt, nr, mmse, snr, columns, method, first, count) of mcle_run_mimo_large"""
    calls = {}
    for cid, (nt, nr, mmse, snr, ns) in zip(ml.CASE_IDS, ml.CASES):
        for mname in METHODS:
            calls["large/%s/%s" % (cid, mname)] = (nt, nr, mmse, snr, ns, mname, FIRST, COUNT)
    for ns in EDGE_COLUMNS:
        calls["edge/%d" % ns] = (5, 6, False, ml.EDGE_SNR, ns, "mindist", FIRST, COUNT)
    calls["split/large/a"] = (7, 9, False, 18.0, 34, "mindist", FIRST, SPLIT_AT - FIRST)
    calls["split/large/b"] = (7, 9, False, 18.0, 34, "mindist", SPLIT_AT, FIRST + COUNT - SPLIT_AT)
    return calls


def pilot_calls():
    """key -> (entry point, case, first, count): 'lpilot' mcle_run_mimo_large_pilot, 'pilot' mcle_run_mimo_pilot_link"""
    calls = {"lpilot/" + name: ("lpilot", lp.CASES[name], FIRST, COUNT) for name in lp.NAMES}
    for name in SMALL:
        for entry in ("lpilot", "pilot"):
            calls["%s/%s" % (entry, name)] = (entry, po.ALL_CASES[name], FIRST, COUNT)
    for entry in ("lpilot", "pilot"):
        calls["rank/" + entry] = (entry, RANK_CASE, 0, 9)
    calls["split/lpilot/a"] = ("lpilot", lp.CASES["7x9-p12"], FIRST, SPLIT_AT - FIRST)
    calls["split/lpilot/b"] = ("lpilot", lp.CASES["7x9-p12"], SPLIT_AT, FIRST + COUNT - SPLIT_AT)
    return calls


def _block(cnt):
    assert set(cnt) == set(COUNTER_KEYS), sorted(cnt)
    return np.array([cnt[k] for k in COUNTER_KEYS], dtype=np.int64)


def collect(engine):
    """Every array of the fixture from `engine`'s library: {key: ndarray}"""
    out = {}
    engine.set_constellation(po.table(), _lib.CONST_QAM)
    for key, (nt, nr, mmse, snr, ns, mname, first, count) in large_calls().items():
        for dt in DTYPES:
            cnt, se, be = engine.run_mimo_large(nt, nr, ns, 1.0 / float(omodem.dB2Linear(snr)), SEED, first, count, mmse=mmse,
                                                method=METHODS[mname], dtype=dt, per_realization=True)
            pre = "%s/%s/" % (key, dt)
            out[pre + "cnt"], out[pre + "se"], out[pre + "be"] = _block(cnt), se, be
    for key, (entry, cfg, first, count) in pilot_calls().items():
        fn = engine.run_mimo_large_pilot_link if entry == "lpilot" else engine.run_mimo_pilot_link
        for dt in DTYPES:
            c0, c1, se, be, err, pw = fn(cfg["nt"], cfg["nr"], cfg["P"], cfg["n_symbols"], cfg["noise_var"], cfg["seed"], first, count,
                                         pilot_power=cfg["pilot_power"], alpha=cfg["alpha"], pilots=cfg["pilots"], chan_factor=cfg["L"],
                                         cov=cfg["cov"], estimator=cfg["estimator"], mmse=cfg["mmse"], method=_lib.DEMOD_MINDIST,
                                         dtype=dt, per_realization=True)
            pre = "%s/%s/" % (key, dt)
            out[pre + "cnt0"], out[pre + "cnt1"], out[pre + "se"], out[pre + "be"] = _block(c0), _block(c1), se, be
            out[pre + "err"], out[pre + "pow"] = np.asarray(err, dtype=np.float64), np.asarray(pw, dtype=np.float64)
    return out
