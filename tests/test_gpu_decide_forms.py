"""GPU: the decision forms the fused pipelines decide with, on points CHOSEN BY THE TEST (tests/test_gpu_decide_probe.py does this for
walk_decide<double, DEC, 4> alone).  tests/gpu_src/decide_forms_probe.hip is compiled at test time (hipcc, ~10 s) against the headers
the library is built from and runs, one launch per form:
  * demod_multi_cert<T, K> around demod_grid4_multi<K> / demod_mindist_multi<K> on the float4 table {re, im, |c|^2/2} (two-FMA metric,
    both ways the pipelines fill |c|^2/2) and the single-symbol demod_grid4, K = 1 ... 4 -- the complex64 decision of the pipelines;
  * demod_multi_cert<double, K> around demod_grid_multi<K> / demod_mindist_multi<K> on double2 -- the complex128 lockstep search;
  * walk_decide<T, DEC, N>, T = float / double, every DEC, N = 2 / 4 / 6: the packed v_cvt_pk_u8_f32 slicer with its `live` mask on the
    partial last word of N = 2 and 6, the level-domain forms at N = 4, the straight-line forms at N % 4 != 0, the complex64
    certificates with their own ranges.
tests/decide_points.py says how tables, points, the three grouping orders, the float64 / longdouble reference and the rounding bounds
are made, and tests/test_decide_forms_cpu.py proves on the CPU that the orders mix certified with uncertified points and short with
long candidate lists inside a group, and that at most a quarter of the complex64 points is unclear.  Rules:
  (a) against the reference: its label on every clear point and on every exact tie (first index), one of the nearest within the
      metric's rounding bound on every other point -- no point is left unchecked;
  (c) form against form, bit for bit, on EVERY point, for every K and every order: the label of a point depends neither on its
      neighbours in the group nor on K; grid search == sweep == single-symbol search; certificates on == demod_nocert=1; the counts of
      the generic walk == the counts implied by the demodulate operator;
  (d) counts: zero against the reference labels on clear points, the popcount of the XOR against random sent labels for N = 2, 4, 6
      (a padding slot of a partial word is never counted);
  (e) the WDEC_* form the library would compile, per table, method and arithmetic.
All probe points are finite (NaN / infinity: see decide_points).

What the first run found (fixed in csrc/modem.hpp dist2): demod_grid_multi_search on double2 with K >= 2 and walk_sweep<float> gave an
exact tie between mirror images or duplicates to the LATER index -- 64-QAM complex128 at (-0, -1.4186162239480016): 47 for 42;
duplicates8 at 144 points: 1 for 0; QPSK complex64 walk at (0, 0.06184394): the runner-up counted as an error -- because the compiler
fused a different product of dx * dx + dy * dy into the sum for the first candidate than for the others.  "Certificates on ==
demod_nocert=1" held on every complex64 point, unclear ones included, with both fills of |c|^2/2."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import decide_points as dp
from pyphysim_amd import _lib

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WDEC = {0: "generic", 1: "slicer", 2: "qam_cert", 3: "quad_cert", 4: "axis4_cert"}
GRID4_MULTI, MINDIST4_MULTI, GRID_MULTI, MINDIST_MULTI, GRID4 = 0, 1, 2, 3, 4
BITS = np.array([bin(v).count("1") for v in range(256)], dtype=np.int64)
CASES = [(n, d) for n in dp.NAMES for d in dp.DTYPES]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    out = tmp_path_factory.mktemp("forms_probe") / "libdecide_forms_probe.so"
    src = os.path.join(REPO, "tests", "gpu_src", "decide_forms_probe.hip")
    csrc = os.path.join(REPO, "pyphysim_amd", "csrc")
    subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-gpu-rdc", "-fno-hip-fp32-correctly-rounded-divide-sqrt",
                    "-ffp-contract=fast", "-shared", "-I", csrc, "-I", os.path.join(REPO, "include"), src, "-o", str(out)], check=True)
    lib = ctypes.CDLL(str(out))
    P, I = ctypes.c_void_p, ctypes.c_int
    lib.probe_multi.argtypes = [P, I, I, I, I, P, I, P]
    lib.probe_multi.restype = I
    lib.probe_walk.argtypes = [P, I, I, I, P, P, I, P, P]
    lib.probe_walk.restype = I
    return lib


def _status(rc):
    """a HIP error from the probe ends the session: nothing more is started on a device that has just faulted"""
    if rc <= -1000:
        pytest.exit("decide_forms_probe: HIP error %d" % (-1000 - rc), returncode=3)
    return rc


def _device_points(pts, dtype):
    return np.ascontiguousarray(pts.astype(np.complex64 if dtype == "f32" else np.complex128))


def _multi(probe, engine, dtype, form, K, half_form, pts):
    arr = _device_points(pts, dtype)
    lab = np.full(arr.size, -1, dtype=np.int32)
    rc = _status(probe.probe_multi(engine.ctx, _lib.dtype_code(dtype), form, K, half_form, arr.ctypes.data, arr.size, lab.ctypes.data))
    assert rc == 0, rc
    return lab


def _walk(probe, engine, dtype, method, N, pts, tx):
    arr = _device_points(pts, dtype)
    n_groups = arr.size // N
    tv = np.ascontiguousarray(tx.astype(np.int32))
    se, be = np.zeros(n_groups, dtype=np.uint32), np.zeros(n_groups, dtype=np.uint32)
    dec = _status(probe.probe_walk(engine.ctx, _lib.dtype_code(dtype), method, N, arr.ctypes.data, tv.ctypes.data, n_groups, se.ctypes.data, be.ctypes.data))
    assert dec >= 0, dec
    return WDEC[dec], se.astype(np.int64), be.astype(np.int64)


def _show(c, idx, *labels):
    i = int(idx[0])
    return "%s %s: %d points differ, first %d = %r, cell count %d, certified %s, reference %d, labels %s" % (
        c.name, c.dtype, idx.size, i, c.pts[i], c.counts[i], c.sure[i], c.ref.best[i], [int(l[i]) for l in labels])


@pytest.mark.parametrize("name,dtype", CASES, ids=["%s-%s" % nd for nd in CASES])
def test_lockstep_searches_on_chosen_points(probe, engine, name, dtype):
    c = dp.case(name, dtype)
    engine.set_constellation(c.table, c.kind)
    forms = (GRID4_MULTI, MINDIST4_MULTI) if dtype == "f32" else (GRID_MULTI, MINDIST_MULTI)
    metric = "two_fma" if dtype == "f32" else "literal"
    for half_form in ((0, 1) if dtype == "f32" else (0,)):
        anchors = {}
        for nocert in (0, 1):
            with engine.options(demod_nocert=nocert):
                # the single-symbol anchor: demod_grid4 (complex64), the demodulate operator (complex128)
                anchor = (_multi(probe, engine, dtype, GRID4, 1, half_form, c.pts) if dtype == "f32"
                          else engine.demodulate(c.pts, dtype="f64").astype(np.int32))
                for form in forms:
                    for K in dp.KS:
                        for oname, order in c.orders.items():
                            got = np.empty_like(anchor)
                            got[order] = _multi(probe, engine, dtype, form, K, half_form, c.pts[order])
                            bad = np.flatnonzero(got != anchor)
                            assert bad.size == 0, ("form %d K %d %s nocert %d half %d" % (form, K, oname, nocert, half_form), _show(c, bad, got, anchor))
            wrong = c.ref.wrong(anchor, metric)                         # (a): every form equals the anchor, bit for bit
            assert wrong.size == 0, ("nocert %d half %d" % (nocert, half_form), _show(c, wrong, anchor))
            anchors[nocert] = anchor
        diff = np.flatnonzero(anchors[0] != anchors[1])
        print("%s %s half form %d: %d points, certificate and search differ on %d" % (name, dtype, half_form, c.pts.size, diff.size))
        assert diff.size == 0, _show(c, diff, anchors[0], anchors[1])     # certificates on == demod_nocert=1, on every point


@pytest.mark.parametrize("name,dtype", CASES, ids=["%s-%s" % nd for nd in CASES])
def test_walk_decide_on_chosen_points(probe, engine, name, dtype):
    c = dp.case(name, dtype)
    engine.set_constellation(c.table, c.kind)
    rs = np.random.RandomState(5)
    sent = rs.randint(0, c.M, size=c.pts.size).astype(np.int64)
    clear_lit = c.ref.decided["literal"]
    runs = [(_lib.DEMOD_MINDIST, 0, c.walk_form, clear_lit), (_lib.DEMOD_MINDIST, 1, "generic", clear_lit)]
    if c.kind == _lib.CONST_QAM:
        runs.append((_lib.DEMOD_QAM_SLICER, 0, "slicer", c.ref.slicer_clear()))
    reached = set()
    for method, nocert, want_form, clear in runs:
        with engine.options(demod_nocert=nocert):
            # the demodulate operator: the literal metric behind the same certificates -- (a) for it, then the anchor of the generic walk
            op = engine.demodulate(_device_points(c.pts, dtype), dtype=dtype) if method == _lib.DEMOD_MINDIST else None
            if op is not None:
                wrong = c.ref.wrong(op, "literal")
                assert wrong.size == 0, ("demodulate nocert %d" % nocert, _show(c, wrong, op))
            for N in dp.NS:
                for oname, order in c.orders.items():
                    what = "method %d nocert %d N %d %s" % (method, nocert, N, oname)
                    pts, want, tx = c.pts[order], c.ref.best[order], sent[order]
                    unclear = (~clear[order]).reshape(-1, N).sum(axis=1)
                    whole = unclear == 0
                    form, se, be = _walk(probe, engine, dtype, method, N, pts, want)
                    assert form == want_form, (what, form)                                   # (e)
                    reached.add(form)
                    # (d) against the reference labels: nothing on clear points (at most the unclear points of a group anywhere)
                    bad = np.flatnonzero((se > unclear) | (whole & (be != 0)))
                    assert bad.size == 0, (what, bad[:5], pts[N * bad[0]: N * bad[0] + N], want[N * bad[0]: N * bad[0] + N])
                    # ... and against labels that are NOT the decisions: every symbol / bit of the difference, and no padding slot
                    _, se, be = _walk(probe, engine, dtype, method, N, pts, tx)
                    x = (tx ^ want).reshape(-1, N)
                    bad = np.flatnonzero(whole & ((se != (x != 0).sum(axis=1)) | (be != BITS[x].sum(axis=1))))
                    assert bad.size == 0, (what, bad[:5], pts[N * bad[0]: N * bad[0] + N])
                    if form == "generic":                                                  # (c): demod_one here and in the operator
                        x = (tx ^ op[order]).reshape(-1, N)
                        bad = np.flatnonzero((se != (x != 0).sum(axis=1)) | (be != BITS[x].sum(axis=1)))
                        assert bad.size == 0, (what, bad[:5], pts[N * bad[0]: N * bad[0] + N])
    print("%s %s: walk forms %s" % (name, dtype, sorted(reached)))
