"""GPU: the complex128 QAM margin certificate in fixed point (csrc/walk_f64.hpp: walk_qam_fixed4).  A group of four
decisions is vouched for by a 32-bit integer test (fraction of (t + 1/2) 2^24 at least 2 counts off either end); a group it declines
takes the f64 certificate and, behind that, the literal sweep.  The new margin is 2^-23 of the spacing where the f64 one is 2^-30,
so no count may move -- tests/test_qam_fixed_cpu.py replays the rule in exact arithmetic; here the compiled code is held to

 (i)   numpy.argmin on chosen points (tests/gpu_src/decide_probe.hip, compiled as tests/test_gpu_decide_probe.py does): that test's
       point set with the offsets 2^-21 ... 2^-27 of the spacing added, both sides of the new margin, for 16- / 64- / 256-QAM; and the
       symbol / bit counts against labels that are not the decisions;
 (ii)  the oracle chain (oracle/chains.py::chain_mimo_ofdm) and the table search (option demod_nocert = 1: no certificate at all) for
       the per-realization symbol and bit counts of run_mimo_ofdm in complex128 at 512 / 1024 / 2048 points (256 / 128 / 64
       realizations), 16- / 64- / 256-QAM, 5 dB (many clamped estimates) and 40 dB, MMSE and ZF, one and three OFDM symbols, prefix 0
       and 16, the tag of mcle_ctx_last_kernel proving the part-wave kernel's default form;
 (iii) 32 n_cu + 7 realizations against the same range in pieces of 251.
Reference: modulators/fundamental.py:241-246 (demodulate: first minimum of |r - c|), apps/mimo/simulate_mimo.py:68-142."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import chains, modem as omodem
from pyphysim_amd import _lib

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1380649
WDEC_QAM_CERT = 2


# ---- (i) chosen points ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    out = tmp_path_factory.mktemp("probe_fixed") / "libdecide_probe.so"
    src = os.path.join(REPO, "tests", "gpu_src", "decide_probe.hip")
    csrc = os.path.join(REPO, "pyphysim_amd", "csrc")
    subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-gpu-rdc", "-fno-hip-fp32-correctly-rounded-divide-sqrt",
                    "-ffp-contract=fast", "-shared", "-I", csrc, "-I", os.path.join(REPO, "include"), src, "-o", str(out)], check=True)
    lib = ctypes.CDLL(str(out))
    P = ctypes.c_void_p
    lib.probe_walk_decide.argtypes = [P, ctypes.c_int, P, P, ctypes.c_int, P, P]
    lib.probe_walk_decide.restype = ctypes.c_int
    return lib


def _argmin(table, pts):
    d = (pts.real[:, None] - table.real[None, :]) ** 2 + (pts.imag[:, None] - table.imag[None, :]) ** 2
    return np.argmin(d, axis=1).astype(np.int32)


def _points(table, seed):
    """The point set of tests/test_gpu_decide_probe.py (bisector points of every pair of neighbours moved off the boundary by +-2^-k
    of the spacing, exact ties on the symmetry axes, the constellation itself, rings far outside, random points) with
    k = 21 ... 27 added to its k = 20, 29, 30, 31, 33, 38, 42: the fixed-point test declines below 2^-23, the f64 one below 2^-30."""
    rs = np.random.RandomState(seed)
    M = table.size
    dmin = np.min(np.abs(table[:, None] - table[None, :]) + 1e9 * np.eye(M))
    offs = [2.0 ** -k for k in (20, 21, 22, 23, 24, 25, 26, 27, 29, 30, 31, 33, 38, 42)]
    pts = [table.copy()]
    for i in range(M):
        order = np.argsort(np.abs(table - table[i]))[1:9]
        for j in order:
            if j < i:
                continue
            mid, u = 0.5 * (table[i] + table[j]), (table[j] - table[i]) / abs(table[j] - table[i])
            for along in (0.0, 0.25, -0.4, 1.0, -3.0):
                base = mid + 1j * u * along * dmin
                for o in offs:
                    pts += [np.array([base + u * o * dmin, base - u * o * dmin])]
    ext = np.max(np.abs(table))
    t = rs.uniform(-1.2, 1.2, 600) * ext
    pts += [1j * t, np.zeros(1, dtype=complex), t + 0j]           # a square QAM is mirror-symmetric about both axes: exact ties
    ang = rs.uniform(0, 2 * np.pi, 400)
    for r in (1.5, 4.0, 50.0, 300.0, 1100.0):
        pts += [r * ext * np.exp(1j * ang)]
    pts += [(rs.uniform(-1.3, 1.3, 4000) + 1j * rs.uniform(-1.3, 1.3, 4000)) * ext]
    p = np.concatenate(pts).astype(np.complex128)
    return p[: 4 * (p.size // 4)]


def _probe_run(probe, engine, pts, tx):
    n_groups = pts.size // 4
    pv = np.ascontiguousarray(pts.view(np.float64))
    tv = np.ascontiguousarray(tx.astype(np.int32))
    se = np.zeros(n_groups, dtype=np.uint32)
    be = np.zeros(n_groups, dtype=np.uint32)
    dec = probe.probe_walk_decide(engine.ctx, _lib.DEMOD_MINDIST, pv.ctypes.data, tv.ctypes.data, n_groups, se.ctypes.data, be.ctypes.data)
    assert dec == WDEC_QAM_CERT, dec
    return se, be


@pytest.mark.parametrize("M", [16, 64, 256])
def test_decisions_on_both_sides_of_the_new_margin(probe, engine, M):
    table = np.asarray(chains.constellation("qam", M), dtype=np.complex128)
    engine.set_constellation(table, _lib.CONST_QAM)
    pts = _points(table, 29 + M)
    want = _argmin(table, pts)
    se, be = _probe_run(probe, engine, pts, want)
    bad = np.flatnonzero(se)
    print("%d-QAM: %d points, %d groups with a wrong decision" % (M, pts.size, bad.size))
    assert bad.size == 0, (bad[:5], pts[4 * bad[0]: 4 * bad[0] + 4], want[4 * bad[0]: 4 * bad[0] + 4])
    assert not be.any()
    # the counts against labels that are NOT the decisions: every symbol / bit of the difference is counted
    bits = np.array([bin(v).count("1") for v in range(256)], dtype=np.int64)
    tx = np.random.RandomState(7).randint(0, M, size=pts.size).astype(np.int32)
    se, be = _probe_run(probe, engine, pts, tx)
    x = (tx ^ want).reshape(-1, 4)
    assert np.array_equal(se, (x != 0).sum(axis=1)) and np.array_equal(be, bits[x].sum(axis=1))


# ---- (ii), (iii) the link ----------------------------------------------------------------------------------------------------------
CASES = [dict(M=64, snr_db=40.0),                                               # MMSE, prefix 16, one symbol
         dict(M=16, snr_db=5.0, cp_size=0, mmse=False, n_ofdm_sym=3),           # ZF, no prefix, three symbols
         dict(M=256, snr_db=40.0, cp_size=0, mmse=False),                       # ZF, no prefix, one symbol
         dict(M=256, snr_db=5.0),                                               # MMSE, prefix 16, one symbol
         dict(M=64, snr_db=5.0, cp_size=0, mmse=False),                         # ZF, no prefix, one symbol
         dict(M=16, snr_db=40.0, n_ofdm_sym=3)]                                 # MMSE, prefix 16, three symbols
DEPTH = {512: 256, 1024: 128, 2048: 64}


def _set(engine, kw):
    engine.set_constellation(chains.constellation("qam", kw["M"]), _lib.CONST_QAM)


def _run(engine, kw, fft, first, count, **opts):
    nv = 1.0 / omodem.dB2Linear(kw["snr_db"])
    with engine.options(**opts):
        out = engine.run_mimo_ofdm(4, 4, fft, kw.get("cp_size", 16), fft, kw.get("n_ofdm_sym", 1), nv, SEED, first, count,
                                   mmse=kw.get("mmse", True), method=_lib.DEMOD_MINDIST, dtype="f64", per_realization=True)
        return out + (engine.last_kernel(),)


@functools.lru_cache(maxsize=None)
def _oracle(case, fft):
    """computed once per (case, size); the arrays are not written to"""
    kw = CASES[case]
    first, count = (1 << 33) + 7919 * case, DEPTH[fft]
    okw = dict(mod="qam", M=kw["M"], nt=4, nr=4, fft_size=fft, cp_size=kw.get("cp_size", 16), num_used=fft,
               n_ofdm_sym=kw.get("n_ofdm_sym", 1), snr_db=kw["snr_db"], mmse=kw.get("mmse", True))
    want = [chains.chain_mimo_ofdm(chains.PhiloxRng(SEED, r), **okw) for r in range(first, first + count)]
    se, be = np.array([w["symbol_errors"] for w in want]), np.array([w["bit_errors"] for w in want])
    se.setflags(write=False)
    be.setflags(write=False)
    return first, count, se, be


@pytest.mark.parametrize("fft", [512, 1024, 2048])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_counts_equal_the_oracle_and_the_table_search(engine, case, fft):
    kw = CASES[case]
    _set(engine, kw)
    first, count, want_se, want_be = _oracle(case, fft)
    if kw["snr_db"] < 30.0:
        assert want_se.sum() > 100
    res, se, be, tag = _run(engine, kw, fft, first, count)
    res_n, se_n, be_n, tag_n = _run(engine, kw, fft, first, count, demod_nocert=1)
    print("case %d fft %d: %s / %s, symbol errors %d / %d (oracle %d)" %
          (case, fft, tag, tag_n, int(se.sum()), int(se_n.sum()), int(want_se.sum())))
    assert tag == "mimo_ofdm_pw<%d>/freq" % (fft // 256)
    assert np.array_equal(se, want_se), np.flatnonzero(se != want_se)[:5]
    assert np.array_equal(be, want_be), np.flatnonzero(be != want_be)[:5]
    assert np.array_equal(se_n, want_se) and np.array_equal(be_n, want_be)
    assert res["n_realizations"] == count and res["n_skipped"] == 0
    assert res["sym_errors"] == int(want_se.sum()) and res["bit_errors"] == int(want_be.sum())


@pytest.mark.parametrize("fft", [512, 1024, 2048])
def test_later_passes_equal_the_range_in_pieces(engine, fft):
    """32 n_cu + 7 realizations: every workgroup of the persistent grid takes several in turn; the same range in pieces of 251"""
    kw = CASES[1]                                                   # 5 dB, three symbols: every realization counts errors
    _set(engine, kw)
    first, n, piece = 6626070, 32 * engine.n_cu + 7, 251
    res, se, be, tag = _run(engine, kw, fft, first, n)
    assert tag == "mimo_ofdm_pw<%d>/freq" % (fft // 256)
    assert se.shape == (n,) and se.min() > 0
    se_p, be_p = np.empty_like(se), np.empty_like(be)
    for off in range(0, n, piece):
        k = min(piece, n - off)
        _, se_p[off:off + k], be_p[off:off + k], _ = _run(engine, kw, fft, first + off, k)
    print("fft %d: %d realizations, symbol errors %d / %d in pieces" % (fft, n, int(se.sum()), int(se_p.sum())))
    assert np.array_equal(se, se_p) and np.array_equal(be, be_p)
    assert res["n_realizations"] == n and res["sym_errors"] == int(se_p.sum()) and res["bit_errors"] == int(be_p.sum())
