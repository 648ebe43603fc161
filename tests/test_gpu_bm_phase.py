"""GPU: the complex128 noise sample in two phases (csrc/philox.hpp: cn_fetch_lds_pairs + cn_finish, the form the headline kernel's
pipelined draw uses) against cn_from_words_lds_pairs, the one-phase form every other pipeline keeps -- ON THE DEVICE.  The library
is compiled with contraction on: the one-phase form fuses ang - theta_k with the product in front of it into one v_fma_f64, and
the split form has to compile to the same fusions.  The host build (tests/test_bm_phase_cpu.py) has no contraction and cannot
show that; tests/gpu_src/bm_phase_probe.hip, compiled at test time with the library's flags against the library's headers,
evaluates both forms from one LDS copy of the tables in one launch and compares them as 64-bit words in the kernel: zero
differences in either component."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import bm_words
from test_bm_phase_cpu import SIGMA, around_sincos_node_boundaries, phase_library

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    out = tmp_path_factory.mktemp("bm_phase_probe") / "libbm_phase_probe.so"
    src = os.path.join(REPO, "tests", "gpu_src", "bm_phase_probe.hip")
    csrc = os.path.join(REPO, "pyphysim_amd", "csrc")
    subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-gpu-rdc", "-fno-hip-fp32-correctly-rounded-divide-sqrt",
                    "-ffp-contract=fast", "-shared", "-I", csrc, "-I", os.path.join(REPO, "include"), src, "-o", str(out)], check=True)
    lib = ctypes.CDLL(str(out))
    P = ctypes.c_void_p
    lib.probe_bm_phase.argtypes = [P, P, ctypes.c_size_t, ctypes.c_double, P, ctypes.c_size_t, P, P]
    lib.probe_bm_phase.restype = ctypes.c_int
    return lib


def _probe_pairs():
    """The word pairs of tests/test_bm_phase_cpu.py with the long range thinned (every fourth word below 2^20 and of the complements),
    the edges whole (the two ends, +-256 around every log node boundary of every binade, +-256 around every sincos node boundary)
    and 1e6 random pairs -- in a fixed random order, so that the first 1e5 (the ones compared with the host build) sample all."""
    low = bm_words.low_and_complement(2 ** 20)
    x0_sets = [low[::4], low[:4096], low[2 ** 20:2 ** 20 + 4096], bm_words.around_node_boundaries(256), bm_words.ends()]
    x0 = np.concatenate(x0_sets)
    x1 = bm_words.random_words(x0.size, 20281)
    t1 = around_sincos_node_boundaries(256)
    t0 = bm_words.random_words(t1.size, 20282)
    corners = np.array([0, 0, 2 ** 32 - 1, 2 ** 32 - 1], dtype=np.uint32), np.array([0, 2 ** 32 - 1, 0, 2 ** 32 - 1], dtype=np.uint32)
    x0 = np.concatenate([x0, t0, corners[0], bm_words.random_words(1_000_000, 20283)])
    x1 = np.concatenate([x1, t1, corners[1], bm_words.random_words(1_000_000, 20284)])
    order = np.random.RandomState(11).permutation(x0.size)
    return np.ascontiguousarray(x0[order]), np.ascontiguousarray(x1[order])


def test_both_forms_agree_on_the_device(probe, engine, tmp_path):
    x0, x1 = _probe_pairs()
    n, n_out = x0.size, 100_000
    assert 2_400_000 < n < 4_000_000
    assert np.isin(np.array([0, 2 ** 32 - 1], dtype=np.uint32), x0).all() and np.isin(np.array([1 << 24, 255 << 24], dtype=np.uint32), x1).all()
    out = np.full(2 * n_out, np.nan)
    diffs = np.zeros(2, dtype=np.uint64)
    first = np.zeros(1, dtype=np.uint64)
    rc = probe.probe_bm_phase(x0.ctypes.data, x1.ctypes.data, n, SIGMA, out.ctypes.data, n_out, diffs.ctypes.data, first.ctypes.data)
    assert rc == 0, rc
    print("%d word pairs: differences real %d, imaginary %d" % (n, int(diffs[0]), int(diffs[1])))
    i = min(int(first[0]), n - 1)
    assert not diffs.any(), (diffs.tolist(), hex(int(x0[i])), hex(int(x1[i])))
    assert int(first[0]) == n
    # ... and the kernel ran on these words: its samples are the host build's to the last place or two (the device contracts, the
    # host build does not: values, not words), and they are samples, not a constant
    host = phase_library(tmp_path)
    want = np.empty(2 * n_out)
    h0, h1 = np.ascontiguousarray(x0[:n_out]), np.ascontiguousarray(x1[:n_out])
    host.bm_phase_one_batch(h0.ctypes.data, h1.ctypes.data, n_out, SIGMA, want.ctypes.data)
    assert np.all(np.isfinite(out))
    assert np.max(np.abs(out - want)) <= 4 * np.spacing(SIGMA * np.sqrt(-np.log(2.0 ** -33)))
    assert np.unique(out).size > 0.99 * out.size
