"""GPU: the two wavefront reductions of a 32-bit count -- csrc/common.hpp::wave_sum_u32 (six ds_bpermute_b32 round trips through the
LDS crossbar) and csrc/walk_f64.hpp::walk_wave_total (six v_add_u32 with DPP modifiers and one v_readlane_b32, no LDS) -- compared
as WORDS in one launch.  The headline complex128 kernel (csrc/pipeline_mimo_pw.hip, default form by lane row) takes its
per-realization symbol and bit error totals by the second one since round 22; eighteen other files keep the first.

Inputs: one nonzero lane at each of the 64 positions (a lane the DPP chain dropped would lose its word), all lanes 0xFFFFFFFF
(the sum wraps: 64 x (2^32 - 1) = -64 mod 2^32), and 10^4 random vectors of full 32-bit words.  Expected: 0 differences between
the two reductions in any lane, and both equal to numpy's sum modulo 2^32.  tests/gpu_src/wave_total_probe.hip is compiled at test
time (hipcc, a few seconds) with the library's flags against the headers the library is built from, as decide_probe.hip is;
nothing in the product refers to it."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = tmp_path_factory.mktemp("probe") / "libwave_total_probe.so"
    src = os.path.join(REPO, "tests", "gpu_src", "wave_total_probe.hip")
    csrc = os.path.join(REPO, "pyphysim_amd", "csrc")
    subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-gpu-rdc", "-fno-hip-fp32-correctly-rounded-divide-sqrt",
                    "-ffp-contract=fast", "-shared", "-I", csrc, "-I", os.path.join(REPO, "include"), src, "-o", str(out)], check=True)
    lib = ctypes.CDLL(str(out))
    P = ctypes.c_void_p
    lib.probe_wave_total.argtypes = [P, ctypes.c_int, P, P, P]
    lib.probe_wave_total.restype = ctypes.c_int
    return lib


def _vectors():
    one = np.zeros((64, 64), dtype=np.uint32)
    one[np.arange(64), np.arange(64)] = 0x9E3779B9 + np.arange(64, dtype=np.uint32)      # lane i alone, a word with high bits
    ones = np.full((1, 64), 0xFFFFFFFF, dtype=np.uint32)
    rs = np.random.RandomState(22)
    rnd = rs.randint(0, 1 << 32, size=(10000, 64), dtype=np.uint64).astype(np.uint32)
    return np.ascontiguousarray(np.concatenate([one, ones, rnd]))


def test_dpp_total_equals_the_bpermute_sum_word_for_word(probe, engine):
    v = _vectors()
    n = v.shape[0]
    assert n == 64 + 1 + 10000
    got_sum = np.zeros(n, dtype=np.uint32)
    got_dpp = np.zeros(n, dtype=np.uint32)
    n_diff = np.full(1, 0xFFFFFFFF, dtype=np.uint32)
    rc = probe.probe_wave_total(v.ctypes.data, n, got_sum.ctypes.data, got_dpp.ctypes.data, n_diff.ctypes.data)
    assert rc == 0, rc
    want = (v.astype(np.uint64).sum(axis=1) & 0xFFFFFFFF).astype(np.uint32)
    print("%d vectors: lanes whose bpermute sum differs from the DPP total %d, vectors off numpy's sum %d / %d" %
          (n, int(n_diff[0]), int(np.count_nonzero(got_sum != want)), int(np.count_nonzero(got_dpp != want))))
    assert int(n_diff[0]) == 0
    assert np.array_equal(got_sum, got_dpp)
    assert np.array_equal(got_dpp, want)
    assert want[64] == np.uint32((64 * 0xFFFFFFFF) & 0xFFFFFFFF)                     # the wrap-around case is what it claims to be
