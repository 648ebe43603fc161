"""CPU: the complex128 noise sample in two phases (csrc/bm_f64.hpp: bm_sample_fetch ends with the three table reads issued,
bm_sample_finish is the arithmetic -- the form the headline kernel's pipelined draw uses) against the one-phase sample, the
expression of csrc/philox.hpp's cn_from_words and cn_from_words_lds_pairs, as 64-bit words in both components.  The finish phase is
meant to be the one-phase functions' expressions operand for operand, so the two must agree on every word pair, not to a
tolerance.  Both are compiled for the host from the header the device includes (tests/host/bm_phase_host.cpp, no contraction);
the device's own compilation of both, with contraction on, is compared in tests/test_gpu_bm_phase.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bm_words

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA = 0.05623413251903491                     # sqrt of the noise variance at 25 dB


def phase_library(tmp_dir):
    out = os.path.join(str(tmp_dir), "libbm_phase_host.so")
    src = os.path.join(REPO, "tests", "host", "bm_phase_host.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", src, "-o", out], check=True)
    lib = ctypes.CDLL(out)
    P = ctypes.c_void_p
    lib.bm_phase_mismatches.argtypes = [P, P, ctypes.c_size_t, ctypes.c_double, P]
    lib.bm_phase_mismatches.restype = ctypes.c_size_t
    lib.bm_phase_one_batch.argtypes = [P, P, ctypes.c_size_t, ctypes.c_double, P]
    lib.bm_phase_two_batch.argtypes = [P, P, ctypes.c_size_t, ctypes.c_double, P]
    return lib


def sincos_node_boundaries():
    """the first angle word of node k + 1: node = ((x1 >> 24) + 1) >> 1 = 0 ... 128 changes at x1 = (2 k + 1) 2^24"""
    return (2 * np.arange(128, dtype=np.int64) + 1) << 24


def around_sincos_node_boundaries(radius):
    off = np.arange(-radius, radius + 1, dtype=np.int64)
    return (sincos_node_boundaries()[:, None] + off[None, :]).ravel().astype(np.uint32)


@pytest.fixture(scope="module")
def bm(tmp_path_factory):
    return phase_library(tmp_path_factory.mktemp("bm_phase"))


def _mismatches(bm, x0, x1):
    x0 = np.ascontiguousarray(x0, dtype=np.uint32)
    x1 = np.ascontiguousarray(x1, dtype=np.uint32)
    assert x0.shape == x1.shape
    first = ctypes.c_size_t(0)
    bad = bm.bm_phase_mismatches(x0.ctypes.data, x1.ctypes.data, x0.size, SIGMA, ctypes.byref(first))
    return bad, (hex(int(x0[first.value])), hex(int(x1[first.value]))) if bad else None


def test_low_radius_words_and_their_complements(bm):
    """every x0 below 2^20 and its complement, each with an angle word of its own"""
    x0 = bm_words.low_and_complement(2 ** 20)
    assert x0.size == 2 ** 21
    bad, first = _mismatches(bm, x0, bm_words.random_words(x0.size, 20271))
    assert bad == 0, (bad, first)


def test_around_every_log_node_boundary_and_the_two_ends(bm):
    x0 = np.concatenate([bm_words.around_node_boundaries(256), bm_words.ends()])
    assert x0.size > 32 * 64 * 400 and x0[-2] == 0 and x0[-1] == 2 ** 32 - 1
    bad, first = _mismatches(bm, x0, bm_words.random_words(x0.size, 20272))
    assert bad == 0, (bad, first)
    # the two ends with the two ends of the angle
    e = np.array([0, 0, 2 ** 32 - 1, 2 ** 32 - 1], dtype=np.uint32), np.array([0, 2 ** 32 - 1, 0, 2 ** 32 - 1], dtype=np.uint32)
    bad, first = _mismatches(bm, *e)
    assert bad == 0, (bad, first)


def test_around_every_sincos_node_boundary(bm):
    x1 = around_sincos_node_boundaries(256)
    assert x1.size == 128 * 513
    node = lambda w: ((w.astype(np.int64) >> 24) + 1) >> 1
    edges = sincos_node_boundaries()
    assert np.all(node(edges) == node(edges - 1) + 1)                 # the boundaries are where the node changes
    bad, first = _mismatches(bm, bm_words.random_words(x1.size, 20273), x1)
    assert bad == 0, (bad, first)


def test_random_pairs(bm):
    n = 10_000_000
    bad, first = _mismatches(bm, bm_words.random_words(n, 20274), bm_words.random_words(n, 20275))
    assert bad == 0, (bad, first)
    # ... and the comparison can fail: neighbouring words give different samples, which the two forms agree on
    x0 = np.array([12345678, 12345679, 12345678], dtype=np.uint32)
    x1 = np.array([87654321, 87654321, 87654322], dtype=np.uint32)
    a, b = np.empty(6), np.empty(6)
    bm.bm_phase_one_batch(x0.ctypes.data, x1.ctypes.data, 3, SIGMA, a.ctypes.data)
    bm.bm_phase_two_batch(x0.ctypes.data, x1.ctypes.data, 3, SIGMA, b.ctypes.data)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert a[0] != a[2] and a[1] != a[3] and a[0] != a[4] and a[1] != a[5]
    # |z| = sigma sqrt(-ln u): the value is the sample, not a constant
    u = (12345678 + 0.5) * 2.0 ** -32
    assert abs(np.hypot(a[0], a[1]) - SIGMA * np.sqrt(-np.log(u))) < 1e-15
