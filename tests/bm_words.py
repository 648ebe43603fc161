"""The 32-bit words the two forms of -ln((x0 + 0.5) 2^-32) (csrc/bm_f64.hpp: bm_neg_log, bm_neg_log_q) are compared on, shared by
tests/test_bm_logq_cpu.py (every word of every range) and tests/test_gpu_bm_logq.py (the ranges thinned, the edges whole), and
the host build of both forms (tests/host/bm_logq_host.cpp).

The argument reduction can go wrong where the double x0 + 0.5 changes shape: at the powers of two (the exponent and the shift of
the fraction change), at the node boundaries of each binade (the fraction f = k 2^26 + 2^25: the node, the sign of the residual
and, at k = 31, the fold change) and at the two ends (x0 = 0: the only double below 1; x0 = 2^32 - 1: node 64 of the top binade)."""
import ctypes
import os
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = 2 ** 32


def _clip(w):
    w = np.asarray(w, dtype=np.int64).ravel()
    return w[(w >= 0) & (w < FULL)].astype(np.uint32)


def low_and_complement(n):
    """every word below n and its complement"""
    w = np.arange(n, dtype=np.int64)
    return _clip(np.concatenate([w, FULL - 1 - w]))


def around_powers_of_two(radius, step=1):
    """2^b - radius ... 2^b + radius for b = 0 ... 32, every step-th word and always the three at the power itself"""
    off = np.arange(-radius, radius + 1, step, dtype=np.int64)
    off = np.union1d(off, np.array([-1, 0, 1]))
    return _clip(np.concatenate([(1 << b) + off for b in range(33)]))


def node_boundaries():
    """the first word of node k + 1 in the binade [2^b, 2^(b+1)): x0 + 0.5 >= 2^b (1 + (2 k + 1) / 128), b = 0 ... 31, k = 0 ... 63"""
    b = np.arange(32, dtype=np.int64)[:, None]
    k = np.arange(64, dtype=np.int64)[None, :]
    return (((129 + 2 * k) << b) >> 7).ravel()


def around_node_boundaries(radius):
    off = np.arange(-radius, radius + 1, dtype=np.int64)
    return _clip(node_boundaries()[:, None] + off[None, :])


def ends():
    return np.array([0, FULL - 1], dtype=np.uint32)


def random_words(n, seed):
    return np.random.RandomState(seed).randint(0, FULL, size=n, dtype=np.uint64).astype(np.uint32)


def host_library(tmp_dir):
    """tests/host/bm_logq_host.cpp compiled without contraction: the header's own expressions, one rounding per operation"""
    out = os.path.join(str(tmp_dir), "libbm_logq_host.so")
    src = os.path.join(REPO, "tests", "host", "bm_logq_host.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", src, "-o", out], check=True)
    lib = ctypes.CDLL(out)
    P = ctypes.c_void_p
    lib.bm_neg_log_batch.argtypes = [P, P, ctypes.c_size_t]
    lib.bm_neg_log_q_batch.argtypes = [P, P, ctypes.c_size_t]
    lib.bm_neg_log_q_mismatches.argtypes = [P, ctypes.c_size_t, P]
    lib.bm_neg_log_q_mismatches.restype = ctypes.c_size_t
    lib.bm_neg_log_q_mismatches_range.argtypes = [ctypes.c_uint64, ctypes.c_uint64, P]
    lib.bm_neg_log_q_mismatches_range.restype = ctypes.c_size_t
    lib.bm_log_table.restype = ctypes.POINTER(ctypes.c_double * 130)
    lib.bm_logq_table.restype = ctypes.POINTER(ctypes.c_double * 130)
    return lib
