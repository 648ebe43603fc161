"""CPU: bm_neg_log_q (csrc/bm_f64.hpp) -- the -ln u of the complex128 Box-Muller with its argument reduction in integer
arithmetic -- against bm_neg_log, the form tests/test_bm_f64_cpu.py pins to NumPy, as 64-bit words: the numerator m - c_j is the
integer d = (low 26 bits of the mantissa's fraction, sign-extended) times 2^-32 (2^-33 on a folded node) EXACTLY, that power of
two sits in the table kBmLogQ, and a power-of-two scale commutes with the one rounding of the product -- so the two forms must
agree on every word, not to a tolerance.  Both are compiled for the host from the header the device includes
(tests/host/bm_logq_host.cpp, no contraction); the device's own compilation of both is compared in tests/test_gpu_bm_logq.py."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

import bm_words

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bm(tmp_path_factory):
    return bm_words.host_library(tmp_path_factory.mktemp("bm_logq"))


def _mismatches(bm, words):
    words = np.ascontiguousarray(words, dtype=np.uint32)
    first = ctypes.c_uint32(0)
    return bm.bm_neg_log_q_mismatches(words.ctypes.data, words.size, ctypes.byref(first)), first.value


def test_low_words_and_their_complements(bm):
    """every word below 2^20 (the binades where the fraction's low bits are all zero) and its complement (u -> 1: nodes 63 / 64)"""
    bad, first = _mismatches(bm, bm_words.low_and_complement(2 ** 20))
    assert bad == 0, (bad, hex(first))


def test_around_every_power_of_two(bm):
    words = bm_words.around_powers_of_two(2 ** 16)
    assert words.size > 24 * 2 ** 17                       # (the low powers' ranges overlap and are clipped at 0)
    bad, first = _mismatches(bm, words)
    assert bad == 0, (bad, hex(first))


def test_around_every_node_boundary_of_every_binade(bm):
    edges = bm_words.node_boundaries()
    assert edges.size == 32 * 64
    # the boundaries are where the witness changes node: (mant + 0x2000) >> 14 of the double x0 + 0.5 (binades of >= 2^7 words)
    big = edges[edges >= 2 ** 8]
    hi = lambda w: (w.astype(np.float64) + 0.5).view(np.uint64) >> np.uint64(32)
    node = lambda w: ((hi(w) & np.uint64(0xFFFFF)) + np.uint64(0x2000)) >> np.uint64(14)
    assert np.all(node(big) == node(big - 1) + 1)
    bad, first = _mismatches(bm, bm_words.around_node_boundaries(256))
    assert bad == 0, (bad, hex(first))


def test_the_two_ends_and_random_words(bm):
    bad, first = _mismatches(bm, bm_words.ends())
    assert bad == 0, hex(first)
    bad, first = _mismatches(bm, bm_words.random_words(10_000_000, 20261))
    assert bad == 0, (bad, hex(first))
    # ... and the comparison can fail: the witness's own values differ between neighbouring words
    w = np.array([12345678, 12345679], dtype=np.uint32)
    a, b = np.empty(2), np.empty(2)
    bm.bm_neg_log_batch(w.ctypes.data, a.ctypes.data, 2)
    bm.bm_neg_log_q_batch(w.ctypes.data, b.ctypes.data, 2)
    assert a[0] != a[1] and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_table_is_the_old_one_scaled_by_a_power_of_two(bm):
    """kBmLogQ = {ldexp(1 / c_j, -32 or -33 from node 32 on), ln c_j}: entry by entry from the compiled header, from the generator,
    and the generated header holds nothing the generator does not write"""
    old = np.array(bm.bm_log_table().contents).reshape(65, 2)
    new = np.array(bm.bm_logq_table().contents).reshape(65, 2)
    shift = np.where(np.arange(65) >= 32, -33, -32)
    assert np.array_equal(new[:, 0].view(np.uint64), np.ldexp(old[:, 0], shift).view(np.uint64))
    assert np.array_equal(new[:, 1].view(np.uint64), old[:, 1].view(np.uint64))
    spec = importlib.util.spec_from_file_location("gen_bm_tables", os.path.join(REPO, "scripts", "gen_bm_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    inv, lnc = gen.tables()[:2]
    assert np.array_equal(gen.log_q(inv), new[:, 0]) and np.array_equal(inv, old[:, 0]) and np.array_equal(lnc, new[:, 1])
    text = open(os.path.join(REPO, "pyphysim_amd", "csrc", "bm_tables.hpp")).read()
    body = re.search(r"kBmLogQ\[65 \* 2\] = \{(.*?)\};", text, re.S).group(1)
    vals = np.array([float.fromhex(t) for t in body.replace("\n", " ").split(",") if t.strip()])
    assert np.array_equal(vals.reshape(65, 2), new)
