"""The lane map of the part-wave kernel's ROWS form (csrc/pipeline_mimo_pw.hip, round 10), replayed in NumPy -- no GPU.

A workgroup of NW wavefronts is one realization of N = 256 NW points and four receive antennas.  The 4 NW (antenna, time class) partial
transforms, flattened f = NW antenna + class, are dealt f = 4 w + rho to lane row rho = lane >> 4 of wavefront w; register c of lane
(rho, h) holds sample NW pw_mtime(h, c) + class of that antenna.  Every lane draws eight Philox NOISE blocks (even rows: those of
registers cc < 8, odd rows: those of registers 8 + cc), X = (w0, w1), Y = (w2, w3), and v_permlane16_swap changes X of the odd rows
with Y of the even rows sixteen lanes below.  The replay shows

* every sample of every antenna is drawn exactly once, and after the swap X is the word pair of register cc and Y that of register
  8 + cc in all 64 lanes -- the block i // 2 and the word pair 2 (i % 2) of the flat sample index i, as oracle/philox.py::cnormal
  draws them (offset = antenna x n_ofdm_sym (N + cp) + symbol (N + cp) + cp + n);
* the exchange: wavefront w leaves element k' of its row rho in slice f of the planes (+ 16 doubles for an odd antenna) and lane
  (r, g) of wavefront jw reads class jj of antenna r at k' = g + 16 (UU jw + uu) -- every bin k' + 256 q reaches the lane that
  finishes it, no two writers share a double, and the two rows of a reading half-wave sit on different halves of the bank row."""
import itertools

import numpy as np
import pytest

K_PLANE = 4 * 272                      # doubles per wavefront plane (kPwPlane)


def pw_mtime(h, c):
    return (c & 3) * 64 + (c >> 2) * 16 + (h & 3) * 4 + (h >> 2)


def pair_of(nw, w, rho):
    f = 4 * w + rho
    return f // nw, f % nw             # antenna, class


def permlane16_swap(x, y):
    """v_permlane16_swap_b32 x, y over 64 lanes: rows 1 and 3 of x change places with rows 0 and 2 of y"""
    x, y = x.copy(), y.copy()
    for lo in (0, 32):
        t = x[lo + 16:lo + 32].copy()
        x[lo + 16:lo + 32] = y[lo:lo + 16]
        y[lo:lo + 16] = t
    return x, y


@pytest.mark.parametrize("nw,cp,n_sym", [(nw, cp, ns) for nw in (2, 4, 8) for cp, ns in ((0, 1), (16, 3))])
def test_every_sample_is_drawn_once_with_the_contracts_block_and_word(nw, cp, n_sym):
    n = 256 * nw
    row = n_sym * (n + cp)
    lane = np.arange(64)
    rho, h = lane >> 4, lane & 15
    for os_ in range(n_sym):
        seen = np.zeros((4, n), dtype=np.int64)
        for w in range(nw):
            ant, cls = zip(*(pair_of(nw, w, int(r)) for r in rho))
            ant, cls = np.array(ant), np.array(cls)
            assert np.array_equal(cls & 1, rho & 1)                     # even / odd classes are even / odd rows
            assert np.array_equal(ant[rho == 0], ant[rho == 1]) and np.array_equal(ant[rho == 2], ant[rho == 3])
            # the kernel's counter: the even sample of the pair, block i00 / 2 + (NW / 2) pw_mtime(0, cc)
            i00 = ant * row + os_ * (n + cp) + cp + (cls & ~1) + 32 * nw * (rho & 1) + nw * pw_mtime(h, 0)
            assert not (i00 & 1).any()
            for cc in range(8):
                blk = (i00 >> 1) + (nw // 2) * pw_mtime(0, cc)
                # a word pair is (block, 0) = words 0, 1 or (block, 1) = words 2, 3
                x, y = permlane16_swap(2 * blk + 0, 2 * blk + 1)
                for c, got in ((cc, x), (8 + cc, y)):
                    t = nw * pw_mtime(h, c) + cls                       # the sample register c holds
                    i = ant * row + os_ * (n + cp) + cp + t             # its flat index: oracle.philox.cnormal's pos
                    assert np.array_equal(got, 2 * (i // 2) + (i % 2)), (w, cc, c)
                    np.add.at(seen, (ant, t), 1)
        assert (seen == 1).all()


@pytest.mark.parametrize("nw", [2, 4, 8])
def test_draws_of_a_lane_pair_do_not_repeat(nw):
    """The sixteen blocks of a lane pair (rho, rho + 1) are drawn eight by each lane: 8 NW / 2 x 64 draws per symbol, none twice."""
    drawn = set()
    for w, l, cc in itertools.product(range(nw), range(64), range(8)):
        rho, h = l >> 4, l & 15
        ant, cls = pair_of(nw, w, rho)
        blk = (ant * (256 * nw) + (cls & ~1) + 32 * nw * (rho & 1) + nw * pw_mtime(h, 0)) // 2 + (nw // 2) * pw_mtime(0, cc)
        assert blk not in drawn
        drawn.add(blk)
    assert drawn == set(range(2 * 256 * nw))                           # 4 antennas x N / 2 blocks


@pytest.mark.parametrize("nw", [2, 4, 8])
def test_every_bin_reaches_the_lane_that_finishes_it(nw):
    uu_n = 16 // nw
    lds = {}
    for w, l, u in itertools.product(range(nw), range(64), range(16)):
        rho, g = l >> 4, l & 15
        ant, cls = pair_of(nw, w, rho)
        pos = w * K_PLANE + rho * 272 + g + 16 * (ant & 1) + 16 * u      # s_mine[wpos + 16 u]
        assert w * K_PLANE <= pos < (w + 1) * K_PLANE                    # a wavefront writes its own plane only
        assert pos not in lds
        lds[pos] = (ant, cls, g + 16 * u)                                # Y_class[k'] of this antenna
    read = set()
    for jw, jj, uu in itertools.product(range(nw), range(nw), range(uu_n)):
        pos = np.empty(64, dtype=np.int64)
        for l in range(64):
            r, g = l >> 4, l & 15
            pos[l] = nw * r * 272 + 16 * (r & 1) + g + 16 * uu_n * jw + jj * 272 + 16 * uu      # s_R[jj kClass + rpos + 16 uu]
            want = (r, jj, g + 16 * (uu_n * jw + uu))                    # er[jj][uu] of lane (r, g): antenna r, class jj, MY k'
            assert lds[int(pos[l])] == want
            assert want not in read
            read.add(want)
        for half in (pos[:32], pos[32:]):                                # ds_read_b64: banks (a / 4) mod 64 per 32-lane half
            banks = np.concatenate([(2 * half) % 64, (2 * half + 1) % 64])
            assert len(set(banks.tolist())) == 64
    assert len(read) == 4 * nw * 256                                     # every element of every partial transform, once
