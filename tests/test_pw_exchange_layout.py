"""CPU: the index arithmetic of the part-wave kernel's exchange in complex halves (csrc/pipeline_mimo_pw.hip, template parameter
XCH), replayed in NumPy for NW = 2, 4 and 8 wavefronts per realization.

The exchange hands the partial spectra of the 4 NW (antenna, time class) pairs from the lane rows that computed them (wavefront w,
row rho: pair f = 4 w + rho = NW antenna + class, sixteen elements k' = g + 16 u per lane) to the lanes that finish the last
radix-NW stage (wavefront jw, row r = antenna: class jj at k' = g + 16 (UU jw + uu), UU = 16 / NW).  The values go as complex
numbers, 16 bytes each, in two halves by uu: phase A carries uu < UU / 2 of every reader and phase B the rest, INTO THE SLOTS THE
SAME LANE HAS JUST READ -- which is why no workgroup barrier stands between the phase-A loads and the phase-B stores.  The
functions below are the kernel's address expressions (in doubles from the base of the planes, lane base + compile-time offset);
the tests derive what they must deliver from the ownership maps alone.

Checked: phase-A stores hit pairwise distinct, 16-byte aligned slots inside the planes; every phase-A slot is loaded by exactly one
(wavefront, lane) and that lane's phase-B stores go to exactly the slots it loaded; after both phases every reader holds what the
old exchange (re planes, then im planes, + 16 doubles for an odd antenna) delivers; the 16-byte loads and stores of both phases
are free of bank conflicts under the lane groups and bank functions of the LDS (ds_read_b128: four groups of sixteen lanes
{0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32, banks (a / 4) mod 64; ds_write_b128: eight groups of eight
consecutive lanes, banks (a / 4) mod 32) -- and with the old shift of the odd antennas kept the same count is NOT zero."""
import numpy as np
import pytest

SLICE = 272                      # doubles per (antenna, class) slice; kPwPlane = 4 slices per wavefront plane
PLANE = 4 * SLICE
NWS = [2, 4, 8]
READ_GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
               [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
READ_GROUPS = READ_GROUPS + [[l + 32 for l in grp] for grp in READ_GROUPS]
WRITE_GROUPS = [list(range(8 * i, 8 * i + 8)) for i in range(8)]


# ---- the kernel's address expressions, in doubles (a complex value = two doubles = one 16-byte slot) ----
def a_store(NW, w, rho, g, u, shift=False):
    """phase A, writer lane (rho, g) of wavefront w: register u = UU jw + uu, uu < UU / 2"""
    UU = 16 // NW
    jw, uu = divmod(u, UU)
    assert uu < UU // 2
    base = (4 * w + rho) * SLICE + 2 * g + (16 * (((4 * w + rho) // NW) & 1) if shift else 0)
    return base + 32 * ((UU // 2) * jw + uu)


def a_base(NW, jw, r, g, shift=False):
    UU = 16 // NW
    return NW * r * SLICE + 2 * (g + 16 * (UU // 2) * jw) + (16 * (r & 1) if shift else 0)


def a_load(NW, jw, r, g, jj, uu, shift=False):
    """phase A, reader lane (r, g) of wavefront jw: class jj, uu < UU / 2"""
    return a_base(NW, jw, r, g, shift) + jj * SLICE + 32 * uu


def b_store(NW, w, rho, g, u):
    """phase B, the same lane as a writer again: register u = UU jw' + uu', uu' >= UU / 2, goes to the slot read for (jj = jw', uu' - UU / 2)"""
    UU = 16 // NW
    jw2, uu2 = divmod(u, UU)
    assert uu2 >= UU // 2
    return a_base(NW, w, rho, g) + jw2 * SLICE + 32 * (uu2 - UU // 2)


def b_load(NW, jw, r, g, jj, uu):
    """phase B, reader lane (r, g) of wavefront jw: class jj, uu >= UU / 2"""
    UU = 16 // NW
    if NW == 2:
        base = (4 * (r & 1) + jw) * SLICE + 2 * g + 128 * (r >> 1)
        off = 2 * jj * SLICE
    else:
        base = jw * SLICE + 2 * g + 64 * r
        off = (jj & 3) * NW * SLICE + 32 * (UU // 2) * (jj >> 2)
    return base + off + 32 * (uu - UU // 2)


# ---- the ownership maps ----
def pair_of(NW, w, rho):
    f = 4 * w + rho
    return f // NW, f % NW                       # (antenna, class)


def value(ant, cls, k):
    return complex(1 + ant + 4 * cls + 64 * k, -(7 + k + 256 * ant + 1024 * cls))


def lanes():
    return [(l >> 4, l & 15) for l in range(64)]


def old_exchange(NW):
    """re planes, barrier, er; im planes, barrier, ei: the addresses of the exchange this one replaces (XCH = false)"""
    UU = 16 // NW
    lds = np.full(NW * PLANE, np.nan)
    got = {}
    for part in (0, 1):
        for w in range(NW):
            for rho, g in lanes():
                ant, cls = pair_of(NW, w, rho)
                wpos = w * PLANE + rho * SLICE + g + 16 * (((4 * w + rho) // NW) & 1)
                for u in range(16):
                    z = value(ant, cls, g + 16 * u)
                    lds[wpos + 16 * u] = z.imag if part else z.real
        for jw in range(NW):
            for r, g in lanes():
                rpos = NW * r * SLICE + 16 * (r & 1) + g + 16 * UU * jw
                for jj in range(NW):
                    for uu in range(UU):
                        got[(jw, r, g, jj, uu, part)] = lds[jj * SLICE + rpos + 16 * uu]
    return {k[:5]: complex(got[k[:5] + (0,)], got[k[:5] + (1,)]) for k in got if k[5] == 0}


@pytest.mark.parametrize("NW", NWS)
def test_phase_a_stores_are_distinct_aligned_and_inside_the_planes(NW):
    UU = 16 // NW
    slots = [a_store(NW, w, rho, g, UU * jw + uu) for w in range(NW) for rho, g in lanes() for jw in range(NW) for uu in range(UU // 2)]
    assert len(slots) == NW * 64 * 8 and len(set(slots)) == len(slots)
    assert all(s % 2 == 0 and 0 <= s and s + 2 <= NW * PLANE for s in slots)
    # a slice keeps its 128 values of a phase inside its own 272 doubles
    for w in range(NW):
        for rho, g in lanes():
            for jw in range(NW):
                for uu in range(UU // 2):
                    s = a_store(NW, w, rho, g, UU * jw + uu) - (4 * w + rho) * SLICE
                    assert 0 <= s and s + 2 <= 256


@pytest.mark.parametrize("NW", NWS)
def test_every_slot_has_one_reader_who_refills_exactly_its_own_slots(NW):
    UU = 16 // NW
    stored = {a_store(NW, w, rho, g, UU * jw + uu) for w in range(NW) for rho, g in lanes() for jw in range(NW) for uu in range(UU // 2)}
    owner = {}
    for jw in range(NW):
        for r, g in lanes():
            mine = [a_load(NW, jw, r, g, jj, uu) for jj in range(NW) for uu in range(UU // 2)]
            assert len(set(mine)) == 8
            for s in mine:
                assert s not in owner, (s, owner[s], (jw, r, g))
                owner[s] = (jw, r, g)
            refill = [b_store(NW, jw, r, g, UU * jw2 + uu2) for jw2 in range(NW) for uu2 in range(UU // 2, UU)]
            assert sorted(refill) == sorted(mine)
    assert set(owner) == stored


@pytest.mark.parametrize("NW", NWS)
def test_both_phases_deliver_what_the_old_exchange_delivers(NW):
    UU = 16 // NW
    lds = np.full(NW * PLANE // 2, np.nan + 0j)                      # one entry per 16-byte slot
    got = {}
    for w in range(NW):                                              # phase A stores, then the barrier
        for rho, g in lanes():
            ant, cls = pair_of(NW, w, rho)
            for jw in range(NW):
                for uu in range(UU // 2):
                    u = UU * jw + uu
                    lds[a_store(NW, w, rho, g, u) // 2] = value(ant, cls, g + 16 * u)
    after_a = lds.copy()
    # phase A loads and phase B stores, wavefront after wavefront in ANY order (no barrier): every lane loads its eight slots, then refills them
    for jw in reversed(range(NW)):
        for r, g in lanes():
            for jj in range(NW):
                for uu in range(UU // 2):
                    s = a_load(NW, jw, r, g, jj, uu) // 2
                    assert lds[s] == after_a[s]                      # nobody else has written the slot yet
                    got[(jw, r, g, jj, uu)] = lds[s]
            ant, cls = pair_of(NW, jw, r)
            for jw2 in range(NW):
                for uu2 in range(UU // 2, UU):
                    u = UU * jw2 + uu2
                    lds[b_store(NW, jw, r, g, u) // 2] = value(ant, cls, g + 16 * u)
    for jw in range(NW):                                             # the barrier, then the phase B loads
        for r, g in lanes():
            for jj in range(NW):
                for uu in range(UU // 2, UU):
                    got[(jw, r, g, jj, uu)] = lds[b_load(NW, jw, r, g, jj, uu) // 2]
    want = old_exchange(NW)
    assert set(got) == set(want) and len(got) == NW * 64 * 16
    for key, z in got.items():
        jw, r, g, jj, uu = key
        assert z == value(r, jj, g + 16 * (UU * jw + uu)), key        # (antenna r, class jj, k' = g + 16 (UU jw + uu))
        assert z == want[key], key


# ---- bank conflicts: extra passes of one wave-instruction = per lane group, (distinct dwords on the busiest bank) - 1 ----
def conflicts(addr_doubles, groups, banks):
    extra = 0
    for grp in groups:
        on_bank = {}
        for l in grp:
            for d in range(4):                                        # a 16-byte access covers four dwords
                dword = 2 * addr_doubles[l] + d
                on_bank.setdefault(dword % banks, set()).add(dword)   # identical addresses broadcast
        extra += max(len(v) for v in on_bank.values()) - 1
    return extra


def exchange_conflicts(NW, shift):
    """(phase-A stores, phase-A loads, phase-B stores, phase-B loads): extra passes summed over every instruction of every wavefront"""
    UU = 16 // NW
    a_st = a_ld = b_st = b_ld = 0
    for w in range(NW):
        for jw in range(NW):
            for uu in range(UU // 2):
                a_st += conflicts([a_store(NW, w, rho, g, UU * jw + uu, shift) for rho, g in lanes()], WRITE_GROUPS, 32)
                b_st += conflicts([b_store(NW, w, rho, g, UU * jw + uu + UU // 2) for rho, g in lanes()], WRITE_GROUPS, 32)
        for jj in range(NW):
            for uu in range(UU // 2):
                a_ld += conflicts([a_load(NW, w, r, g, jj, uu, shift) for r, g in lanes()], READ_GROUPS, 64)
                b_ld += conflicts([b_load(NW, w, r, g, jj, uu + UU // 2) for r, g in lanes()], READ_GROUPS, 64)
    return a_st, a_ld, b_st, b_ld


@pytest.mark.parametrize("NW", NWS)
def test_no_bank_conflicts_in_either_phase(NW):
    assert exchange_conflicts(NW, shift=False) == (0, 0, 0, 0)


@pytest.mark.parametrize("NW", NWS)
def test_the_old_shift_of_odd_antennas_would_conflict(NW):
    """the + 16 doubles that keep the 8-byte re / im reads of two rows apart put the 16-byte reads of rows r, r + 1 on the same
    banks: the count above can fail"""
    a_st, a_ld, _, _ = exchange_conflicts(NW, shift=True)
    assert a_st == 0 and a_ld > 0


def test_the_conflict_count_sees_a_two_way_conflict():
    same_bank = [32 * l for l in range(64)]                           # every lane 256 bytes from the next: one bank quadruple
    assert conflicts(same_bank, READ_GROUPS, 64) == 4 * 15 and conflicts(same_bank, WRITE_GROUPS, 32) == 8 * 7
    assert conflicts([2 * l for l in range(64)], READ_GROUPS, 64) == 0
