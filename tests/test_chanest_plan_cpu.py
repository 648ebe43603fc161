"""CPU: the host-side arithmetic of csrc/kernels_chanest.hip replayed in NumPy -- no GPU, no library call:
  * mod_small: x mod n from a float32 reciprocal and a float32 product with two conditional corrections, against Python's exact
    `%` on both sides of every multiple of n up to 2^24 and on every product the kernel forms with a delay of Ne - 1 = 4095;
  * cazac_shape: the lanes-per-tap power of two, the run length of a lane group, the runs tiling [0, Ne) exactly once and the
    tap loop visiting every kept tap exactly once -- and pass 1 as the 64 lanes evaluate it (runs, butterfly, the write by
    group 0) against the direct sum;
  * cazac_lds_plan: wavefronts per workgroup and the table's place for the shapes of tests/test_gpu_chanest_envelope.py.  That
    file imports SHAPES, TAGS and OPERATOR_TAGS from here and asserts the same strings on the device's last_kernel()."""
import numpy as np
import pytest

# name -> (Ne, size multiplier m, K = num_taps_to_keep, users, receive antennas, channel taps)
SHAPES = {
    "A": (37, 2, 36, 1, 1, 1),          # odd prime Ne < 64, K = Ne - 1, one of everything
    "B": (139, 4, 0, 8, 3, 24),         # K = 0: 64 runs of 3 samples, 17 of them empty; 576 draws
    "C": (149, 1, 70, 2, 4, 3),         # 71 taps kept: two trips of the tap loop
    "D": (1024, 2, 15, 8, 4, 24),       # 768 draws, more than 63 KiB of LDS
    "E": (2047, 2, 64, 3, 1, 5),        # odd Ne, 65 taps kept
    "F": (4096, 1, 15, 1, 1, 2),        # table in global memory (complex128); delays [0, 4095]
    "G": (4096, 1, 4095, 1, 1, 1),      # complex128: one realization does not fit the LDS at all
    "H": (1365, 3, 31, 2, 3, 4),        # N = 4095, odd and not a power of two
    "E2": (2047, 2, 64, 2, 1, 5),       # E with two users: the later trips of one wavefront per workgroup
    "D2": (1024, 2, 15, 2, 1, 4),       # D with 2 users x 1 antenna x 4 taps: the later trips of two wavefronts per workgroup
}
# (shape, dtype) -> engine.last_kernel() after mcle_run_chanest; None = refused ("does not fit")
TAGS = {
    ("A", "f64"): "chanest f64 w4", ("A", "f32"): "chanest f32 w4",
    ("B", "f64"): "chanest f64 w4", ("B", "f32"): "chanest f32 w4",
    ("C", "f64"): "chanest f64 w4", ("C", "f32"): "chanest f32 w4",
    ("D", "f64"): "chanest f64 w2", ("D", "f32"): "chanest f32 w4",
    ("E", "f64"): "chanest f64 w1", ("E", "f32"): "chanest f32 w2",
    ("F", "f64"): "chanest f64 w1 gtw", ("F", "f32"): "chanest f32 w1",
    ("G", "f64"): None, ("G", "f32"): "chanest f32 w1",
    ("H", "f64"): "chanest f64 w2", ("H", "f32"): "chanest f32 w4",
    ("E2", "f64"): "chanest f64 w1",
    ("D2", "f64"): "chanest f64 w2",
}
# (Ne, m, K, dtype) -> engine.last_kernel() after mcle_cazac_estimate; the first two need exactly 163 840 bytes
OPERATOR_TAGS = {
    (2048, 1, 2047, "f64"): "cazac_estimate f64 w2",
    (4096, 1, 4095, "f32"): "cazac_estimate f32 w2",
    (4096, 1, 4095, "f64"): "cazac_estimate f64 w1 gtw",
}
LDS_BUDGET = 160 * 1024
CX_BYTES = {"f64": 16, "f32": 8}
TWO24 = 1 << 24


# ---- mod_small ------------------------------------------------------------------------------------------------------------
def mod_small(x, n):
    """kernels_chanest.hip mod_small on an int64 array: float32 reciprocal, float32 product, truncation, two corrections"""
    inv = np.float32(1.0) / np.float32(n)
    q = (x.astype(np.float32) * inv).astype(np.int64)
    r = x - q * n
    r = np.where(r < 0, r + n, r)
    return np.where(r >= n, r - n, r)


MODULI = sorted({m * ne for ne, m, *_ in SHAPES.values()} | {1 << b for b in range(13)} | {4095, 4093, 3})


@pytest.mark.parametrize("n", MODULI)
def test_mod_small_on_both_sides_of_every_multiple(n):
    assert 1 <= n <= 4096
    step = 1 << 21
    for q0 in range(0, TWO24 // n + 1, step):
        mult = np.arange(q0, min(q0 + step, TWO24 // n + 1), dtype=np.int64) * n
        x = np.concatenate([mult - 1, mult, mult + 1])
        x = x[(x >= 0) & (x <= TWO24)]                                         # the function's stated domain
        got = mod_small(x, n)
        bad = np.nonzero(got != x % n)[0]
        assert bad.size == 0, (n, x[bad[:4]].tolist(), got[bad[:4]].tolist())


def test_mod_small_on_the_products_of_a_delay_of_ne_minus_one():
    """Shape F: k * 4095 (pass 2's true response) and m n * 4095 (the received comb) for every k, n < 4096 = N; shapes E and H:
    the same with their N and Ne - 1."""
    for name in ("F", "E", "H", "G"):
        ne, m = SHAPES[name][:2]
        x = np.arange(m * ne, dtype=np.int64) * (ne - 1)
        assert x.max() <= TWO24
        assert np.array_equal(mod_small(x, m * ne), x % (m * ne)), name


# ---- cazac_shape ------------------------------------------------------------------------------------------------------------
def cazac_shape(ne, K):
    n_tap = K + 1
    tp_shift = 0
    while tp_shift < 6 and (1 << tp_shift) < n_tap:
        tp_shift += 1
    parts = 64 >> tp_shift
    return tp_shift, (ne + parts - 1) // parts


def lane_run(lane, ne, tp_shift, chunk):
    part = lane >> tp_shift
    n0 = min(part * chunk, ne)
    return n0, min(n0 + chunk, ne)


SHAPE_CASES = [(ne, n_tap) for ne in (2, 37, 63, 64, 65, 4096) for n_tap in (1, 2, 3, 33, 64, 65, 4096) if n_tap <= ne]
# n_tap -> tp_shift, written out
TP_SHIFT = {1: 0, 2: 1, 3: 2, 33: 6, 64: 6, 65: 6, 4096: 6}


@pytest.mark.parametrize("ne,n_tap", SHAPE_CASES)
def test_cazac_shape_tiles_samples_and_taps_once(ne, n_tap):
    tp_shift, chunk = cazac_shape(ne, n_tap - 1)
    TP, parts = 1 << tp_shift, 64 >> tp_shift
    assert tp_shift == TP_SHIFT[n_tap] and TP * parts == 64
    assert chunk == -(-ne // parts) and chunk >= 1
    # a tap's samples: over the lanes that own tap tl (one per part), every n in [0, ne) exactly once
    for tl in {0, TP - 1}:
        seen = np.zeros(ne, dtype=int)
        for lane in range(64):
            if lane & (TP - 1) == tl:
                n0, n1 = lane_run(lane, ne, tp_shift, chunk)
                assert 0 <= n0 <= n1 <= ne
                seen[n0:n1] += 1
        assert np.all(seen == 1)
    # the tap loop: t = tb + tl for tb = 0, TP, 2 TP .. < n_tap visits every kept tap once, written by part 0 only
    taps = np.zeros(n_tap, dtype=int)
    for tb in range(0, n_tap, TP):
        for lane in range(64):
            t = tb + (lane & (TP - 1))
            if lane >> tp_shift == 0 and t < n_tap:
                taps[t] += 1
    assert np.all(taps == 1)
    assert len(range(0, n_tap, TP)) == (1 if n_tap <= 64 else -(-n_tap // 64))


def test_empty_runs_of_shape_b():
    ne, _, K = SHAPES["B"][:3]
    tp_shift, chunk = cazac_shape(ne, K)
    runs = [lane_run(lane, ne, tp_shift, chunk) for lane in range(64)]
    assert (tp_shift, chunk) == (0, 3)
    assert runs[45] == (135, 138) and runs[46] == (138, 139) and all(r == (139, 139) for r in runs[47:])


@pytest.mark.parametrize("ne,m,K", [(37, 2, 36), (139, 4, 0), (149, 1, 70), (65, 3, 64), (64, 1, 2), (2, 1, 1), (63, 2, 32)])
def test_pass_one_as_the_lanes_evaluate_it(ne, m, K):
    """cazac_taps on 64 simulated lanes -- stepped twiddle index from mod_small, butterfly over the lane groups, the write by
    group 0 -- against h[t] = (1 / Ne) sum_n z[n] exp(+2 pi i n t / Ne)."""
    N, n_tap = m * ne, K + 1
    tp_shift, chunk = cazac_shape(ne, K)
    TP = 1 << tp_shift
    rs = np.random.RandomState(ne + K)
    z = rs.randn(ne) + 1j * rs.randn(ne)
    w = np.exp(-2j * np.pi * np.arange(N) / N)
    h = np.full(n_tap, np.nan, dtype=complex)
    for tb in range(0, n_tap, TP):
        acc = np.zeros(64, dtype=complex)
        for lane in range(64):
            t = tb + (lane & (TP - 1))
            if t < n_tap:
                n0, n1 = lane_run(lane, ne, tp_shift, chunk)
                step = m * t
                idx = int(mod_small(np.array([step * n0], dtype=np.int64), N)[0])
                for n in range(n0, n1):
                    acc[lane] += z[n] * np.conj(w[idx])
                    idx += step
                    if idx >= N:
                        idx -= N
        off = TP
        while off < 64:
            acc = acc + acc[np.arange(64) ^ off]
            off <<= 1
        for lane in range(64):
            t = tb + (lane & (TP - 1))
            if lane >> tp_shift == 0 and t < n_tap:
                assert np.isnan(h[t].real)
                h[t] = acc[lane] / ne
    want = (z[None, :] * np.exp(2j * np.pi * np.outer(np.arange(n_tap), np.arange(ne)) / ne)).sum(1) / ne
    assert np.max(np.abs(h - want)) <= 1e-12 * np.max(np.abs(want))


# ---- cazac_lds_plan ---------------------------------------------------------------------------------------------------------
def cazac_lds_plan(table_bytes, per_wave, fixed):
    """-> (wavefronts per workgroup, table in LDS, bytes) or (0, 0, 0)"""
    for twl in (1, 0):
        for waves in (4, 2, 1):
            need = fixed + (table_bytes if twl else 0) + waves * per_wave
            if need <= LDS_BUDGET:
                return waves, twl, need
    return 0, 0, 0


def _tag(what, dtype, waves, twl):
    return "%s %s w%d%s" % (what, dtype, waves, "" if twl else " gtw") if waves else None


def chanest_plan(shape, dtype):
    ne, m, K, users, rx, taps = shape
    cx = CX_BYTES[dtype]
    return cazac_lds_plan(m * ne * cx, (users * rx * taps + 2 * ne + K + 1) * cx, 512)


def operator_plan(ne, m, K, dtype):
    cx = CX_BYTES[dtype]
    return cazac_lds_plan(m * ne * cx, (ne + K + 1) * cx, 0)


@pytest.mark.parametrize("name,dtype", sorted(TAGS))
def test_pipeline_plan_reproduces_the_tag_table(name, dtype):
    waves, twl, need = chanest_plan(SHAPES[name], dtype)
    assert _tag("chanest", dtype, waves, twl) == TAGS[(name, dtype)]
    assert need <= LDS_BUDGET


def test_every_pipeline_plan_is_in_the_table():
    assert {t.split(" ", 2)[2] for t in TAGS.values() if t} == {"w4", "w2", "w1", "w1 gtw"}
    assert sorted(k for k, t in TAGS.items() if t is None) == [("G", "f64")]
    # the launch raises the dynamic-LDS limit above 63 KiB (the 512 fixed bytes are static): D, E, F, H and the trip shapes do
    for (name, dtype), tag in TAGS.items():
        if tag:
            above = chanest_plan(SHAPES[name], dtype)[2] - 512 > 63 * 1024
            assert above == (SHAPES[name][0] >= 1024), (name, dtype)


@pytest.mark.parametrize("case", sorted(OPERATOR_TAGS))
def test_operator_plan_at_the_exact_budget(case):
    ne, m, K, dtype = case
    waves, twl, need = operator_plan(ne, m, K, dtype)
    assert _tag("cazac_estimate", dtype, waves, twl) == OPERATOR_TAGS[case]
    assert need == (LDS_BUDGET if twl else 131072)
    if twl:          # one more element per wavefront and two of them no longer fit: `need <= budget` is the boundary
        assert cazac_lds_plan(m * ne * CX_BYTES[dtype], (ne + K + 2) * CX_BYTES[dtype], 0)[0] == 1
