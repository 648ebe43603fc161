"""CPU: the restatement of the interference-cancellation rules (tests/chanest_ic_oracle.py) against the reference's own
numbers (tests/golden/g2_chanest_ic.npz, written by scripts/make_golden_chanest_ic.py), its properties on the two shapes
the GPU tests use (tests/test_gpu_chanest_ic.py), the launch plan of mcle_run_chanest_ic replayed on the host, and what
the two new entry points refuse without a device.  mcle_ctx_create needs a device, so beyond the NULL-context refusals the
argument rules are driven through the stand-alone host program scripts/asan/chanest_argcheck.cpp, which keeps a context of its
own on the host: built here against the library as it stands and run once (`make -C pyphysim_amd/csrc asan-argcheck` builds the
same program from source under a host sanitizer); on the device, tests/test_gpu_chanest_ic.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import chanest_ic_oracle as io
import chanest_oracle as co
from helpers import GOLDEN
from pyphysim_amd import _lib
from pyphysim_amd import reference_signals as rs
from test_chanest_plan_cpu import CX_BYTES, LDS_BUDGET, _tag, cazac_lds_plan

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, COUNT = 7, 64
PROFILE = dict(tap_power=list(10.0 ** (np.array([0.0, -3.0, -6.0, -9.0]) / 10.0)), tap_delay=[0, 1, 2, 4])


def users_on_roots(roots, ne, shift=4):
    return np.stack([rs.SrsUeSequence(rs.RootSequence(root_index=u, size=ne), shift).seq_array() for u in roots])


# name -> (cfg of chanest_oracle, gains, direct user)
SHAPES = {
    "A": (dict(ref_seqs=users_on_roots((1, 2, 3), 48), n_rx=2, size_multiplier=2, num_taps_to_keep=5, noise_var=1e-3, **PROFILE),
          (1.0, 0.2, 0.03), 0),
    "B": (dict(ref_seqs=users_on_roots((1, 2, 3, 5), 37), n_rx=3, size_multiplier=2, num_taps_to_keep=7, noise_var=1e-3,
               **PROFILE), (0.5, 1.0, 0.1, 0.02), 1),
}
_cache = {}


def oracle_run(name, mode):
    """(err [64, n_users], pow, orders, margins) of realizations 0 .. 63 of seed 7, computed once per (shape, mode)."""
    if (name, mode) not in _cache:
        cfg, gains, direct = SHAPES[name]
        rows = [io.ic_realization(SEED, r, cfg, gains, direct, mode) for r in range(COUNT)]
        _cache[(name, mode)] = (np.array([x[0] for x in rows]), np.array([x[1] for x in rows]),
                                np.array([x[2] for x in rows]), np.array([x[3] for x in rows]))
    return _cache[(name, mode)]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "g2_chanest_ic.npz"), allow_pickle=False)


def test_restatement_equals_the_reference_rules(gold):
    """Once per receiver, that receiver's own user the direct one; the app keeps 11 taps."""
    for i in range(3):
        for mode, name in ((1, "direct"), (2, "sic")):
            est, order, _ = io.ic_estimates(gold["ref"], gold["rx"][i], 10, 2, i, mode)
            assert est.shape == gold[name][i].shape == (3, 2, 48)
            assert float(np.max(np.abs(est - gold[name][i]))) <= 1e-12, (i, name)
            assert order[0] == i and sorted(order) == [0, 1, 2]
    assert float(np.max(np.abs(gold["sic"] - gold["direct"]))) > 1e-3          # the second rule does change an estimate


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_mode_0_with_unit_gains_is_the_plain_restatement(name):
    cfg, gains, direct = SHAPES[name]
    for r in range(4):
        err, pw, order, margin = io.ic_realization(SEED, r, cfg, np.ones(len(gains)), direct, 0)
        want_err, want_pow = co.chanest_realization(SEED, r, cfg)
        assert np.array_equal(err, want_err) and np.array_equal(pw, want_pow)
        assert order == list(range(len(gains))) and margin == np.inf


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_parseval_norm_from_the_taps(name):
    """||H^||^2 over all N bins = N sum |h|^2: what lets the kernel order the users from the kept taps alone."""
    cfg, gains, direct = SHAPES[name]
    seqs, K, m = cfg["ref_seqs"], cfg["num_taps_to_keep"], cfg["size_multiplier"]
    ne = seqs.shape[1]
    taps, noise = co.chanest_draws(SEED, 3, cfg)
    _, Y = co.chanest_channels(taps * np.sqrt(np.asarray(gains))[:, None, None], noise, cfg)
    for u in range(len(gains)):
        h = np.fft.ifft(np.conj(seqs[u]) * Y, ne, axis=-1)[..., :K + 1]
        full = np.linalg.norm(co.estimate(seqs[u], Y, K, m)) ** 2
        assert abs(full - m * ne * (np.abs(h) ** 2).sum()) <= 1e-12 * full


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_ordering_condition(name):
    """The GPU test compares the kernel's order with the restatement's wherever the margin is >= 1e-3; at most 5 % of the
    realizations may fall under it (measured: none -- the minimum is 0.36 on A, 2.0e-3 on B)."""
    _, _, orders, margins = oracle_run(name, 2)
    direct = SHAPES[name][2]
    print(name, "smallest margin %.3g" % margins.min())
    assert np.count_nonzero(margins < 1e-3) <= 0.05 * COUNT
    assert np.all(orders[:, 0] == direct) and np.all(np.sort(orders, axis=1) == np.arange(orders.shape[1]))
    assert len({tuple(o) for o in orders.tolist()}) > 1 or name == "A"          # B's three members do change places


def test_forced_order_and_the_tie_rule():
    cfg, gains, direct = SHAPES["B"]
    err, pw, order, margin = io.ic_realization(SEED, 0, cfg, gains, direct, 2)
    again = io.ic_realization(SEED, 0, cfg, gains, direct, 2, order=order)
    assert np.array_equal(again[0], err) and again[2] == order and again[3] == margin
    other = [order[0]] + order[:0:-1]
    forced = io.ic_realization(SEED, 0, cfg, gains, direct, 2, order=other)
    assert forced[2] == other and not np.array_equal(forced[0], err) and np.array_equal(forced[1], pw)
    # two interferers with the same estimate: the higher index counts as stronger (the app's `>`)
    seqs = np.stack([cfg["ref_seqs"][0], cfg["ref_seqs"][1], cfg["ref_seqs"][1]])
    Y = np.ones((2, 37)) * cfg["ref_seqs"][0]
    _, order, margin = io.ic_estimates(seqs, Y, 7, 2, 0, 2)
    assert order == [0, 2, 1] and margin == 0.0


def test_cancellation_helps_the_weak_users_on_shape_a():
    nmse = []
    for mode in (0, 1, 2):
        err, pw, _, _ = oracle_run("A", mode)
        nmse.append(err.sum(0) / pw.sum(0))
    nmse = np.array(nmse)
    print("NMSE per user, modes 0 / 1 / 2:", nmse.tolist())
    assert nmse[0, 0] == nmse[1, 0] == nmse[2, 0]
    for u in (1, 2):
        assert nmse[2, u] <= nmse[1, u] <= nmse[0, u]
    assert nmse[2, 2] < 0.1 * nmse[0, 2]


# ---- the launch plan of mcle_run_chanest_ic (csrc/kernels_chanest_ic.hip run_chanest_ic_impl) -------------------------------
def ic_plan(ne, m, K, users, rx, taps, dtype):
    """Per wavefront: the drawn taps, the comb of every antenna, z, and the kept taps of every (user, antenna) link."""
    cx = CX_BYTES[dtype]
    return cazac_lds_plan(m * ne * cx, (users * rx * taps + (rx + 1) * ne + users * rx * (K + 1)) * cx, 512)


# (Ne, m, K, users, antennas, taps, dtype) -> engine.last_kernel() after mcle_run_chanest_ic; None = refused ("does not fit")
IC_TAGS = {
    (48, 2, 5, 3, 2, 4, "f64"): "chanest_ic f64 w4", (48, 2, 5, 3, 2, 4, "f32"): "chanest_ic f32 w4",          # A
    (37, 2, 7, 4, 3, 4, "f64"): "chanest_ic f64 w4", (37, 2, 7, 4, 3, 4, "f32"): "chanest_ic f32 w4",          # B
    (150, 2, 15, 3, 4, 4, "f64"): "chanest_ic f64 w4",                                                         # the README's shape
    (512, 2, 15, 3, 4, 4, "f64"): "chanest_ic f64 w2", (1024, 2, 15, 3, 4, 4, "f64"): "chanest_ic f64 w1",
    (1500, 2, 15, 3, 4, 4, "f64"): "chanest_ic f64 w1 gtw",
    (2048, 2, 15, 3, 4, 4, "f64"): None, (2048, 2, 15, 3, 4, 4, "f32"): "chanest_ic f32 w1",      # five combs of 2048: 160 KiB
    (2048, 2, 2047, 8, 4, 4, "f64"): None, (2048, 2, 2047, 8, 4, 4, "f32"): None,                              # 1 MiB of kept taps
}


@pytest.mark.parametrize("case", sorted(IC_TAGS, key=str))
def test_launch_plan_tags(case):
    waves, twl, need = ic_plan(*case)
    assert _tag("chanest_ic", case[-1], waves, twl) == IC_TAGS[case]
    assert need <= LDS_BUDGET


# ---- what needs no device ---------------------------------------------------------------------------------------------------
def test_struct_layout_and_null_context():
    assert ctypes.sizeof(_lib.ChanestIcCfg) == ctypes.sizeof(_lib.ChanestCfg) + 8 + 8 * 8
    assert _lib.ChanestIcCfg.mode.offset == ctypes.sizeof(_lib.ChanestCfg)
    lib = _lib.load()
    cfg = _lib.ChanestIcCfg()
    assert lib.mcle_run_chanest_ic(None, _lib.MCLE_F64, ctypes.byref(cfg), 1, 0, 4, None, None, None) == -1
    assert b"null argument" in lib.mcle_last_error()
    assert lib.mcle_cazac_cancel(None, _lib.MCLE_F64, None, 48, None, None, 1, 2, None) == -1
    assert b"null context" in lib.mcle_last_error()


def test_argument_rules_in_the_stand_alone_checker(tmp_path):
    """Every argument rule of the four channel-estimation entry points, the new two among them, on a context that lives on the
    host: the checker's host code alone is compiled (a few seconds), linked against the built library and run."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "chanest_argcheck")
    lib_dir, lib_name = os.path.split(_lib.LIB_PATH)
    subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-host-only", "-x", "hip",
                    os.path.join(REPO, "scripts", "asan", "chanest_argcheck.cpp"), "-o", exe, "-L", lib_dir, "-l:" + lib_name,
                    "-Wl,-rpath," + lib_dir], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "chanest argument checks: 0 failure(s)" in out.stdout


def test_staged_route_refuses_bad_arguments_before_any_launch():
    from pyphysim_amd.channel_estimation import estimate_with_interference_cancellation as staged
    seqs = SHAPES["A"][0]["ref_seqs"]
    rx = np.zeros((2, 48), dtype=complex)
    boom = object()          # an engine that must not be touched
    with pytest.raises(ValueError, match="mode"):
        staged(seqs, rx, 5, 2, 0, 3, engine=boom)
    with pytest.raises(ValueError, match="direct_user"):
        staged(seqs, rx, 5, 2, 3, "sic", engine=boom)
    with pytest.raises(ValueError, match="rx must be"):
        staged(seqs, np.zeros((2, 47), dtype=complex), 5, 2, 0, "sic", engine=boom)
    with pytest.raises(ValueError, match="rx must be"):
        staged(seqs, np.zeros(48, dtype=complex), 5, 2, 0, "direct", engine=boom)
