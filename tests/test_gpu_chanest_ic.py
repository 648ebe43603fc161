"""GPU: mcle_run_chanest_ic and mcle_cazac_cancel (csrc/kernels_chanest_ic.hip) against the NumPy restatement under common
random numbers (tests/chanest_ic_oracle.py, draw ledger of DESIGN section 4) and the reference's own numbers
(tests/golden/g2_chanest_ic.npz); the staged route, grid and split invariance, the simulator on top, the argument rules.
Shapes, seeds and the restatement's cached realizations are those of tests/test_chanest_ic_cpu.py; the tolerances are the
operator's (tests/test_gpu_chanest_pipeline.py), element-wise relative on err and pow."""
import os

import numpy as np
import pytest

import chanest_ic_oracle as io
import chanest_oracle as co
from helpers import GOLDEN
from pyphysim_amd import reference_signals as rs
from pyphysim_amd.channel_estimation import estimate_with_interference_cancellation
from pyphysim_amd.simulators import ChannelEstimationSimulator
from test_chanest_ic_cpu import COUNT, IC_TAGS, PROFILE, SEED, SHAPES, oracle_run, users_on_roots
from test_gpu_chanest_pipeline import F32_TOL, F64_TOL

pytestmark = pytest.mark.gpu

TOL = {"f64": F64_TOL, "f32": F32_TOL}
MODES = (0, 1, 2)


def run(engine, cfg, gains, direct, mode, first, count, dtype):
    return engine.run_chanest_ic(cfg["ref_seqs"], cfg["n_rx"], cfg["num_taps_to_keep"], cfg["size_multiplier"],
                                 cfg["noise_var"], cfg["tap_power"], cfg["tap_delay"], SEED, first, count, mode,
                                 direct_user=direct, link_gain=gains, dtype=dtype, per_realization=True, return_order=True)


def worst(got, want):
    return float(np.max(np.abs(got - want) / want))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_parity_under_common_random_numbers(engine, name, mode, dtype):
    cfg, gains, direct = SHAPES[name]
    res, err, pw, order = run(engine, cfg, gains, direct, mode, 0, COUNT, dtype)
    assert engine.last_kernel() == "chanest_ic %s w4" % dtype
    want_err, want_pow, want_order, margin = (v.copy() for v in oracle_run(name, mode))
    assert order.dtype == np.int32 and order.shape == want_order.shape
    # err and pow against the restatement evaluated with the order the kernel reported: no realization is left out
    for r in np.flatnonzero((order != want_order).any(axis=1)):
        assert order[r, 0] == direct and sorted(order[r]) == list(range(len(gains))), (r, order[r])
        want_err[r], want_pow[r], _, _ = io.ic_realization(SEED, int(r), cfg, gains, direct, mode, order=order[r].tolist())
    e_err, e_pow = worst(err, want_err), worst(pw, want_pow)
    print(name, mode, dtype, "err %.3g pow %.3g (element-wise relative)" % (e_err, e_pow), "smallest margin %.3g" % margin.min(),
          "nmse", (err.sum(0) / pw.sum(0)).tolist())
    assert e_err <= TOL[dtype] and e_pow <= TOL[dtype]
    decided = margin >= 1e-3          # everywhere on these inputs (test_chanest_ic_cpu.py::test_ordering_condition)
    assert np.array_equal(order[decided], want_order[decided])
    if mode != 2:
        assert np.all(order == np.asarray(io.fixed_order(len(gains), direct, mode)))
    assert np.array_equal(res["err"], np.cumsum(err, axis=0)[-1]) and res["n_realizations"] == COUNT


# The launch plans the two small shapes never reach (tests/test_chanest_ic_cpu.py IC_TAGS): two and one wavefront per workgroup, the
# table read from global memory, and more than 64 KiB of dynamic LDS (every one of these), which takes the attribute call.
PLAN_CASES = [(512, "f64"), (1024, "f64"), (1500, "f64"), (2048, "f32")]
PLAN_GAINS = (0.25, 1.0, 0.5)


@pytest.mark.parametrize("ne,dtype", PLAN_CASES)
def test_every_launch_plan(engine, ne, dtype):
    """Mode 2 at the README's K = 15, 3 users, 4 antennas, 4 realizations, against the restatement evaluated with the order the
    kernel reported.  Bound, as tests/test_gpu_chanest_envelope.py reasons it, with the power P of all users in place of the
    user's own: every estimate is formed from a comb that carries all users, and after a subtraction also the rounding of what
    was subtracted, so it lies within TOL sqrt(P) of the restatement's; that moves the error sum by at most
    2 TOL sqrt(err P) + TOL^2 P.  pow comes from the user's own drawn taps alone: 2 TOL pow."""
    tag = IC_TAGS[(ne, 2, 15, 3, 4, 4, dtype)]
    cfg = dict(ref_seqs=users_on_roots((1, 2, 3), ne), n_rx=4, size_multiplier=2, num_taps_to_keep=15, noise_var=1e-3, **PROFILE)
    count, direct, tol = 4, 1, TOL[dtype]
    _, err, pw, order = run(engine, cfg, PLAN_GAINS, direct, 2, 0, count, dtype)
    assert engine.last_kernel() == tag and tag.split()[2] in ("w1", "w2")
    for r in range(count):
        _, _, own_order, margin = io.ic_realization(SEED, r, cfg, PLAN_GAINS, direct, 2)
        assert margin < 1e-3 or order[r].tolist() == own_order, (r, order[r], own_order, margin)
        assert order[r, 0] == direct and sorted(order[r]) == [0, 1, 2]
        want_err, want_pow, _, _ = io.ic_realization(SEED, r, cfg, PLAN_GAINS, direct, 2, order=order[r].tolist())
        total = want_pow.sum()
        r_err = float(np.max(np.abs(err[r] - want_err) / (2 * tol * np.sqrt(want_err * total) + tol ** 2 * total)))
        r_pow = float(np.max(np.abs(pw[r] - want_pow) / (2 * tol * want_pow)))
        print(tag, "realization", r, "worst ratio to the bound err %.3g pow %.3g" % (r_err, r_pow), "order", order[r].tolist())
        assert r_err <= 1.0 and r_pow <= 1.0, (r, r_err, r_pow)


def test_order_row_is_complete_when_the_norms_do_not_compare(engine):
    """A NaN in one user's sequence reaches every estimate through the comb; a NaN norm counts as infinite, so the tie rule
    (the higher index first) still fills the whole row."""
    cfg, gains, direct = SHAPES["A"]
    seqs = cfg["ref_seqs"].copy()
    seqs[2, 5] = np.nan
    for dtype in ("f64", "f32"):
        _, err, pw, order = run(engine, dict(cfg, ref_seqs=seqs), gains, direct, 2, 0, 4, dtype)
        assert np.all(np.isnan(err)) and order.tolist() == [[0, 2, 1]] * 4


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_mode_0_with_unit_gains_is_run_chanest(engine, name, dtype):
    cfg, gains, direct = SHAPES[name]
    _, err, pw, order = run(engine, cfg, None, direct, 0, 0, COUNT, dtype)
    _, e0, p0 = engine.run_chanest(cfg["ref_seqs"], cfg["n_rx"], cfg["num_taps_to_keep"], cfg["size_multiplier"],
                                   cfg["noise_var"], cfg["tap_power"], cfg["tap_delay"], SEED, 0, COUNT, dtype=dtype,
                                   per_realization=True)
    assert engine.last_kernel().startswith("chanest " + dtype)
    print(name, dtype, "err %.3g pow %.3g" % (worst(err, e0), worst(pw, p0)))
    assert worst(err, e0) <= TOL[dtype] and worst(pw, p0) <= TOL[dtype]
    assert np.all(order == np.arange(len(gains)))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_staged_route_equals_the_reference_rules(engine, dtype):
    """Once per receiver, its own user the direct one; the app keeps 11 taps."""
    gold = np.load(os.path.join(GOLDEN, "g2_chanest_ic.npz"), allow_pickle=False)
    for i in range(3):
        for mode, key in (("direct", "direct"), ("sic", "sic")):
            got = estimate_with_interference_cancellation(gold["ref"], gold["rx"][i], 10, 2, i, mode, engine=engine,
                                                          dtype=dtype)
            want = gold[key][i].transpose(1, 0, 2)                                   # [antennas, users, 48]
            assert got.shape == want.shape == (2, 3, 48)
            e = float(np.max(np.abs(got - want))) / float(np.max(np.abs(want)))
            print(dtype, "receiver", i, key, "%.3g of the largest magnitude" % e)
            assert e <= TOL[dtype]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("mode", MODES)
def test_staged_route_meets_the_fused_tolerances(engine, mode, dtype):
    """Shape A's draws formed on the host, estimated through mcle_cazac_estimate / mcle_cazac_cancel, errors summed on the host."""
    cfg, gains, direct = SHAPES["A"]
    want_err, _, want_order, _ = oracle_run("A", mode)
    H, Y = [], []
    for r in range(COUNT):
        taps, noise = co.chanest_draws(SEED, r, cfg)
        h, y = co.chanest_channels(taps * np.sqrt(np.asarray(gains))[:, None, None], noise, cfg)
        H.append(h), Y.append(y)
    H, Y = np.array(H), np.array(Y)                                                  # [64, 3, 2, 96], [64, 2, 48]
    est = estimate_with_interference_cancellation(cfg["ref_seqs"], Y, 5, 2, direct, mode, engine=engine, dtype=dtype)
    assert est.shape == (COUNT, 2, 3, 96)
    err = (np.abs(est.astype(np.complex128).transpose(0, 2, 1, 3) - H) ** 2).sum((2, 3))
    print(mode, dtype, "staged err %.3g (element-wise relative)" % worst(err, want_err))
    assert worst(err, want_err) <= TOL[dtype]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_cancel_in_place_equals_out_of_place(engine, dtype):
    rng = np.random.RandomState(5)
    cplx = np.complex128 if dtype == "f64" else np.complex64
    ref = SHAPES["B"][0]["ref_seqs"][0]
    rx = (rng.randn(67, 3, 37) + 1j * rng.randn(67, 3, 37)).astype(cplx)
    est = (rng.randn(67, 3, 74) + 1j * rng.randn(67, 3, 74)).astype(cplx)
    want = rx.astype(np.complex128) - est.astype(np.complex128)[..., ::2] * ref
    out = engine.cazac_cancel(ref, rx, est, size_multiplier=2, dtype=dtype)
    assert engine.last_kernel() == "cazac_cancel " + dtype
    assert out.shape == rx.shape and float(np.max(np.abs(out - want))) <= TOL[dtype] * float(np.max(np.abs(want)))
    d_rx, d_est = engine.to_device(rx), engine.to_device(est)
    same = engine.cazac_cancel(ref, d_rx, d_est, size_multiplier=2, dtype=dtype, out=d_rx)
    assert same is d_rx and np.array_equal(d_rx.get(), out)
    assert engine.cazac_cancel(ref, rx[:0], est[:0], dtype=dtype).shape == (0, 3, 37)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_grid_and_split_invariance(engine, dtype):
    """As tests/test_gpu_chanest_pipeline.py does it: grid_oversub = 1 makes every wavefront take three or four trips of the
    grid-stride loop, 8 holds all realizations in one trip, a split run shifts which wavefront gets which realization."""
    cfg, gains, direct = SHAPES["A"]
    per_trip = 2 * engine.n_cu * 4
    count = 3 * per_trip + 37
    with engine.options(grid_oversub=1):
        _, err, pw, order = run(engine, cfg, gains, direct, 2, 0, count, dtype)
    assert engine.last_kernel() == "chanest_ic %s w4" % dtype and np.all(pw > 0) and np.all(err > 0)
    with engine.options(grid_oversub=8):
        _, e8, p8, o8 = run(engine, cfg, gains, direct, 2, 0, count, dtype)
    assert np.array_equal(e8, err) and np.array_equal(p8, pw) and np.array_equal(o8, order)
    cut = per_trip + 3
    with engine.options(grid_oversub=1):
        _, e1, p1, o1 = run(engine, cfg, gains, direct, 2, 0, cut, dtype)
        _, e2, p2, o2 = run(engine, cfg, gains, direct, 2, cut, count - cut, dtype)
    assert np.array_equal(np.concatenate([e1, e2]), err) and np.array_equal(np.concatenate([p1, p2]), pw)
    assert np.array_equal(np.concatenate([o1, o2]), order)
    for r in (0, per_trip - 1, per_trip, 2 * per_trip + 5, count - 1):          # first trip, both sides of a wrap, the tail
        want_err, want_pow, want_order, margin = io.ic_realization(SEED, r, cfg, gains, direct, 2)
        assert margin >= 1e-3 and order[r].tolist() == want_order, r
        assert worst(err[r], want_err) <= TOL[dtype] and worst(pw[r], want_pow) <= TOL[dtype], r


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("mode", MODES)
def test_exact_recovery_without_noise(engine, mode, dtype):
    """Users of one root with shifts (0, 2, 5): no user's taps fall into another's window 0 .. 5, so there is nothing to cancel
    and cancellation must not add error."""
    root = rs.RootSequence(root_index=7, size=48)
    cfg = dict(ref_seqs=np.stack([rs.SrsUeSequence(root, s).seq_array() for s in (0, 2, 5)]), n_rx=2, size_multiplier=2,
               num_taps_to_keep=5, noise_var=0.0, **PROFILE)
    _, err, pw, _ = run(engine, cfg, (1.0, 0.2, 0.03), 0, mode, 0, COUNT, dtype)
    assert err.shape == pw.shape == (COUNT, 3) and np.all(pw > 0)
    print(mode, dtype, "worst err / pow %.3g" % float(np.max(err / pw)))
    assert float(np.max(err / pw)) <= TOL[dtype] ** 2


def test_simulator(engine):
    kw = dict(SNR=[30.0], n_users=3, shifts=(4, 4, 4), root_indexes=(1, 2, 3), Ne=48, size_multiplier=2, num_taps_to_keep=5, Nr=2,
              rep_max=48, seed=3, batch_size=64, dtype="f64", engine=engine, common_random_numbers=True)
    gains = (1.0, 0.2, 0.03)
    nmse = {}
    for rule in ("none", "direct", "sic"):
        sim = ChannelEstimationSimulator(interference_cancellation=rule, pathloss=gains, **kw)
        sim.simulate()
        assert engine.last_kernel() == "chanest_ic f64 w4"
        assert np.array_equal(sim.ref_seqs, SHAPES["A"][0]["ref_seqs"])
        res = engine.run_chanest_ic(sim.ref_seqs, 2, 5, 2, 1e-3, sim._tap_power, sim._tap_delay, 3, 0, 48, rule, link_gain=gains,
                                    dtype="f64")
        nmse[rule] = [sim.results.get_result_values_list("nmse_user%d" % u)[0] for u in range(3)]
        assert nmse[rule] == [res["err"][u] / res["pow"][u] for u in range(3)], rule
    print(nmse)
    assert nmse["none"][2] > nmse["direct"][2] > nmse["sic"][2] > 0
    assert nmse["none"][0] == nmse["direct"][0] == nmse["sic"][0]
    # the defaults: the plain pipeline, as before
    plain = ChannelEstimationSimulator(**kw)
    plain.simulate()
    assert engine.last_kernel() == "chanest f64 w4"
    res = engine.run_chanest(plain.ref_seqs, 2, 5, 2, 1e-3, plain._tap_power, plain._tap_delay, 3, 0, 48, dtype="f64")
    for u in range(3):
        assert plain.results.get_result_values_list("nmse_user%d" % u)[0] == res["err"][u] / res["pow"][u]
    with pytest.raises(ValueError, match="interference_cancellation"):
        ChannelEstimationSimulator(interference_cancellation="all", **kw)
    with pytest.raises(ValueError, match="pathloss"):
        ChannelEstimationSimulator(pathloss=(1.0, 0.5), **kw)


def test_argument_rules(engine):
    cfg, gains, direct = SHAPES["A"]
    with pytest.raises(ValueError, match="mode"):
        run(engine, cfg, gains, direct, 3, 0, 4, "f64")
    with pytest.raises(ValueError, match="direct_user"):
        run(engine, cfg, gains, 3, 1, 0, 4, "f64")
    with pytest.raises(ValueError, match="direct_user"):
        run(engine, cfg, gains, -1, 1, 0, 4, "f32")
    with pytest.raises(ValueError, match="link gains"):
        run(engine, cfg, (1.0, 0.0, 0.03), direct, 2, 0, 4, "f64")
    with pytest.raises(ValueError, match="link gains"):
        run(engine, cfg, (1.0, 0.2, float("nan")), direct, 2, 0, 4, "f64")
    with pytest.raises(ValueError, match="n_rx"):                                  # a rule of mcle_run_chanest
        run(engine, dict(cfg, n_rx=5), gains, direct, 2, 0, 4, "f64")
    assert engine.last_kernel() == ""
    big = dict(cfg, ref_seqs=np.ones((3, 2048), dtype=complex), num_taps_to_keep=15, n_rx=4)
    with pytest.raises(ValueError, match="does not fit"):
        run(engine, big, gains, direct, 2, 0, 4, "f64")
    assert engine.last_kernel() == ""
    with pytest.raises(ValueError, match="4096"):
        engine.cazac_cancel(np.ones(2049), np.ones((1, 2049)), np.ones((1, 4098)), size_multiplier=2)
    res, err, pw, order = run(engine, cfg, gains, direct, 2, 0, 0, "f64")
    assert err.shape == pw.shape == order.shape == (0, 3) and res["n_realizations"] == 0 and engine.last_kernel() == ""
