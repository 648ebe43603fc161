"""GPU: the fused CoMP link with an external interferer (csrc/pipeline_comp.hip, mcle_run_comp / Engine.run_comp /
simulators.CompSimulator).

Staged equality: the channels are built from the draw ledger on the host (tests/comp_oracle.py) and solved with the
EXISTING operator Engine.bd_extint -- singular-vector phases are the kernel's own, so the comparison goes through the
operator (the rule tests/test_gpu_bd_extint.py states) -- then comp_oracle's link runs on those precoders and filters, and
the stream counts and the per-stream symbol and bit counts of every realization must be equal.

Gap rule ('capacity' and 'effective_throughput' only): a realization in which some user's two best candidate values differ
by at most 1e-9 |best| + 1e-12 is left out of the comparison; at most 5 % of the realizations may be (a condition, asserted;
tests/test_comp_cpu.py shows with the oracle alone that the inputs meet it)."""
import functools
import math

import numpy as np
import pytest

import comp_oracle as co

pytestmark = pytest.mark.gpu

PLB = 10 ** -12.81
NOISE_VAR = 10.0 ** (-116.4 / 10.0) / 1000.0
SEED, FIRST, COUNT = 7, 37, 150                 # three 64-lane chunks, the last ragged
NS, PACKET = 50, 60
SHAPES = [(3, 2, 1), (2, 2, 1), (2, 3, 2), (4, 2, 1), (2, 4, 3), (1, 2, 1)]
SNR_DB, PE_DBM = 5.0, 10.0                      # about half the realizations reduce a stream under 'effective_throughput'


def scenario(K, E, snr_db=SNR_DB, pe_dbm=PE_DBM):
    pl = PLB * (2.0 * np.ones((K, K)) + 6.0 * np.eye(K))
    ple = 1.5 * PLB * np.ones((K, E))
    iPu = 10.0 ** (snr_db / 10.0) * NOISE_VAR / PLB
    pe = 10.0 ** (pe_dbm / 10.0) / 1000.0
    return pl, ple, iPu, pe


@functools.lru_cache(maxsize=None)
def channels(K, r, E):
    pl, ple, _, _ = scenario(K, E)
    H = np.stack([co.draw_big_H(SEED, FIRST + i, K, r, E, pl, ple) for i in range(COUNT)])
    H.setflags(write=False)
    return H


def bind(engine, mod, M):
    from pyphysim_amd import modulators
    m = {"psk": lambda: modulators.PSK(M, engine=engine), "qam": lambda: modulators.QAM(M, engine=engine),
         "bpsk": lambda: modulators.BPSK(engine=engine)}[mod]()
    m._bind()
    return m


def run(engine, K, r, E, variant, dtype="f64", ns=NS, first=FIRST, count=COUNT, method=0, **kw):
    pl, ple, iPu, pe = scenario(K, E)
    args = dict(pathloss=pl, pathloss_ext=ple if E else None, packet_length=PACKET, num_streams=1, method=method, dtype=dtype,
                per_realization=True)
    iPu, noise_var, pe = kw.pop("iPu", iPu), kw.pop("noise_var", NOISE_VAR), kw.pop("pe", pe)
    args.update(kw)
    return engine.run_comp(K, r, E, ns, iPu, noise_var, pe, SEED, first, count, variant=variant, **args)


def operator_solution(engine, modulator, H, K, r, E, variant, iPu, pe):
    """(Ms [b, K, n, r], W [b, K, r, r], Ns [b, K], left_out [b]) from the existing operator."""
    b = H.shape[0]
    left_out = np.zeros(b, dtype=bool)
    if variant == "Whitening":
        sol = engine.bd_extint(H, K, r, E, iPu, NOISE_VAR, pe, "whitening")
    elif variant in ("None", "naive", "fixed"):
        sol = engine.bd_extint(H, K, r, E, iPu, NOISE_VAR, pe, "enhanced", None if variant == "None" else variant, num_streams=1)
    else:
        cand = engine.bd_extint(H, K, r, E, iPu, NOISE_VAR, pe, "enhanced", "candidates")["cand_sinr"]
        if variant == "capacity":
            values = np.array([co.candidate_values(c, "capacity", None, None, None) for c in cand])
            sol = engine.bd_extint(H, K, r, E, iPu, NOISE_VAR, pe, "enhanced", "capacity")
        else:
            # the host argmax of EnhancedBD.block_diagonalize_no_waterfilling with the modulator's own closed form
            values = np.array([[[float(np.sum(modulator.calcTheoreticalSpectralEfficiency(10.0 * np.log10(c[k, n - 1, :n]), PACKET)))
                                 for n in range(1, r + 1)] for k in range(K)] for c in cand])
            ns_all = np.argmax(values, axis=2) + 1
            sol = dict(Ms=np.zeros((b, K, K * r, r), complex), W=np.zeros((b, K, r, r), complex), Ns=ns_all.astype(np.int32))
            for tup in sorted(set(map(tuple, ns_all.tolist()))):
                idx = np.flatnonzero(np.all(ns_all == np.array(tup), axis=1))
                part = engine.bd_extint(H[idx], K, r, E, iPu, NOISE_VAR, pe, "enhanced", "per_user", ns_user=list(tup))
                sol["Ms"][idx], sol["W"][idx] = part["Ms"], part["W"]
                assert np.array_equal(part["Ns"], ns_all[idx])
        left_out = np.array([co.near_tie(v) for v in values])
    return sol["Ms"], sol["W"], np.asarray(sol["Ns"]), left_out


def staged_check(engine, K, r, E, variant, mod="psk", M=4, ns=NS, slicer=False):
    modulator = bind(engine, mod, M)
    table = co.table_for(mod, M)
    pl, ple, iPu, pe = scenario(K, E)
    H = channels(K, r, E)
    Ms, W, Ns, left_out = operator_solution(engine, modulator, H, K, r, E, variant, iPu, pe)
    assert left_out.sum() <= 0.05 * COUNT, "gap rule: %d of %d realizations left out" % (left_out.sum(), COUNT)
    res, got = run(engine, K, r, E, variant, ns=ns, method=1 if slicer else 0)
    n = K * r
    assert res["n_realizations"] == COUNT and res["n_skipped"] == 0
    assert res["n_symbols"] == n * ns and res["n_bits"] == n * ns * co.omodem.level2bits(M)
    assert res["sym_errors"] == int(got["sym_err"].sum()) and res["bit_errors"] == int(got["bit_err"].sum())
    assert res["sym_errors_sq"] == int((got["sym_err"].astype(np.int64) ** 2).sum())
    assert np.array_equal(got["sym_err"], got["stream_sym_err"].sum(axis=1))
    assert np.array_equal(got["bit_err"], got["stream_bit_err"].sum(axis=1))
    reduced = 0
    for i in range(COUNT):
        if left_out[i]:
            continue
        nsi = [int(v) for v in Ns[i]]
        assert [int(v) for v in got["ns"][i]] == nsi, (i, variant)
        reduced += any(v < r for v in nsi)
        MsPk = [Ms[i, k][:, :nsi[k]] for k in range(K)]
        Wk = [W[i, k][:nsi[k], :] for k in range(K)]
        data, ext, noise = co.draw_link_inputs(SEED, FIRST + i, K, r, E, nsi, ns, M, NOISE_VAR, pe)
        out = co.link(H[i], MsPk, Wk, data, ext, noise, table, slicer_M=M if slicer else None)
        assert np.array_equal(got["stream_sym_err"][i], co.to_slots(out["sym_err"], nsi, r)), (i, variant)
        assert np.array_equal(got["stream_bit_err"][i], co.to_slots(out["bit_err"], nsi, r)), (i, variant)
        want = co.to_slots(np.concatenate(co.jp_sinr(H[i], K, r, MsPk, Wk, NOISE_VAR, pe=1.0)), nsi, r)
        assert np.all(np.abs(got["sinr"][i] - want) <= 1e-9 * np.abs(want)), (i, variant)
    return got, reduced


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "K%dr%de%d" % s)
@pytest.mark.parametrize("variant", co.VARIANTS)
def test_staged_equality_f64(engine, variant, shape):
    K, r, E = shape
    got, reduced = staged_check(engine, K, r, E, variant)
    assert engine.last_kernel() == "comp_link f64 r%d pairs" % r
    if variant in ("naive", "fixed"):
        assert np.all(got["ns"] == 1)
    if variant in ("None", "Whitening"):
        assert np.all(got["ns"] == r)
    if variant == "effec_throughput" and shape == (3, 2, 1):
        assert 0.25 * COUNT <= reduced <= 0.75 * COUNT        # the stream counts really vary at this point
    assert got["sym_err"].sum() > 0                           # an operating point at which the link makes errors


@pytest.mark.parametrize("case", ["one_symbol", "qam16_slicer", "qam16_mindist", "bpsk", "odd_symbols"])
@pytest.mark.parametrize("variant", co.VARIANTS)
def test_staged_equality_other_modulations(engine, variant, case):
    kw = dict(one_symbol=dict(ns=1), qam16_slicer=dict(mod="qam", M=16, slicer=True), qam16_mindist=dict(mod="qam", M=16),
              bpsk=dict(mod="bpsk", M=2), odd_symbols=dict(ns=67))[case]
    staged_check(engine, 3, 2, 1, variant, **kw)
    want = "comp_link f64 r2 %s" % ("single" if kw.get("ns", NS) % 2 else "pairs")
    assert engine.last_kernel() == want


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "K%dr%de%d" % s)
@pytest.mark.parametrize("variant", co.VARIANTS)
def test_f32_against_f64(engine, variant, shape):
    K, r, E = shape
    bind(engine, "psk", 4)
    _, g64 = run(engine, K, r, E, variant, "f64")
    _, g32 = run(engine, K, r, E, variant, "f32")
    assert np.array_equal(g32["ns"], g64["ns"])               # the solve is f64 in both
    symbols = int(g64["ns"].sum()) * NS
    assert abs(int(g32["sym_err"].sum()) - int(g64["sym_err"].sum())) <= 1e-4 * symbols
    assert np.all(np.abs(g32["sinr"] - g64["sinr"]) <= 1e-12 * np.abs(g64["sinr"]))


def test_identities(engine):
    bind(engine, "psk", 4)
    K, r = 3, 2
    pl, ple, iPu, pe = scenario(K, 1)
    _, se, be = engine.run_bd(K, r, NS, iPu, NOISE_VAR, SEED, FIRST, COUNT, pathloss=pl, waterfilling=False, dtype="f64",
                              per_realization=True)
    assert se.sum() > 0
    # no interferer antennas, metric None
    _, g = run(engine, K, r, 0, "None")
    assert np.array_equal(g["sym_err"], se) and np.array_equal(g["bit_err"], be)
    # an interferer of zero power
    _, g0 = run(engine, K, r, 1, "None", pe=0.0)
    assert np.array_equal(g0["sym_err"], se) and np.array_equal(g0["bit_err"], be)
    # 'fixed' with every stream kept == None in stream counts and transmit power: the same link up to the rotation of
    # the streams inside a user, so the per-user error statistics agree and the SINRs are those of an equal-power link
    _, gn = run(engine, K, r, 1, "None")
    _, gf = run(engine, K, r, 1, "fixed", num_streams=r)
    assert np.array_equal(gf["ns"], gn["ns"]) and np.all(gf["ns"] == r)
    H = channels(K, r, 1)
    sol = engine.bd_extint(H, K, r, 1, iPu, NOISE_VAR, pe, "enhanced", "fixed", num_streams=r)
    power = np.sum(np.abs(sol["Ms"]) ** 2, axis=(2, 3))
    assert np.all(np.abs(power - iPu) <= 1e-9 * iPu)          # every user transmits iPu, as under None
    # no noise, no interference: no errors in either arithmetic
    for dtype in ("f64", "f32"):
        for variant in co.VARIANTS:
            _, gz = run(engine, K, r, 1, variant, dtype, noise_var=1e-40 * NOISE_VAR, pe=0.0)
            assert gz["sym_err"].sum() == 0 and gz["bit_err"].sum() == 0, (dtype, variant)


@pytest.mark.parametrize("variant", ["None", "effec_throughput", "Whitening"])
def test_splits_and_per_realization_pathloss(engine, variant):
    bind(engine, "psk", 4)
    K, r, E = 3, 2, 1
    res, g = run(engine, K, r, E, variant)
    for cut in (1, 64, 77):
        ra, a = run(engine, K, r, E, variant, first=FIRST, count=cut)
        rb, b = run(engine, K, r, E, variant, first=FIRST + cut, count=COUNT - cut)
        for key in g:
            assert np.array_equal(np.concatenate([a[key], b[key]]), g[key]), (cut, key)
        for key in ("n_realizations", "n_skipped", "sym_errors", "sym_errors_sq", "bit_errors", "bit_errors_sq"):
            assert ra[key] + rb[key] == res[key]
    # adding into one counter block
    cnt = engine.new_counters()
    run(engine, K, r, E, variant, first=FIRST, count=64, counters=cnt, per_realization=False)
    run(engine, K, r, E, variant, first=FIRST + 64, count=COUNT - 64, counters=cnt, per_realization=False)
    both = engine.read_counters(cnt)
    assert all(both[k] == res[k] for k in res)
    # an empty range is a no-op
    z, gz = run(engine, K, r, E, variant, count=0)
    assert z["n_realizations"] == 0 and z["sym_errors"] == 0 and gz["sym_err"].size == 0
    assert engine.last_kernel() == ""
    # the constant set handed in per realization
    pl, ple, _, _ = scenario(K, E)
    per = np.broadcast_to(np.hstack([pl, ple])[None], (COUNT, K, K + E))
    rp, gp = run(engine, K, r, E, variant, pathloss=None, pathloss_ext=None, pathloss_per_realization=per)
    for key in g:
        assert np.array_equal(gp[key], g[key]), key
    assert rp == res


def test_argument_errors(engine):
    bind(engine, "psk", 4)
    before = engine.new_counters()
    bad = [dict(K=5), dict(r=5), dict(K=3, r=3), dict(E=9), dict(variant="fixed", num_streams=0),
           dict(variant="fixed", num_streams=3), dict(variant="effec_throughput", packet_length=0), dict(iPu=0.0),
           dict(ns=0), dict(pathloss=np.ones((2, 2))), dict(pathloss_ext=np.ones((3, 2))),
           dict(pathloss=None, pathloss_ext=None, pathloss_per_realization=np.ones((4, 3, 3)))]
    for kw in bad:
        kw = dict(kw)
        K, r, E, variant = kw.pop("K", 3), kw.pop("r", 2), kw.pop("E", 1), kw.pop("variant", "None")
        if "pathloss" not in kw and (K, E) != (3, 1):
            kw.update(pathloss=None, pathloss_ext=None)
        with pytest.raises(ValueError):
            run(engine, K, r, E, variant, count=4, counters=before, **kw)
        assert engine.last_kernel() == ""
    assert engine.read_counters(before)["n_realizations"] == 0        # nothing was launched
    with pytest.raises(ValueError):
        run(engine, 3, 2, 1, "nonsense", count=4)


def _mean_and_var(result):
    n = result.num_updates
    mean = result._result_sum / n
    return mean, max(result._result_squared_sum / n - mean * mean, 0.0) * n / (n - 1), n


def test_against_the_reference_run(engine):
    """CompSimulator on the fixture's scenario against the reference's own seeded run (independent draws): for every
    variant |ser - ser_ref| <= 4 sqrt(s2_ref / R_ref + s2_gpu / R_gpu), both variances from the sums and sums of squares
    of the per-realization values; the same for spec_effic."""
    from helpers import GOLDEN
    from pyphysim_amd.simulators import CompSimulator
    z = np.load(GOLDEN + "/g5_comp.npz", allow_pickle=False)
    R_ref = int(z["ref_realizations"])
    for pi, (snr, pe_dbm) in enumerate(z["ref_points"]):
        sim = CompSimulator([float(snr)], [float(pe_dbm)], modulator="psk", M=4, K=3, Nr=2, ext_int_rank=1, NSymbs=int(z["ref_nsymbs"]),
                            packet_length=int(z["ref_packet_length"]), pathloss=z["pathloss"], pathloss_ext=z["pathlossInt"],
                            rep_max=2000, batch_size=2000, seed=11, dtype="f64", engine=engine)
        sim.simulate()
        means = {}
        for v in co.VARIANTS:
            for m in ("ser", "spec_effic"):
                mean, var, n = _mean_and_var(sim.results["%s_%s" % (m, v)][0])
                s1, s2 = float(z["ref_p%d_%s_%s_sum" % (pi, m, v)]), float(z["ref_p%d_%s_%s_sq" % (pi, m, v)])
                mean_ref = s1 / R_ref
                var_ref = max(s2 / R_ref - mean_ref ** 2, 0.0) * R_ref / (R_ref - 1)
                bound = 4.0 * math.sqrt(var_ref / R_ref + var / n)
                print(pi, v, m, mean, mean_ref, bound)
                assert abs(mean - mean_ref) <= bound, (snr, pe_dbm, v, m, mean, mean_ref, bound)
                means[(m, v)] = mean
        if (float(snr), float(pe_dbm)) == (5.0, 10.0):
            assert means[("spec_effic", "capacity")] >= means[("spec_effic", "None")]
