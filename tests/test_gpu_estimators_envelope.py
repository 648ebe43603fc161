"""GPU: the LS / MMSE block-pilot estimators (csrc/kernels_estimators.hip) over their whole shape envelope, against the NumPy
restatement under common random numbers (tests/estimators_oracle.py; the case table ENVELOPE_CASES is checked on the
restatement alone by tests/test_estimators_envelope_cpu.py):

  * the pipeline's launches above the default dynamic-LDS limit (cases d, e, f, g: up to the 133 120-byte maximum), several
    trips per wavefront there, and small launches of the same kernel after its limit was raised;
  * a channel factor together with nt > 1, nt = 4 .. 7, fixed pilots with nt > 1 (cases g .. l);
  * the row-padding edges nr = 1, 15, 17, 113, 128 and P = 1, nt, 255, 256 (pipeline) and 1024 (operators);
  * realization indices across 2^32, bit for bit against the split that cuts there;
  * noise_power = 0 with a covariance (MMSE = LS = h);
  * the one-entry cache of the MMSE matrix: each of cov, n_pilots and noise_power alone replaces the entry, and returning
    to an earlier key returns the earlier bits.

Tolerances: the operator tolerances of tests/test_gpu_estimators.py and tests/test_gpu_pilot_mse.py (TOL: 1e-11 complex128,
2e-5 complex64) -- element-wise relative for the pipeline's err_ls, err_mmse and pow, relative to the largest expected element
for the staged operators.  Every test prints its worst figure and the kernel that served it.

Measured on an MI355X, next to the tolerance each was held to:
    pipeline, worst element-wise relative error of err_ls, err_mmse and pow over the twelve cases and both index ranges:
        complex128 6.64e-15 (case c, err_mmse) against 1e-11;  complex64 5.8e-06 (case a, err_ls) against 2e-5
        (the large-P complex64 cases d, f, g, k: 8.95e-07, 3.34e-07, 1.77e-07, 2.2e-07 -- no bound had to be derived)
    pipeline without noise, worst err / pow:  complex128 5.76e-31 against 1e-22;  complex64 1.49e-13 against 4e-10
    LS operator, relative to the largest element:    complex128 5.63e-15, complex64 1.27e-06   (both at 16 x 6 x 7)
    MMSE operator:                                   complex128 2.75e-15, complex64 1.08e-06   (both at 128 x 1024)
    MMSE operator without noise against LS:          complex128 7.72e-15, complex64 1.09e-06
    cache sequences (complex128):                    operator 2.36e-15, pipeline 1.25e-14
"""
import numpy as np
import pytest

import estimators_oracle as eo
from test_estimators_envelope_cpu import envelope_want, gram_cond, held_cond

pytestmark = pytest.mark.gpu

TOL = {"f64": 1e-11, "f32": 2e-5}
CDT = {"f64": np.complex128, "f32": np.complex64}
SEED, COUNT = eo.ENVELOPE_SEED, eo.ENVELOPE_COUNT
ACROSS = eo.ENVELOPE_FIRSTS[1]          # 2^32 - 5
CASES = sorted(eo.ENVELOPE_CASES)
DTYPES = ["f64", "f32"]


def run(engine, cfg, first, count, dtype):
    return engine.run_pilot_mse(cfg["nr"], cfg["nt"], cfg["n_pilots"], cfg["noise_power"], SEED, first, count,
                                pilot_power=cfg["pilot_power"], alpha=cfg["alpha"], pilots=cfg["pilots"],
                                chan_factor=cfg["L"], cov=cfg["cov"], dtype=dtype, per_realization=True)


def worst(got, want):
    return float(np.max(np.abs(got - want) / want))


def rel_err(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.max(np.abs(got.astype(np.complex128) - want)) / np.max(np.abs(want)))


def check_parity(engine, what, cfg, want, out, dtype):
    """The assertions of test_parity_under_common_random_numbers, for a case with or without a covariance."""
    res, e_ls, e_mm, pw = out
    keys = [("err_ls", e_ls), ("pow", pw)] + ([("err_mmse", e_mm)] if cfg["cov"] is not None else [])
    for key, got in keys:
        assert got.shape == want[key].shape and got.dtype == np.float64, key
        assert np.all(np.isfinite(got)) and np.all(got > 0), key
        if key != "pow":
            assert np.min(want[key] / want["pow"]) > 1e-2, key
    errs = {key: worst(got, want[key]) for key, got in keys}
    print(what, dtype, " ".join("%s %.3g" % kv for kv in sorted(errs.items())), "(element-wise relative)", engine.last_kernel())
    assert max(errs.values()) <= TOL[dtype], errs
    assert engine.last_kernel() == eo.envelope_kernel_name(cfg, dtype)
    assert res["n_realizations"] == len(pw) and res["err_ls"] == np.cumsum(e_ls)[-1] and res["pow"] == np.cumsum(pw)[-1]
    if cfg["cov"] is not None:
        assert res["err_mmse"] == np.cumsum(e_mm)[-1]
    else:
        assert e_mm is None and res["err_mmse"] is None


# ---- a. the parity table -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES)
def test_parity_over_the_case_table(engine, case, dtype):
    cfg = eo.ENVELOPE_CASES[case]
    check_parity(engine, "case " + case, cfg, envelope_want(case, 0), run(engine, cfg, 0, COUNT, dtype), dtype)


# ---- b. indices across 2^32 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["b", "i", "l"])
def test_realization_indices_across_2_to_the_32(engine, case, dtype):
    """Realizations 2^32 - 5 .. 2^32 + 31 in one call, and as 5 + 32 with the cut exactly at 2^32."""
    cfg = eo.ENVELOPE_CASES[case]
    whole = run(engine, cfg, ACROSS, COUNT, dtype)
    check_parity(engine, "case %s from 2^32 - 5" % case, cfg, envelope_want(case, ACROSS), whole, dtype)
    lo, hi = run(engine, cfg, ACROSS, 5, dtype), run(engine, cfg, 2 ** 32, 32, dtype)
    for i in (1, 2, 3):
        if whole[i] is not None:
            assert np.array_equal(np.concatenate([lo[i], hi[i]]), whole[i]), i


# ---- c. trips and grid invariance at the LDS maximum ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_trips_and_grid_invariance_at_the_lds_maximum(engine, dtype):
    """Case g (133 120 bytes of LDS per wavefront in complex128, 67 584 in complex64: one and two workgroups per compute
    unit, two realizations each).  `count` is two passes of the launcher's grid at grid_oversub = 1 and a tail of five, so
    every wavefront takes at least two trips and the tail falls in a third; grid_oversub = 8 gives every tile its own
    workgroup.  Then a small launch of another and of the same kernel instance after the dynamic-LDS limit was raised, and
    the large launch again."""
    g, small, same = eo.ENVELOPE_CASES["g"], eo.ENVELOPE_CASES["l"], eo.default_cfg(nr=3, nt=8, n_pilots=16, pilot_power=1.5, alpha=0.7)
    per_trip = eo.pilot_mse_per_trip(g, dtype, engine.n_cu)
    assert per_trip == engine.n_cu * {"f64": 1, "f32": 2}[dtype] * 2
    count = 2 * per_trip + 5
    tiles, grid = (count + 1) // 2, per_trip // 2
    assert tiles >= 2 * grid + 1 and (count - 1) // 2 >= 2 * grid and tiles <= 8 * grid
    before = [run(engine, cfg, 0, COUNT, dtype) for cfg in (small, same)]
    with engine.options(grid_oversub=1):
        _, e_ls, _, pw = run(engine, g, 0, count, dtype)
    assert engine.last_kernel() == eo.envelope_kernel_name(g, dtype)
    assert np.all(np.isfinite(e_ls)) and np.all(e_ls > 0) and np.all(pw > 0)
    with engine.options(grid_oversub=8):
        _, l8, _, p8 = run(engine, g, 0, count, dtype)
    assert np.array_equal(l8, e_ls) and np.array_equal(p8, pw)
    rows = np.array([0, per_trip - 1, per_trip, count - 1])
    want = eo.pilot_mse(SEED, rows, g)
    errs = [worst(e_ls[rows], want["err_ls"]), worst(pw[rows], want["pow"])]
    print("case g", dtype, "count", count, "probe rows: err_ls %.3g pow %.3g" % tuple(errs), engine.last_kernel())
    assert np.min(want["err_ls"] / want["pow"]) > 1e-2 and max(errs) <= TOL[dtype]
    for cfg, (_, b_ls, _, b_pw) in zip((small, same), before):
        _, a_ls, _, a_pw = run(engine, cfg, 0, COUNT, dtype)
        assert engine.last_kernel() == eo.envelope_kernel_name(cfg, dtype)
        assert np.array_equal(a_ls, b_ls) and np.array_equal(a_pw, b_pw)
    _, again_ls, _, again_pw = run(engine, g, 0, count, dtype)
    assert np.array_equal(again_ls, e_ls) and np.array_equal(again_pw, pw)


# ---- d. noise-free MMSE --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["b", "f"])
def test_mmse_and_ls_recover_the_channel_without_noise(engine, case, dtype):
    """noise_power = 0 with a covariance: no noise is drawn, A = (P C)^-1 C = I / P, so both estimates are h."""
    cfg = dict(eo.ENVELOPE_CASES[case], noise_power=0.0)
    res, e_ls, e_mm, pw = run(engine, cfg, 0, COUNT, dtype)
    assert engine.last_kernel() == "pilot_mse %s b16 ls+mmse gl" % dtype
    assert e_ls.shape == e_mm.shape == pw.shape == (COUNT,) and np.all(pw > 0)
    w_ls, w_mm = float(np.max(e_ls / pw)), float(np.max(e_mm / pw))
    w_pw = worst(pw, eo.pilot_mse(SEED, np.arange(COUNT), cfg)["pow"])
    print("case", case, dtype, "noise-free: worst err_ls / pow %.3g err_mmse / pow %.3g; pow %.3g" % (w_ls, w_mm, w_pw),
          engine.last_kernel())
    assert np.all(e_ls >= 0) and np.all(e_mm >= 0)
    assert w_ls <= TOL[dtype] ** 2 and w_mm <= TOL[dtype] ** 2
    assert w_pw <= TOL[dtype]


# ---- e. the staged operators on the same edges ---------------------------------------------------------------------------
LS_SHAPES = [(1, 1, 1, 37), (128, 8, 8, 33), (15, 4, 4, 37), (33, 5, 12, 37), (16, 6, 7, 37), (64, 7, 1024, 5), (3, 2, 1024, 37)]
MMSE_SHAPES = [(1, 1, 37), (15, 2, 37), (17, 9, 37), (113, 16, 19), (128, 1024, 5)]
_INPUTS = {}


def per_realization_pilots(nt, P, batch):
    """DFT rows under a per-realization phase ramp of the columns where P = nt (s s^H = P power I); random phases otherwise:
    the first `batch` draws of RandomState(5) whose Gram matrix is no worse conditioned than held_cond()."""
    rs = np.random.RandomState(5)
    if P == nt:
        return eo.dft_pilots(nt, P, 1.5)[None] * np.exp(2j * np.pi * rs.rand(batch, 1, P))
    s = np.sqrt(1.5) * np.exp(2j * np.pi * rs.rand(4 * batch, nt, P))
    s = s[np.linalg.cond(s @ np.conj(np.swapaxes(s, 1, 2))) <= held_cond()][:batch]
    assert len(s) == batch
    return s


def staged_inputs(nr, nt, P, batch, per, rho=None):
    """(Y [batch, nr, P], s [nt, P] or [batch, nt, P], C): h and the noise are the pipeline's own (eo.pilot_mse) where it
    reaches (P <= 256), NumPy's RandomState(7) in the same model otherwise; computed once per key."""
    key = (nr, nt, P, batch, per, rho)
    if key not in _INPUTS:
        C0 = eo.toeplitz_cov(nr, rho)
        shared = eo.dft_pilots(nt, P, 1.5) if P == nt else eo.random_phase_pilots(nt, P, 1.5)
        s = per_realization_pilots(nt, P, batch) if per else shared
        assert gram_cond(s) <= held_cond()
        if P <= eo.MAX_PIPELINE_PILOTS:
            cfg = eo.default_cfg(nr=nr, nt=nt, n_pilots=P, pilot_power=1.5, noise_power=0.5, alpha=0.7, pilots=shared,
                                 L=np.linalg.cholesky(C0) if rho else None)
            base = eo.pilot_mse(SEED, np.arange(batch), cfg)
            h, noise = base["h"], base["Y"] - base["h"] @ base["s"]
        else:
            rs = np.random.RandomState(7)
            w = (rs.randn(batch, nr, nt) + 1j * rs.randn(batch, nr, nt)) / np.sqrt(2.0)
            h = 0.7 * (np.linalg.cholesky(C0) @ w if rho else w)
            noise = np.sqrt(0.5 / 2.0) * (rs.randn(batch, nr, P) + 1j * rs.randn(batch, nr, P))
        _INPUTS[key] = (h @ s + noise, s, 0.49 * C0)
        for v in _INPUTS[key]:
            v.setflags(write=False)
    return _INPUTS[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("per", [False, True], ids=["shared", "per_realization"])
@pytest.mark.parametrize("shape", LS_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_ls_operator_on_the_envelope(engine, shape, per, dtype):
    nr, nt, P, batch = shape
    Y, s, _ = staged_inputs(nr, nt, P, batch, per)
    got = engine.ls_estimate(Y, s, dtype=dtype)
    e = rel_err(got, eo.ls_estimate(Y, s))
    print(shape, "per" if per else "shared", dtype, "ls %.3g" % e, engine.last_kernel())
    assert got.dtype == CDT[dtype] and got.shape == (batch, nr, nt) and e <= TOL[dtype]
    assert engine.last_kernel() == "ls_estimate %s nt%d" % (dtype, eo.ntp_of(nt))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("per", [False, True], ids=["shared", "per_realization"])
@pytest.mark.parametrize("shape", MMSE_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_mmse_operator_on_the_envelope(engine, shape, per, dtype):
    """With noise_power = 0.5 against the restatement; with noise_power = 0 (A = I / P) against the LS estimate of the same
    inputs."""
    nr, P, batch = shape
    Y, s, C = staged_inputs(nr, 1, P, batch, per, rho=0.9 if nr <= 17 else 0.7)
    got = engine.mmse_estimate(Y, s, 0.5, C, dtype=dtype)
    e = rel_err(got, eo.mmse_estimate(Y, s, 0.5, C))
    quiet = engine.mmse_estimate(Y, s, 0.0, C, dtype=dtype)
    e0 = rel_err(quiet, eo.ls_estimate(Y, s))
    print(shape, "per" if per else "shared", dtype, "mmse %.3g; noise-free against ls %.3g" % (e, e0), engine.last_kernel())
    assert got.dtype == CDT[dtype] and got.shape == (batch, nr, 1) and e <= TOL[dtype]
    assert e0 <= TOL[dtype]
    assert engine.last_kernel() == "mmse_estimate %s ga" % dtype


# ---- f. the cache of the MMSE matrix -------------------------------------------------------------------------------------
def cache_sequence(call):
    """The five calls of the cache test; `call(C, noise_power, P)` -> (got, want).  C2 is C1 with one off-diagonal pair changed
    IN PLACE, so the host address of the covariance stays.  Returns the five (got, want)."""
    C = np.array(eo.ENVELOPE_CASES["c"]["cov"], dtype=np.complex128, order="C")
    c1 = (C[2, 5], C[5, 2])
    out = [call(C, 0.5, 9)]
    C[2, 5] = c1[0] + (0.05 + 0.02j)
    C[5, 2] = np.conj(C[2, 5])
    out.append(call(C, 0.5, 9))
    C[2, 5], C[5, 2] = c1
    out.append(call(C, 0.25, 9))
    out.append(call(C, 0.5, 9))
    out.append(call(C, 0.5, 8))
    return out


def test_mmse_matrix_cache_follows_every_part_of_its_key_operator(engine):
    want_c = envelope_want("c", 0)
    Y, s = want_c["Y"], eo.ENVELOPE_CASES["c"]["pilots"]

    def call(C, noise_power, P):
        got = engine.mmse_estimate(Y[..., :P], s[:, :P], noise_power, C, dtype="f64")
        return got, eo.mmse_estimate(Y[..., :P], s[:, :P], noise_power, C.copy())

    out = cache_sequence(call)
    errs = [rel_err(got, want) for got, want in out]
    print("cache, operator: " + " ".join("%.3g" % e for e in errs))
    assert max(errs) <= TOL["f64"]
    # the keys differ by far more than the tolerance: a stale entry cannot pass
    for i in (1, 2):
        assert rel_err(out[i][1], out[0][1]) > 1e3 * TOL["f64"]
    # (the fifth call with the entry of P = 9 left in place: A of nine pilots applied to the matched filter of eight)
    z8 = (Y[..., :8] @ np.conj(s[:, :8].T)) * (8 / np.real(s[:, :8] @ np.conj(s[:, :8].T)))
    assert rel_err(eo.mmse_matrix(9, 0.5, eo.ENVELOPE_CASES["c"]["cov"]) @ z8, out[4][1]) > 1e3 * TOL["f64"]
    assert np.array_equal(out[3][0], out[0][0])


def test_mmse_matrix_cache_follows_every_part_of_its_key_pipeline(engine):
    """The same sequence through mcle_run_pilot_mse on err_mmse.  (At noise_power = 0.25 the restatement's smallest
    err_mmse / pow is 0.0093: complex128 leaves five orders of magnitude between its rounding and TOL, so the guard here is
    5e-3.)"""
    base = eo.ENVELOPE_CASES["c"]

    def call(C, noise_power, P):
        cfg = dict(base, cov=C, noise_power=noise_power, n_pilots=P, pilots=base["pilots"][:, :P])
        got = run(engine, cfg, 0, COUNT, "f64")[2]
        want = eo.pilot_mse(SEED, np.arange(COUNT), dict(cfg, cov=C.copy()))
        assert np.min(want["err_mmse"] / want["pow"]) > 5e-3
        return got, want["err_mmse"]

    out = cache_sequence(call)
    errs = [worst(got, want) for got, want in out]
    print("cache, pipeline: " + " ".join("%.3g" % e for e in errs))
    assert max(errs) <= TOL["f64"]
    assert worst(out[1][1], out[0][1]) > 1e3 * TOL["f64"]
    assert np.array_equal(out[3][0], out[0][0])
