"""50-digit reference of the general-geometry iterative IA solver (Engine.ia_solve_general).  TEST INFRASTRUCTURE.

A plain mpmath restatement (mp.dps = 50; mpmath.eigh, lu_solve, svd_c) of what oracle/ia.py::general_solve restates in
NumPy: calc_Q / calc_Q_rev, the update pairs of AlternatingMin / MinLeakage / MaxSinr, _is_diff_significant, the 'svd'
start, _solve_finalize, full_W_H, the SINRs and the sum capacity, and the greedy / brute-force wrappers with the
reference's iteration bookkeeping (paths and line numbers: the header of oracle/ia.py).  Eigenvectors (and the singular
vectors of the 'svd' start) take the solver's stated phase convention -- the component of largest modulus is real and
positive -- so that F, the `rel > 0` stopping test and the iteration counts are comparable.

Beside the results every run returns the margin of each discrete decision it took (`margins`), and `sensitivity` gives
the movement of the results under a 1e-14 relative perturbation of the channel: a case is STRICT when every realization
has sensitivity <= 1e-8 and every margin >= 1e-6 (the margin "stop0" apart: with rel = 0 the loop stops on `dmax > 0`,
which an iterate that converges in finitely many steps decides by rounding noise; such a case keeps every comparison but
the iteration count -- `iterations_pinned`) (tests/test_ia_general_envelope_cpu.py asserts it from the fixture
tests/golden/g7_ia_envelope.npz, written by scripts/make_golden_ia_envelope.py).  Channels and starts are drawn from
np.random.RandomState, so the fixture stores seeds and not matrices."""
import functools
import itertools
import json
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 50

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g7_ia_envelope.npz")
COST_ITERATIONS = (0, 1, 2, 3, 5, 8)
QUANTITIES = ("capacity", "sinr", "PF", "PU")
MARGINS = ("stop", "select", "cond", "phase", "stop0")
PERTURBATION = 1e-14
STRICT_SENSITIVITY, STRICT_MARGIN = 1e-8, 1e-6
EPS = 2.0 ** -52


# ---- the case table ------------------------------------------------------------------------------------------------
def _case(kind, K, nr, nt, Ns, algo, init, rel, max_iterations, select=None, noise_var=0.01, n_real=3, seed=None):
    ns = [int(Ns)] * K if np.isscalar(Ns) else [int(n) for n in Ns]
    # one seed per shape: every algorithm and start of a shape sees the same channels
    seed = 7000 + 1000 * K + 100 * nr + 10 * nt + sum((i + 1) * n for i, n in enumerate(ns)) if seed is None else seed
    name = "%s-%s-K%d-%dx%d-Ns%s-%s-rel%g-it%d%s%s" % (kind, algo, K, nr, nt, "".join(map(str, ns)), init, rel, max_iterations,
                                                       "-" + select if select else "", "-nv0" if noise_var == 0 else "")
    return dict(name=name, kind=kind, K=K, nr=nr, nt=nt, Ns=ns, algo=algo, init=init, rel=rel, max_iterations=max_iterations,
                select=select, noise_var=noise_var, n_real=n_real, seed=seed)


STRICT_SHAPES = [(2, 2, 2, 1), (2, 1, 1, 1), (4, 2, 2, 1), (4, 3, 3, 1), (4, 4, 4, 1), (4, 4, 4, (2, 1, 1, 1)),
                 (3, 4, 5, 2), (3, 5, 4, 2), (3, 5, 3, 2)]
MAX_SINR_SHAPES = [(2, 3, 3, (2, 1)), (2, 6, 6, 3), (4, 6, 6, (2, 1, 2, 1)), (3, 3, 6, (1, 2, 3)), (3, 6, 1, 1), (3, 1, 4, 1),
                   (4, 5, 5, 1)]
ALGOS = ("alt_min", "min_leakage", "max_sinr")
# seeds replaced because a realization of the shape's default seed failed the strict condition: {(shape, algo): seed}
RESEEDED = {}


def _build_cases():
    cases = []
    for shape in STRICT_SHAPES:
        for algo in ALGOS:
            seed = RESEEDED.get((shape, algo))
            cases.append(_case("strict", *shape, algo, "fix", 0.0, 8, seed=seed))
            cases.append(_case("strict", *shape, algo, "fix", 1e-6, 80, seed=seed))
            if shape[1] == shape[2]:
                cases.append(_case("strict", *shape, algo, "svd", 0.0, 8, seed=seed))
    for shape in MAX_SINR_SHAPES:
        seed = RESEEDED.get((shape, "max_sinr"))
        cases.append(_case("strict", *shape, "max_sinr", "fix", 0.0, 8, seed=seed))
        cases.append(_case("strict", *shape, "max_sinr", "fix", 1e-6, 80, seed=seed))
    for shape in MAX_SINR_SHAPES:
        for algo in ("alt_min", "min_leakage"):
            cases.append(_case("slack", *shape, algo, "fix", 0.0, 8))
    cases.append(_case("select", 2, 3, 3, 3, "max_sinr", "fix", 1e-6, 40, select="greedy", seed=RESEEDED.get("greedy-2")))
    cases.append(_case("select", 4, 4, 4, 2, "max_sinr", "fix", 1e-6, 40, select="greedy", seed=RESEEDED.get("greedy-4")))
    cases.append(_case("select", 4, 2, 2, 2, "max_sinr", "svd", 1e-6, 40, select="brute", seed=RESEEDED.get("brute-16")))
    cases.append(_case("select", 3, 3, 3, (1, 2, 3), "max_sinr", "svd", 1e-6, 40, select="brute", seed=RESEEDED.get("brute-6")))
    cases.append(_case("select", 4, 4, 4, 4, "max_sinr", "svd", 1e-6, 1, select="brute", n_real=1, seed=RESEEDED.get("brute-256")))
    # noise_var = 0 with interference of full rank at every receiver
    for algo in ALGOS:
        cases.append(_case("strict", 4, 2, 2, 1, algo, "fix", 0.0, 8, noise_var=0.0))
    return cases


CASES = _build_cases()
CASE_BY_NAME = {c["name"]: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
# 130 distinct problems each, one lane per problem: three waves in two blocks of 64 + a ragged tail, lanes that stop at
# different iterations.  Not in the fixture: batches are compared with the same problems solved one per call.
# noise_var = 1: at the table's 0.01 max-SINR needs 170 to 400 and more iterations to meet rel = 1e-3 (measured with
# oracle.ia), so that every lane would run into max_iterations = 60; at 1 the counts spread from about 20 to 60.
BATCH_CASES = [_case("batch", 3, 3, 3, 1, "max_sinr", "fix", 1e-3, 60, n_real=130, noise_var=1.0),
               _case("batch", 3, 5, 4, 2, "max_sinr", "fix", 1e-3, 60, n_real=130, noise_var=1.0)]


def randn_c(rs, rows, cols):
    return (rs.randn(rows, cols) + 1j * rs.randn(rows, cols)) / np.sqrt(2.0)


def draw(case, r):
    """-> (big_H [K nr, K nt], F_init list of nt x Ns[k], unit Frobenius norm) of realization r, complex128."""
    rs = np.random.RandomState([int(case["seed"]), int(r)])
    big_H = randn_c(rs, case["K"] * case["nr"], case["K"] * case["nt"])
    F = []
    for k in range(case["K"]):
        f = randn_c(rs, case["nt"], case["Ns"][k])
        F.append(f / np.linalg.norm(f, "fro"))
    return big_H, F


def perturbed(case, r, big_H):
    rs = np.random.RandomState([int(case["seed"]), int(r), 1])
    return big_H * (1.0 + PERTURBATION * rs.randn(*big_H.shape))


def pad_F(F_list, D):
    """[K] list of nt x ns -> [4, D, D] zero padded (the engine's F_init layout)."""
    out = np.zeros((4, D, D), dtype=complex)
    for k, f in enumerate(F_list):
        out[k, :f.shape[0], :f.shape[1]] = f
    return out


# ---- small mp helpers ----------------------------------------------------------------------------------------------
def to_mp(a):
    a = np.asarray(a)
    m = mp.matrix(a.shape[0], a.shape[1])
    for i in range(a.shape[0]):
        for j in range(a.shape[1]):
            m[i, j] = mp.mpc(float(a[i, j].real), float(a[i, j].imag))
    return m


def to_np(m):
    return np.array([[complex(m[i, j]) for j in range(m.cols)] for i in range(m.rows)], dtype=complex).reshape(m.rows, m.cols)


def _blocks(big_H, K, nr, nt):
    return [[to_mp(big_H[k * nr:(k + 1) * nr, l * nt:(l + 1) * nt]) for l in range(K)] for k in range(K)]


def _fro(A):
    return mp.sqrt(mp.fsum(abs(A[i, j]) ** 2 for i in range(A.rows) for j in range(A.cols)))


def _cols(A, idx):
    out = mp.matrix(A.rows, len(idx))
    for j, c in enumerate(idx):
        for i in range(A.rows):
            out[i, j] = A[i, c]
    return out


def _rows(A, n):
    out = mp.matrix(n, A.cols)
    for i in range(n):
        for j in range(A.cols):
            out[i, j] = A[i, j]
    return out


def _hstack(A, B):
    out = mp.matrix(A.rows, A.cols + B.cols)
    for i in range(A.rows):
        for j in range(A.cols):
            out[i, j] = A[i, j]
        for j in range(B.cols):
            out[i, A.cols + j] = B[i, j]
    return out


def _outer(A):
    return A * A.H


def _solve(A, B):
    """A X = B, column by column (mpmath.lu_solve)."""
    out = mp.matrix(A.cols, B.cols)
    for j in range(B.cols):
        x = mp.lu_solve(A, B[:, j])
        for i in range(A.cols):
            out[i, j] = x[i]
    return out


def _canonical(V, cols, rec):
    """Columns `cols` of V: the component of largest modulus made real and positive; the margin of that choice recorded."""
    for j in cols:
        mods = [abs(V[i, j]) for i in range(V.rows)]
        m = max(range(V.rows), key=lambda i: mods[i])
        if rec is not None:
            srt = sorted(mods, reverse=True)
            rec["phase"].append(mp.mpf(1) if len(srt) < 2 else 1 - srt[1] / srt[0])
        ph = mp.conj(V[m, j]) / mods[m]
        for i in range(V.rows):
            V[i, j] = V[i, j] * ph
        V[m, j] = mp.mpc(mods[m], 0)


def _eigh(A):
    """-> (eigenvalues ascending as a list, eigenvectors in the columns)."""
    if A.rows == 1:
        return [mp.re(A[0, 0])], mp.matrix([[mp.mpc(1)]])
    E, Q = mp.eigh((A + A.H) / 2)
    return [E[i] for i in range(A.rows)], Q


def leig(A, n, rec=None):
    """Eigenvectors of the n smallest eigenvalues, ascending, canonical phase (util/misc.py leig)."""
    _, Q = _eigh(A)
    _canonical(Q, range(n), rec)
    return _cols(Q, list(range(n)))


def peig(A, n):
    """Eigenvectors of the n largest eigenvalues, descending (util/misc.py peig).  Only their span is used."""
    _, Q = _eigh(A)
    return _cols(Q, [A.rows - 1 - j for j in range(n)])


def calc_Q(H, F, k, noise_var):
    Q = mp.zeros(H[k][k].rows)
    for l in range(len(F)):
        if l != k:
            Q = Q + _outer(H[k][l] * F[l])
    return Q + mp.eye(Q.rows) * noise_var


def calc_Q_rev(H, W, k):
    Q = mp.zeros(H[k][k].cols)
    for l in range(len(W)):
        if l != k:
            Q = Q + _outer(H[l][k].H * W[l])
    return Q


def is_diff_significant(F_old, F_new, rel, rec):
    for fo, fn in zip(F_old, F_new):
        dmax = max(abs(fn[i, j] - fo[i, j]) for i in range(fn.rows) for j in range(fn.cols))
        fmin = min(abs(fn[i, j]) for i in range(fn.rows) for j in range(fn.cols))
        if rel > 0 and fmin > 0:
            rec["stop"].append(abs(dmax / (fmin * rel) - 1))
        elif rel == 0 and fmin > 0:
            # `dmax > 0`: an iterate that has converged to the last digit stops (or not) on rounding noise alone
            rec["stop0"].append(dmax / fmin)
        if dmax > fmin * rel:
            return True
    return False


def _iterate(F, step, max_iterations, rel, rec, history):
    old_F, state, runned = F, None, 0
    for _ in range(max_iterations):
        runned += 1
        F, state = step(F, state)
        if history is not None:
            history.append(F)
        if not is_diff_significant(old_F, F, rel, rec):
            break
        old_F = F
    return F, state, runned


def _alt_min(H, F0, nv, max_iterations, rel, full_F_first, rec, history):
    K = len(F0)
    Ns = [f.cols for f in F0]
    Nr = [H[k][k].rows for k in range(K)]

    def update_C(F):
        return [peig(calc_Q(H, F, k, nv), Nr[k] - Ns[k]) for k in range(K)]

    def step(F, C):
        if C is None:
            C = update_C(F if full_F_first is None else full_F_first)
        Y = [mp.eye(Nr[k]) - (C[k] * C[k].H if C[k].cols else mp.zeros(Nr[k])) for k in range(K)]
        newF = [mp.zeros(H[0][k].cols) for k in range(K)]
        for (l, k) in itertools.permutations(range(K), 2):
            newF[l] = newF[l] + H[k][l].H * Y[k] * H[k][l]
        F = []
        for k in range(K):
            f = leig(newF[k], Ns[k], rec)
            F.append(f / _fro(f))
        return F, update_C(F)

    F, C, runned = _iterate(F0, step, max_iterations, rel, rec, history)
    W_H = []
    for k in range(K):
        M = _hstack(H[k][k] * F[k], C[k]) if C[k].cols else H[k][k] * F[k]
        W_H.append(_rows(_solve(M, mp.eye(M.rows)), Ns[k]))
    return F, W_H, runned


def _min_leakage(H, F0, nv, max_iterations, rel, full_F_first, rec, history):
    K = len(F0)
    Ns = [f.cols for f in F0]

    def update_W(F):
        return [leig(calc_Q(H, F, k, nv), Ns[k]) for k in range(K)]

    def step(F, W):
        if W is None:
            W = update_W(F if full_F_first is None else full_F_first)
        F = [leig(calc_Q_rev(H, W, k), Ns[k], rec) for k in range(K)]
        # beyond the reference (one stream, where the eigenvector is the unit-norm precoder): unit power per user
        F = [f / _fro(f) if f.cols > 1 else f for f in F]
        return F, update_W(F)

    F, W, runned = _iterate(F0, step, max_iterations, rel, rec, history)
    return F, [w.H for w in W], runned


def _max_sinr(H, F0, nv, max_iterations, rel, full_F_first, rec, history):
    K = len(F0)

    def calc_U(Hkk_of, V, chan, per_stream_power, V_cov=None):
        out = []
        Vc = V if V_cov is None else V_cov
        for k in range(K):
            Hkk = Hkk_of(k)
            first = mp.zeros(Hkk.rows)
            for j in range(K):
                a = _outer(chan(k, j) * Vc[j])
                first = first + (a / V[j].cols if per_stream_power else a)
            U = mp.matrix(Hkk.rows, V[k].cols)
            for l in range(V[k].cols):
                a = _outer(Hkk * Vc[k][:, l])
                B = first - (a / V[k].cols if per_stream_power else a) + mp.eye(Hkk.rows) * nv
                u = mp.lu_solve(B, Hkk * V[k][:, l])
                n = _fro(u)
                for i in range(Hkk.rows):
                    U[i, l] = u[i] / n
            out.append(U / _fro(U))
        return out

    fwd = lambda k, j: H[k][j]
    rev = lambda k, j: H[j][k].H

    def update_W(F, F_cov=None):
        return calc_U(lambda k: H[k][k], F, fwd, False, F_cov)

    def step(F, W):
        if W is None:
            W = update_W(F, full_F_first)
        F = calc_U(lambda k: H[k][k].H, W, rev, True)
        return F, update_W(F)

    F, W, runned = _iterate(F0, step, max_iterations, rel, rec, history)
    return F, [w.H for w in W], runned


_ALGO = {"alt_min": _alt_min, "min_leakage": _min_leakage, "max_sinr": _max_sinr}


def svd_init(H, Ns, rec):
    """The Ns[k] most significant right singular vectors of H_kk in the reference's column order (the reversed index list
    of least_right_singular_vectors: columns Ns-1 ... 0 of the descending ordering), Frobenius-normalised."""
    F = []
    for k in range(len(H)):
        _, _, Vh = mp.svd_c(H[k][k])
        V = Vh.H
        V1 = _cols(V, [Ns[k] - 1 - j for j in range(Ns[k])])
        _canonical(V1, range(Ns[k]), rec)
        F.append(V1 / _fro(V1))
    return F


def principal_components(A, n):
    U, S, Vh = mp.svd_c(A)
    out = mp.zeros(A.rows, n)
    for i in range(A.rows):
        for c in range(n):
            out[i, c] = sum((U[i, m] * S[m] * Vh[m, c] for m in range(n)), mp.mpc(0))
    return out


def solve_finalize(F, W_H, rec):
    F, W_H = list(F), list(W_H)
    for k in range(len(F)):
        if F[k].cols > 1:
            S = mp.svd_c(F[k], compute_uv=False)
            S = [S[i] for i in range(len(S))]
            smax, smin = max(S), min(S)
            rec["cond"].append(abs(smax / (smin * mp.mpf(10) ** 4) - 1) if smin > 0 else mp.inf)
            if smin == 0 or smax / smin > 1e4:
                rec["cond"].extend(abs(s * mp.mpf(10) ** 4 / smax - 1) for s in S)
                n = sum(1 for s in S if s > smax / mp.mpf(10) ** 4)
                f = principal_components(F[k], n)
                F[k] = f / _fro(f)
                W_H[k] = principal_components(W_H[k].H, n).H
    return F, W_H, [f.cols for f in F]


def evaluate(H, F, W_H, nv):
    """-> (U = full_W_H, per-user SINR lists, sum capacity)."""
    K = len(F)
    U = [_solve(W_H[k] * (H[k][k] * F[k]), W_H[k]) for k in range(K)]
    sinr = []
    for k in range(K):
        first = mp.zeros(H[k][k].rows)
        for j in range(K):
            first = first + _outer(H[k][j] * F[j])
        s_k = []
        for l in range(F[k].cols):
            a = H[k][k] * F[k][:, l]
            B = first - _outer(a) + mp.eye(first.rows) * nv
            u_h = U[k][l, :]
            num = (u_h * a)[0, 0]
            den = (u_h * B * u_h.H)[0, 0]
            s_k.append(abs(num * mp.conj(num) / den))
        sinr.append(s_k)
    cap = mp.fsum(mp.log(1 + s, 2) for s_k in sinr for s in s_k)
    return U, sinr, cap


def _relgap(a, b):
    m = max(abs(a), abs(b))
    return abs(a - b) / m if m > 0 else mp.mpf(0)


def mp_solve(case, big_H, F_init, history=None):
    """The whole solve of `case` on one channel in mp -> dict(F, U, sinr, cap, Ns, runned[, every], margins)."""
    K, nv = case["K"], mp.mpf(case["noise_var"])
    H = _blocks(big_H, K, case["nr"], case["nt"])
    rec = {m: [] for m in MARGINS}
    rel = mp.mpf(case["rel"])
    run = _ALGO[case["algo"]]

    def solve(F0, full_F_first=None, hist=None):
        F, W_H, runned = run(H, F0, nv, case["max_iterations"], rel, full_F_first, rec, hist)
        F, W_H, ns = solve_finalize(F, W_H, rec)
        U, sinr, cap = evaluate(H, F, W_H, nv)
        return dict(F=F, U=U, sinr=sinr, cap=cap, Ns=ns), runned

    if case["select"] == "brute":
        best, total, every = None, 0, []
        for comb in itertools.product(*[range(1, n + 1) for n in case["Ns"]]):
            sol, runned = solve(svd_init(H, comb, rec))
            total += runned
            every.append(sol["cap"])
            if best is None or sol["cap"] > best["cap"]:
                best = sol
        srt = sorted(every, reverse=True)
        if len(srt) > 1:
            rec["select"].append(_relgap(srt[0], srt[1]))
        best = dict(best, runned=total, every=every)
        sol = best
    else:
        F0 = svd_init(H, case["Ns"], rec) if case["init"] == "svd" else [to_mp(f) for f in F_init]
        if history is not None:
            history.append(F0)
        sol, counter = solve(F0, None, history)
        total = counter
        while case["select"] == "greedy" and any(n > 1 for n in sol["Ns"]):
            old = sol
            sinr, ns = sol["sinr"], sol["Ns"]
            mins = [min(range(ns[i]), key=lambda l: sinr[i][l]) for i in range(K)]
            order = [i for i in sorted(range(K), key=lambda i: sinr[i][mins[i]]) if ns[i] > 1]
            user, stream = order[0], mins[order[0]]
            keep = [c for c in range(ns[user]) if c != stream]
            F = list(sol["F"])
            full_F = list(sol["F"])
            full_F[user] = _cols(F[user], keep)
            F[user] = full_F[user] / _fro(full_F[user])
            sol, runned = solve(F, full_F)
            counter += runned
            total += counter
            rec["select"].append(_relgap(old["cap"], sol["cap"]))
            if old["cap"] > sol["cap"]:
                sol = old
                break
        sol = dict(sol, runned=total)
    sol["margins"] = {m: (float(min(v)) if v else float("inf")) for m, v in rec.items()}
    return sol


# ---- results as f64 arrays -----------------------------------------------------------------------------------------
def herm_pack(P):
    """Hermitian [.., n, n] complex -> real [.., n, n]: real parts on and above the diagonal, imaginary parts below."""
    P = np.asarray(P)
    n = P.shape[-1]
    iu = np.triu_indices(n, 1)
    out = np.array(P.real)
    out[..., iu[1], iu[0]] = P.imag[..., iu[0], iu[1]]
    return out


def herm_unpack(R):
    R = np.asarray(R)
    n = R.shape[-1]
    iu = np.triu_indices(n, 1)
    out = np.zeros(R.shape, dtype=complex)
    out[..., iu[0], iu[1]] = R[..., iu[0], iu[1]] + 1j * R[..., iu[1], iu[0]]
    out = out + np.conj(np.swapaxes(out, -1, -2))
    idx = np.arange(n)
    out[..., idx, idx] = R[..., idx, idx]
    return out


def summarise(case, sol):
    """mp solution -> f64: PF [K, nt, nt], PU [K, nr, nr], sinr [K, D] zero padded, capacity, Ns, iterations[, every]."""
    K, D = case["K"], max(case["nr"], case["nt"])
    out = dict(PF=np.stack([to_np(f * f.H) for f in sol["F"]]), PU=np.stack([to_np(u.H * u) for u in sol["U"]]),
               sinr=np.zeros((K, D)), capacity=float(sol["cap"]), Ns_final=np.array(sol["Ns"], dtype=np.int64),
               iterations=int(sol["runned"]))
    for k in range(K):
        out["sinr"][k, :len(sol["sinr"][k])] = [float(s) for s in sol["sinr"][k]]
    if "every" in sol:
        out["every_capacity"] = np.array([float(c) for c in sol["every"]])
    return out


def summarise_np(case, sol):
    """The same quantities of oracle.ia.general_solve's result."""
    K, D = case["K"], max(case["nr"], case["nt"])
    out = dict(PF=np.stack([f @ f.conj().T for f in sol["F"]]), PU=np.stack([u.conj().T @ u for u in sol["U"]]),
               sinr=np.zeros((K, D)), capacity=float(sol["cap"]), Ns_final=np.array(sol["Ns"], dtype=np.int64),
               iterations=int(sol["runned"]))
    for k in range(K):
        out["sinr"][k, :len(sol["sinr"][k])] = sol["sinr"][k]
    if "every_sum_capacity" in sol:
        out["every_capacity"] = np.array(sol["every_sum_capacity"])
    return out


def relmax(got, want):
    """max |got - want| / max |want| (the error measure of every comparison of this envelope)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return float("inf")
    scale = float(np.max(np.abs(want))) if want.size else 0.0
    return float(np.max(np.abs(got - want))) / scale if scale > 0 else float(np.max(np.abs(got - want), initial=0.0))


def errors(got, want):
    """-> relmax of two summaries per quantity of QUANTITIES (+ every_capacity where the case has it)."""
    names = QUANTITIES + (("every_capacity",) if "every_capacity" in want else ())
    return np.array([relmax(got[q], want[q]) for q in names])


def numpy_solve(case, big_H, F_init):
    from oracle import ia as oia
    H = oia.split_blocks(big_H, case["K"], case["nr"], case["nt"])
    sol = oia.general_solve(case["algo"], H, case["Ns"], case["noise_var"], case["max_iterations"], case["rel"],
                            F_init=None if (case["init"] == "svd" or case["select"] == "brute") else F_init,
                            select=case["select"])
    return summarise_np(case, sol)


def run_case(case, r):
    """mp results of realization r as f64 arrays (+ margins [len(MARGINS)], cost [len(COST_ITERATIONS)] for the two
    leakage-minimising algorithms: NaN past the iterations the run took)."""
    big_H, F_init = draw(case, r)
    history = [] if case["algo"] != "max_sinr" and not case["select"] else None
    sol = mp_solve(case, big_H, F_init, history)
    out = summarise(case, sol)
    out["margins"] = np.array([sol["margins"][m] for m in MARGINS])
    if history is not None:
        H = _blocks(big_H, case["K"], case["nr"], case["nt"])
        out["cost"] = np.array([float(_cost_mp(H, history[n], case["Ns"])) if n < len(history) else np.nan
                                for n in COST_ITERATIONS])
    return out


def sensitivity(case, r, base=None):
    """Relative movement [len(QUANTITIES)] of capacity, SINRs, F_k F_k^H and U_k^H U_k when H is multiplied entry-wise by
    1 + 1e-14 N(0, 1), both runs in mp."""
    big_H, F_init = draw(case, r)
    if base is None:
        base = summarise(case, mp_solve(case, big_H, F_init))
    moved = summarise(case, mp_solve(case, perturbed(case, r, big_H), F_init))
    return errors(moved, base)


# ---- the leakage both alt-min and min-leakage minimise in turn -------------------------------------------------------
def _cost_mp(H, F, ns):
    K = len(F)
    B = []
    for k in range(K):
        U, _, _ = mp.svd_c(F[k])
        B.append(_cols(U, list(range(ns[k]))))
    total = mp.mpf(0)
    for k in range(K):
        Q = mp.zeros(H[k][k].rows)
        for l in range(K):
            if l != k:
                Q = Q + _outer(H[k][l] * B[l])
        E, _ = _eigh(Q)
        total += mp.fsum(E[:ns[k]])
    return total


def cost(big_H, F, ns, use_mp=False):
    """sum_k of the ns[k] smallest eigenvalues of the noise-free interference covariance at receiver k, every F_k
    orthonormalised first.  big_H [K nr, K nt], F: list of K matrices nt x ns[k].  f64 (eigvalsh) unless use_mp."""
    K = len(F)
    nr, nt = big_H.shape[0] // K, big_H.shape[1] // K
    if use_mp:
        return float(_cost_mp(_blocks(big_H, K, nr, nt), [to_mp(f) for f in F], ns))
    B = [np.linalg.svd(np.asarray(f), full_matrices=False)[0][:, :ns[k]] for k, f in enumerate(F)]
    total = 0.0
    for k in range(K):
        Q = np.zeros((nr, nr), dtype=complex)
        for l in range(K):
            if l != k:
                a = big_H[k * nr:(k + 1) * nr, l * nt:(l + 1) * nt] @ B[l]
                Q = Q + a @ a.conj().T
        total += float(np.sum(np.linalg.eigvalsh(Q)[:ns[k]]))
    return total


# ---- the fixture ---------------------------------------------------------------------------------------------------
def pack_fixture(results):
    """{case name: {field: array}} -> dict(data=one f64 vector, index=json) (one zip member instead of thousands)."""
    index, chunks, offset = {}, [], 0
    for name, fields in results.items():
        index[name] = {}
        for key, arr in fields.items():
            arr = np.asarray(arr, dtype=np.float64)
            index[name][key] = [offset, list(arr.shape)]
            chunks.append(arr.reshape(-1))
            offset += arr.size
    return dict(data=np.concatenate(chunks), index=np.array(json.dumps(index)))


@functools.lru_cache(maxsize=None)
def load_fixture():
    """-> {case name: {field: read-only f64 array, leading axis = realization}}."""
    z = np.load(GOLDEN, allow_pickle=False)
    data, index = z["data"], json.loads(str(z["index"]))
    out = {}
    for name, fields in index.items():
        out[name] = {}
        for key, (offset, shape) in fields.items():
            a = data[offset:offset + int(np.prod(shape, dtype=np.int64))].reshape(shape)
            a.setflags(write=False)
            out[name][key] = a
    return out


def case_fields(case):
    """Everything the fixture keeps of one case: per realization the mp results, e_np, kappa and the margins."""
    rows = []
    for r in range(case["n_real"]):
        big_H, F_init = draw(case, r)
        res = run_case(case, r)
        res["kappa"] = sensitivity(case, r, res) / PERTURBATION
        if case["kind"] != "slack":
            res["e_np"] = errors(numpy_solve(case, big_H, F_init), res)
        rows.append(res)
    fields = {}
    for key in rows[0]:
        vals = [row[key] for row in rows]
        if key in ("PF", "PU"):
            vals = [herm_pack(v) for v in vals]
        if key == "every_capacity" or case["kind"] != "slack" or key in ("kappa", "margins", "cost"):
            fields[key] = np.stack([np.asarray(v, dtype=np.float64) for v in vals])
    return fields


def is_strict(fx):
    """The strict condition on one case of the fixture."""
    return bool(np.all(fx["kappa"] * PERTURBATION <= STRICT_SENSITIVITY) and np.all(fx["margins"][:, :4] >= STRICT_MARGIN))


def iterations_pinned(fx):
    """Is the iteration count decided by more than rounding noise?  (rel = 0: the last `dmax > 0` of every realization)"""
    return bool(np.all(fx["margins"][:, 4] >= STRICT_MARGIN))


def bounds(case, fixture_case):
    """The strict bound per quantity: 16 x max(e_np, kappa x 2^-52) at the case's worst realization."""
    return 16.0 * np.maximum(fixture_case["e_np"], fixture_case["kappa"] * EPS).max(axis=0)
