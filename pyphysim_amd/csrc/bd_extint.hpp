// bd_extint.hpp -- the per-lane block-diagonalisation arithmetic shared by the operator kernels of kernels_bd.hip and the
// fused CoMP pipeline with external interference (pipeline_comp.hip): the LQ / Jacobi solve (bd_solve), the zero-forcing
// receive filter, water-filling, and the WhiteningBD / EnhancedBD body (bd_extint_lane) that k_bd_extint and
// k_comp_solve_links both call.  One lane per channel realization, f64.  References: kernels_bd.hip's header.
#pragma once
#include "common.hpp"

namespace mcle {

using cd = double2;
constexpr int kBdMaxN = 8;                      // total antennas per side
constexpr int kBdMaxR = 4;                      // antennas per user
constexpr int kWfMaxN = 64;

__device__ __forceinline__ double bd_abs2(cd z) { return z.x * z.x + z.y * z.y; }

// doWF (waterfilling.py:15-92).  Channels sorted by descending gain (ascending stable sort reversed, which is
// what np.argsort(...)[::-1] gives for these sizes); the worst channel is dropped until the powers that
// touch its level fit the budget; the remainder is shared equally.  Sums run left to right like Python's sum.
static __device__ __noinline__ void bd_waterfill(const double* gains, int n, double total_power, double nv, double* P,
                                          double* mu) {
    int ord[kWfMaxN];
    for (int i = 0; i < n; ++i) ord[i] = i;
    for (int i = 1; i < n; ++i) {               // insertion sort, ascending, stable
        const int v = ord[i];
        int j = i - 1;
        while (j >= 0 && gains[ord[j]] > gains[v]) {
            ord[j + 1] = ord[j];
            --j;
        }
        ord[j + 1] = v;
    }
    // descending position p <-> ord[n - 1 - p]
    int removed = 0;
    double sum = 0.0, level = 0.0;
    for (;;) {
        const int m = n - removed;
        level = nv / gains[ord[n - m]];         // worst of the remaining channels: descending position m - 1
        sum = 0.0;
        for (int p = 0; p < m; ++p) sum += level - nv / gains[ord[n - 1 - p]];
        if (sum > total_power && removed < n - 1)
            ++removed;
        else
            break;
    }
    const int kept = n - removed;
    const double share = (total_power - sum) / kept;
    for (int i = 0; i < n; ++i) P[i] = 0.0;
    for (int p = 0; p < kept; ++p) P[ord[n - 1 - p]] = share + (level - nv / gains[ord[n - 1 - p]]);
    if (mu) *mu = P[ord[n - 1]] + nv / gains[ord[n - 1]];
}

// One-sided (Hestenes) Jacobi on the columns of A [rows x cols, row-major]: on return the columns are mutually
// orthogonal (A <- A V); V [cols x cols] (may be NULL) accumulates the rotations.
static __device__ __noinline__ void bd_jacobi(cd* A, int rows, int cols, cd* V) {
    if (V)
        for (int i = 0; i < cols; ++i)
            for (int c = 0; c < cols; ++c) V[i * cols + c] = mk<double>(i == c ? 1.0 : 0.0, 0.0);
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < cols - 1; ++p)
            for (int q = p + 1; q < cols; ++q) {
                double alpha = 0, beta = 0;
                cd gam = mk<double>(0, 0);
                for (int i = 0; i < rows; ++i) {
                    alpha += bd_abs2(A[i * cols + p]);
                    beta += bd_abs2(A[i * cols + q]);
                    gam = cadd(gam, cmulc(A[i * cols + q], A[i * cols + p]));     // a_p^H a_q
                }
                const double g = sqrt(bd_abs2(gam));
                const double rel = g / (sqrt(alpha * beta) + 1e-300);
                off = fmax(off, rel);
                // orthogonal to rounding (or a zero column): leave the pair alone
                if (!(rel >= 1e-15) || !(g > 0.0)) continue;
                const cd ph = mk<double>(gam.x / g, -gam.y / g);                  // e^{-j phi}
                const double zeta = (beta - alpha) / (2.0 * g);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                for (int i = 0; i < rows; ++i) {
                    const cd ap = A[i * cols + p], aq = cmul(A[i * cols + q], ph);
                    A[i * cols + p] = csub(cscale(ap, c), cscale(aq, s));
                    A[i * cols + q] = cadd(cscale(ap, s), cscale(aq, c));
                }
                if (V)
                    for (int i = 0; i < cols; ++i) {
                        const cd vp = V[i * cols + p], vq = cmul(V[i * cols + q], ph);
                        V[i * cols + p] = csub(cscale(vp, c), cscale(vq, s));
                        V[i * cols + q] = cadd(cscale(vp, s), cscale(vq, c));
                    }
            }
        if (off < 1e-15) break;
    }
}

// Block diagonalisation of H [n x n row-major], n = K * r.  On return Ms [n x n] is the power-scaled precoder
// and sigma [n] the singular values of the users' equivalent channels (ascending inside each user).
// Q and L are n*n scratch.  Returns false for a numerically singular channel.
static __device__ __noinline__ bool bd_solve(const cd* H, int K, int r, double iPu, double nv, int waterfill, cd* Q, cd* L,
                                      cd* Ms, double* sigma) {
    const int n = K * r;
    bool ok = true;
    // ---- LQ by modified Gram-Schmidt on the rows, orthogonalised twice ----
    for (int i = 0; i < n; ++i) {
        double h2 = 0.0;
        for (int c = 0; c < n; ++c) {
            Q[i * n + c] = H[i * n + c];
            h2 += bd_abs2(H[i * n + c]);
        }
        for (int j = 0; j < n; ++j) L[i * n + j] = mk<double>(0, 0);
        for (int pass = 0; pass < 2; ++pass)
            for (int j = 0; j < i; ++j) {
                cd d = mk<double>(0, 0);
                for (int c = 0; c < n; ++c) d = cadd(d, cmulc(Q[i * n + c], Q[j * n + c]));   // v . conj(q_j)
                for (int c = 0; c < n; ++c) Q[i * n + c] = csub(Q[i * n + c], cmul(d, Q[j * n + c]));
                L[i * n + j] = cadd(L[i * n + j], d);
            }
        double v2 = 0.0;
        for (int c = 0; c < n; ++c) v2 += bd_abs2(Q[i * n + c]);
        if (!(v2 > 1e-26 * h2) || !(h2 > 0.0)) {
            ok = false;
            v2 = 1.0;
        }
        const double nrm = sqrt(v2), inv = 1.0 / nrm;
        L[i * n + i] = mk<double>(nrm, 0.0);
        for (int c = 0; c < n; ++c) Q[i * n + c] = cscale(Q[i * n + c], inv);
    }
    // ---- M = L^-1 in place, column by column ----
    for (int j = 0; j < n; ++j) {
        L[j * n + j] = mk<double>(1.0 / L[j * n + j].x, 0.0);
        for (int i = j + 1; i < n; ++i) {
            cd acc = cmul(L[i * n + j], L[j * n + j]);                 // m = j term: L[i][j] * M[j][j]
            for (int m = j + 1; m < i; ++m) acc = cadd(acc, cmul(L[i * n + m], L[m * n + j]));
            const double inv = -1.0 / L[i * n + i].x;                  // L[i][i] still the original diagonal
            L[i * n + j] = cscale(acc, inv);
        }
    }
    // ---- per user: thin SVD of M_k by one-sided Jacobi, precoder columns Q^H u ----
    for (int k = 0; k < K; ++k) {
        cd A[kBdMaxN * kBdMaxR];               // rows k*r .. n-1 of M's columns k*r .. k*r+r-1 (the rest is zero)
        const int r0 = k * r, rows = n - r0;
        for (int i = 0; i < rows; ++i)
            for (int c = 0; c < r; ++c) A[i * r + c] = (r0 + i >= r0 + c) ? L[(r0 + i) * n + r0 + c] : mk<double>(0, 0);
        bd_jacobi(A, rows, r, nullptr);
        double S[kBdMaxR];
        int col[kBdMaxR];
        for (int c = 0; c < r; ++c) {
            double n2 = 0;
            for (int i = 0; i < rows; ++i) n2 += bd_abs2(A[i * r + c]);
            S[c] = sqrt(n2);
            col[c] = c;
        }
        for (int i = 0; i < r - 1; ++i)                                         // descending S == ascending sigma
            for (int j = i + 1; j < r; ++j)
                if (S[col[j]] > S[col[i]]) {
                    const int t = col[i];
                    col[i] = col[j];
                    col[j] = t;
                }
        for (int jj = 0; jj < r; ++jj) {
            const int c = col[jj];
            const double inv = 1.0 / S[c];
            sigma[r0 + jj] = inv;
            // v = Q^H u, u = A[:, c] / S[c] living on rows r0 ..
            double best = -1.0;
            cd piv = mk<double>(1.0, 0.0);
            for (int m = 0; m < n; ++m) {
                cd v = mk<double>(0, 0);
                for (int i = 0; i < rows; ++i) v = cadd(v, cmulc(A[i * r + c], Q[(r0 + i) * n + m]));  // u_i conj(Q[i][m])
                v = cscale(v, inv);
                Ms[m * n + r0 + jj] = v;
                const double m2 = bd_abs2(v);
                if (m2 > best * (1.0 + 1e-12)) {
                    best = m2;
                    piv = v;
                }
            }
            const double pm = sqrt(bd_abs2(piv));
            const cd rot = mk<double>(piv.x / pm, -piv.y / pm);
            for (int m = 0; m < n; ++m) Ms[m * n + r0 + jj] = cmul(Ms[m * n + r0 + jj], rot);
        }
    }
    // ---- power scaling ----
    if (waterfill) {
        double gains[kBdMaxN], P[kBdMaxN];
        for (int j = 0; j < n; ++j) gains[j] = sigma[j] * sigma[j];
        bd_waterfill(gains, n, K * iPu, nv, P, nullptr);
        double worst = 0.0;
        for (int k = 0; k < K; ++k) {
            double f2 = 0.0;
            for (int j = k * r; j < (k + 1) * r; ++j) {
                const double a = sqrt(P[j]);
                for (int m = 0; m < n; ++m) {
                    Ms[m * n + j] = cscale(Ms[m * n + j], a);
                    f2 += bd_abs2(Ms[m * n + j]);
                }
            }
            worst = fmax(worst, sqrt(f2));
        }
        const double scale = sqrt(iPu) / worst;
        for (int e = 0; e < n * n; ++e) Ms[e] = cscale(Ms[e], scale);
    } else {
        for (int k = 0; k < K; ++k) {
            double f2 = 0.0;
            for (int j = k * r; j < (k + 1) * r; ++j)
                for (int m = 0; m < n; ++m) f2 += bd_abs2(Ms[m * n + j]);
            const double scale = sqrt(iPu) / sqrt(f2);
            for (int j = k * r; j < (k + 1) * r; ++j)
                for (int m = 0; m < n; ++m) Ms[m * n + j] = cscale(Ms[m * n + j], scale);
        }
    }
    return ok;
}

// W = pinv(H Ms) [n x n, block diagonal]: row s = conj(newH[block rows, s]) / |.|^2, zero for a zero column.
static __device__ __noinline__ void bd_receive_filter(const cd* H, const cd* Ms, int K, int r, cd* W) {
    const int n = K * r;
    for (int e = 0; e < n * n; ++e) W[e] = mk<double>(0, 0);
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < r; ++j) {
            const int s = k * r + j;
            cd b[kBdMaxR];
            double n2 = 0.0;
            for (int a = 0; a < r; ++a) {
                cd acc = mk<double>(0, 0);
                for (int m = 0; m < n; ++m) acc = cadd(acc, cmul(H[(k * r + a) * n + m], Ms[m * n + s]));
                b[a] = acc;
                n2 += bd_abs2(acc);
            }
            if (n2 > 0.0)
                for (int a = 0; a < r; ++a) W[s * n + k * r + a] = mk<double>(b[a].x / n2, -b[a].y / n2);
        }
}

// ---- block diagonalisation with external interference (blockdiagonalization.py:666-1469) --------------------------
// BDWithExtIntBase.calc_whitening_matrices :690-720, WhiteningBD :722-836, EnhancedBD :839-1469;
// channels/multiuser.py:2469-2520 calc_cov_matrix_extint_plus_noise; util/misc.py:1167-1200 calc_whitening_matrix;
// subspace/projections.py:96-130 calcProjectionMatrix.  One lane per channel realization, f64.
struct BdExtParams {
    int K, r, n_ext;        // users, antennas per user (both sides), total antennas of the external interferers
    int method;             // 0: WhiteningBD, 1: EnhancedBD
    int metric;             // EnhancedBD: 0 None, 1 'naive', 2 'fixed', 3 'capacity', 4 report the SINRs of every stream
                            // count (caller-side metrics such as 'effective_throughput'), 5 stream counts given per user
    int num_streams;        // 'naive' / 'fixed'
    int ns_user[4];         // metric 5
    double iPu, nv, pe;
};

// eigen-decomposition of a Hermitian positive semi-definite R [r x r] by one-sided Jacobi on its columns:
// w ascending, eigenvectors in the columns of V (R V = V diag(w)); largest component of each vector real positive
static __device__ __noinline__ void bd_heig_psd(const cd* R, int r, double* w, cd* V) {
    cd A[kBdMaxR * kBdMaxR], Vt[kBdMaxR * kBdMaxR];
    for (int e = 0; e < r * r; ++e) A[e] = R[e];
    bd_jacobi(A, r, r, Vt);
    double val[kBdMaxR];
    int ord[kBdMaxR];
    for (int c = 0; c < r; ++c) {
        double n2 = 0.0;
        for (int i = 0; i < r; ++i) n2 += bd_abs2(A[i * r + c]);
        val[c] = sqrt(n2);
        ord[c] = c;
    }
    for (int i = 0; i < r - 1; ++i)
        for (int j = i + 1; j < r; ++j)
            if (val[ord[j]] < val[ord[i]]) {
                const int t = ord[i];
                ord[i] = ord[j];
                ord[j] = t;
            }
    for (int c = 0; c < r; ++c) {
        w[c] = val[ord[c]];
        double best = -1.0;
        cd piv = mk<double>(1.0, 0.0);
        for (int i = 0; i < r; ++i) {
            const cd v = Vt[i * r + ord[c]];
            if (bd_abs2(v) > best * (1.0 + 1e-12)) {
                best = bd_abs2(v);
                piv = v;
            }
        }
        const double pm = sqrt(bd_abs2(piv));
        const cd rot = mk<double>(piv.x / pm, -piv.y / pm);
        for (int i = 0; i < r; ++i) V[i * r + c] = cmul(Vt[i * r + ord[c]], rot);
    }
}

// out [n x m] = pinv(A [m x n]) (numpy's cut-off); the k_pinv arithmetic as a device function
static __device__ __noinline__ void bd_pinv_small(const cd* Ain, int m, int n, cd* out) {
    cd A[kBdMaxR * kBdMaxR], V[kBdMaxR * kBdMaxR];
    double s2[kBdMaxR];
    for (int e = 0; e < m * n; ++e) A[e] = Ain[e];
    bd_jacobi(A, m, n, V);
    double top = 0.0;
    for (int c = 0; c < n; ++c) {
        double v = 0.0;
        for (int i = 0; i < m; ++i) v += bd_abs2(A[i * n + c]);
        s2[c] = v;
        top = fmax(top, v);
    }
    const double cut = 1e-30 * top;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < m; ++j) {
            cd acc = mk<double>(0, 0);
            for (int c = 0; c < n; ++c)
                if (s2[c] > cut && s2[c] > 0.0) acc = cadd(acc, cscale(cmulc(V[i * n + c], A[j * n + c]), 1.0 / s2[c]));
            out[i * m + j] = acc;
        }
}

// log2(1 + SINR): the 'capacity' value of a candidate stream (EnhancedBD._calc_capacity)
struct BdValueLog2 {
    __device__ __forceinline__ double operator()(double sinr) const { return log2(1.0 + sinr); }
};

// The per-lane body of WhiteningBD / EnhancedBD on one realization's channel Hb [n][n + n_ext] (row-major, the last n_ext
// columns the interferers' antennas).  emit(k, MsPk [n x ns], W [ns x r], ns) receives every user's result in user order;
// value_of(sinr) is one candidate stream's contribution to the selection value of metrics 3 and 4 (the first maximum over
// the stream counts wins, as np.argmax); cand (may be NULL) [K][r][r]: metric 4 reports row ns-1 = the SINRs with ns streams.
// Returns false for a numerically singular channel.
template <class Emit, class Value>
__device__ __forceinline__ bool bd_extint_lane(const BdExtParams& pp, const cd* Hb, Emit&& emit, Value&& value_of,
                                               double* cand) {
    const int K = pp.K, r = pp.r, n = K * r, cols = n + pp.n_ext;
    cd H[kBdMaxN * kBdMaxN], Q[kBdMaxN * kBdMaxN], L[kBdMaxN * kBdMaxN], Ms[kBdMaxN * kBdMaxN];
    double sigma[kBdMaxN];
    bool ok = true;
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < n; ++c) H[i * n + c] = Hb[(size_t)i * cols + c];
    auto cov = [&](int k, cd* Re) {       // Re_k = pe H_ext,k H_ext,k^H + nv I
        for (int i = 0; i < r; ++i)
            for (int j = 0; j < r; ++j) {
                cd acc = mk<double>(0, 0);
                for (int e = 0; e < pp.n_ext; ++e)
                    acc = cadd(acc, cmulc(Hb[(size_t)(k * r + i) * cols + n + e], Hb[(size_t)(k * r + j) * cols + n + e]));
                acc = cscale(acc, pp.pe);
                if (i == j) acc.x += pp.nv;
                Re[i * r + j] = acc;
            }
    };
    // W [r x r] = pinv(G_k MsPk), G_k = rows of user k of G [n x n].  The columns of G_k MsPk are orthogonal only up to
    // eps |G_k| |MsPk|, which against a small column is eps cond^2: the conjugate-transpose shortcut of bd_receive_filter
    // left W G_k MsPk = I off by that much (0.5 at cond 1e8), so the block goes through the Jacobi pseudo-inverse, which
    // loses one power of the condition number as numpy.linalg.pinv does.
    auto own_block_pinv = [&](const cd* G, int k, const cd* MsPk, cd* W) {
        cd E[kBdMaxR * kBdMaxR];
        for (int i = 0; i < r; ++i)
            for (int c = 0; c < r; ++c) {
                cd acc = mk<double>(0, 0);
                for (int m = 0; m < n; ++m) acc = cadd(acc, cmul(G[(k * r + i) * n + m], MsPk[m * r + c]));
                E[i * r + c] = acc;
            }
        bd_pinv_small(E, r, r, W);
    };
    if (pp.method == 0) {
        // WhiteningBD: whiten every user's rows with W_k^H = diag(L^-1/2) V^H of eig(Re_k), block-diagonalise the
        // whitened channel, receive filter = pinv(newH) x whitening filter (:781-836)
        cd Wf[4][kBdMaxR * kBdMaxR];
        cd Heq[kBdMaxN * kBdMaxN];
        for (int k = 0; k < K; ++k) {
            cd Re[kBdMaxR * kBdMaxR], V[kBdMaxR * kBdMaxR];
            double w[kBdMaxR];
            cov(k, Re);
            bd_heig_psd(Re, r, w, V);
            // Re_k is numerically singular when an eigenvalue is <= 2^-42 of the largest (w ascends): Jacobi returns
            // about 1e-17 w_max, not 0, for a rank-deficient covariance, and 1 / sqrt of that means nothing.  Relative,
            // so big_H times a power of two flags the same lanes (mcle_blast_filter's rule and tolerance).
            const double floor_w = 0x1p-42 * w[r - 1];
            for (int i = 0; i < r; ++i) {
                const bool pos = w[i] > floor_w && w[i] > 0.0;
                ok = ok && pos;
                const double s = 1.0 / sqrt(pos ? w[i] : 1.0);
                for (int j = 0; j < r; ++j) Wf[k][i * r + j] = cscale(cconj(V[j * r + i]), s);
            }
            for (int i = 0; i < r; ++i)
                for (int c = 0; c < n; ++c) {
                    cd acc = mk<double>(0, 0);
                    for (int j = 0; j < r; ++j) acc = cadd(acc, cmul(Wf[k][i * r + j], H[(k * r + j) * n + c]));
                    Heq[(k * r + i) * n + c] = acc;
                }
        }
        ok = bd_solve(Heq, K, r, pp.iPu, pp.nv, 0, Q, L, Ms, sigma) && ok;
        for (int k = 0; k < K; ++k) {
            cd MsPk[kBdMaxN * kBdMaxR], W[kBdMaxR * kBdMaxR], Pi[kBdMaxR * kBdMaxR];
            for (int m = 0; m < n; ++m)
                for (int c = 0; c < r; ++c) MsPk[m * r + c] = Ms[m * n + k * r + c];
            own_block_pinv(Heq, k, MsPk, Pi);                // pinv(newH)'s block of user k
            for (int i = 0; i < r; ++i)
                for (int c = 0; c < r; ++c) {
                    cd acc = mk<double>(0, 0);
                    for (int j = 0; j < r; ++j) acc = cadd(acc, cmul(Pi[i * r + j], Wf[k][j * r + c]));
                    W[i * r + c] = acc;
                }
            emit(k, MsPk, W, r);
        }
    } else if (pp.metric == 0) {
        // EnhancedBD without a metric: plain BD, every user inverts its own block (:1140-1195)
        ok = bd_solve(H, K, r, pp.iPu, pp.nv, 0, Q, L, Ms, sigma);
        for (int k = 0; k < K; ++k) {
            cd MsPk[kBdMaxN * kBdMaxR], W[kBdMaxR * kBdMaxR];
            for (int m = 0; m < n; ++m)
                for (int c = 0; c < r; ++c) MsPk[m * r + c] = Ms[m * n + k * r + c];
            own_block_pinv(H, k, MsPk, W);
            emit(k, MsPk, W, r);
        }
    } else {
        // EnhancedBD with stream reduction (:1197-1411): unit-norm BD directions Ms_bad, then per user a reduction
        // matrix Pk onto the directions least hit by the external interference, power renormalised, receive filter
        // pinv(Pbar Heq_red) Pbar with Pbar the projector onto span(Pk)
        ok = bd_solve(H, K, r, (double)r, pp.nv, 0, Q, L, Ms, sigma);
        for (int k = 0; k < K; ++k) {
            cd Re[kBdMaxR * kBdMaxR], V[kBdMaxR * kBdMaxR], Heq[kBdMaxR * kBdMaxR];
            double w[kBdMaxR];
            cov(k, Re);
            bd_heig_psd(Re, r, w, V);                        // ascending: column 0 = least interfered direction
            for (int i = 0; i < r; ++i)
                for (int c = 0; c < r; ++c) {
                    cd acc = mk<double>(0, 0);
                    for (int m = 0; m < n; ++m) acc = cadd(acc, cmul(H[(k * r + i) * n + m], Ms[m * n + k * r + c]));
                    Heq[i * r + c] = acc;
                }
            int lo = 1, hi = r;
            if (pp.metric == 1 || pp.metric == 2) lo = hi = pp.num_streams;
            if (pp.metric == 5) lo = hi = pp.ns_user[k];
            double best_val = -1e300;
            int best_ns = 0;
            cd best_Ms[kBdMaxN * kBdMaxR], best_W[kBdMaxR * kBdMaxR];
            for (int ns = lo; ns <= hi; ++ns) {
                cd Pk[kBdMaxR * kBdMaxR];                    // r x ns
                const bool identity = pp.metric == 1 || (pp.metric != 2 && ns == r);
                for (int i = 0; i < r; ++i)
                    for (int c = 0; c < ns; ++c)
                        Pk[i * ns + c] = identity ? mk<double>(i == c ? 1.0 : 0.0, 0.0) : V[i * r + c];
                cd MsPk[kBdMaxN * kBdMaxR];
                double f2 = 0.0;
                for (int m = 0; m < n; ++m)
                    for (int c = 0; c < ns; ++c) {
                        cd acc = mk<double>(0, 0);
                        for (int j = 0; j < r; ++j) acc = cadd(acc, cmul(Ms[m * n + k * r + j], Pk[j * ns + c]));
                        MsPk[m * ns + c] = acc;
                        f2 += bd_abs2(acc);
                    }
                const double inv_norm = sqrt(pp.iPu) / sqrt(f2);
                for (int e = 0; e < n * ns; ++e) MsPk[e] = cscale(MsPk[e], inv_norm);
                cd Hred[kBdMaxR * kBdMaxR], Pbar[kBdMaxR * kBdMaxR], PH[kBdMaxR * kBdMaxR], Pi[kBdMaxR * kBdMaxR];
                for (int i = 0; i < r; ++i)
                    for (int c = 0; c < ns; ++c) {
                        cd acc = mk<double>(0, 0);
                        for (int j = 0; j < r; ++j) acc = cadd(acc, cmul(Heq[i * r + j], Pk[j * ns + c]));
                        Hred[i * ns + c] = cscale(acc, inv_norm);
                    }
                for (int i = 0; i < r; ++i)                  // Pk has orthonormal columns: Pbar = Pk Pk^H
                    for (int j = 0; j < r; ++j) {
                        cd acc = mk<double>(0, 0);
                        for (int c = 0; c < ns; ++c) acc = cadd(acc, cmulc(Pk[i * ns + c], Pk[j * ns + c]));
                        Pbar[i * r + j] = acc;
                    }
                for (int i = 0; i < r; ++i)
                    for (int c = 0; c < ns; ++c) {
                        cd acc = mk<double>(0, 0);
                        for (int j = 0; j < r; ++j) acc = cadd(acc, cmul(Pbar[i * r + j], Hred[j * ns + c]));
                        PH[i * ns + c] = acc;
                    }
                bd_pinv_small(PH, r, ns, Pi);                // ns x r
                cd W[kBdMaxR * kBdMaxR];
                for (int i = 0; i < ns; ++i)
                    for (int c = 0; c < r; ++c) {
                        cd acc = mk<double>(0, 0);
                        for (int j = 0; j < r; ++j) acc = cadd(acc, cmul(Pi[i * r + j], Pbar[j * r + c]));
                        W[i * r + c] = acc;
                    }
                double value = 0.0;
                if (pp.metric == 3 || pp.metric == 4) {      // EnhancedBD._calc_linear_SINRs (:1101-1138)
                    for (int i = 0; i < ns; ++i) {
                        double desired = 0.0, internal = 0.0;
                        for (int c = 0; c < ns; ++c) {
                            cd acc = mk<double>(0, 0);
                            for (int j = 0; j < r; ++j) acc = cadd(acc, cmul(W[i * r + j], Hred[j * ns + c]));
                            if (c == i) desired = bd_abs2(acc);
                            else internal += bd_abs2(acc);
                        }
                        double ext = 0.0;
                        for (int p = 0; p < r; ++p)
                            for (int q = 0; q < r; ++q) ext += cmul(cmul(W[i * r + p], Re[p * r + q]), cconj(W[i * r + q])).x;
                        const double sinr = desired / (internal + fabs(ext));
                        value += value_of(sinr);
                        if (cand && pp.metric == 4) cand[(k * r + (ns - 1)) * r + i] = sinr;
                    }
                }
                if (ns == lo || value > best_val) {          // np.argmax: the first maximum
                    best_val = value;
                    best_ns = ns;
                    for (int e = 0; e < n * ns; ++e) best_Ms[e] = MsPk[e];
                    for (int e = 0; e < ns * r; ++e) best_W[e] = W[e];
                }
            }
            emit(k, best_Ms, best_W, best_ns);
        }
    }
    return ok;
}

}  // namespace mcle
