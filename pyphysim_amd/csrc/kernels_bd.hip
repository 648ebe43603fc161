// kernels_bd.hip -- block diagonalisation of a multi-user MIMO downlink, water-filling, and the fused
// CoMP pipeline built on them.
//
// Reference: comm/waterfilling.py:15-92 (doWF); comm/blockdiagonalization.py:272-363
// (_calc_BD_matrix_no_power_scaling), :365-464 (global / normalised water-filling power scaling), :466-508
// (block_diagonalize), :510-566 (block_diagonalize_no_waterfilling), :568-585 (calc_receive_filter);
// channels/multiuser.py:256-292 (path loss), :1179-1221 (corrupt_concatenated_data);
// apps/comp_BD/simulate_comp_simple.py:95-140 (the application).
//
// The reference takes two SVDs per user (null space of the other users' rows, then the equivalent
// channel).  For the square case (as many transmit as receive antennas -- the only one in which the
// reference's stream count, blockdiagonalization.py:332, equals the null-space dimension) the same
// precoder follows from ONE LQ factorisation H = L Q shared by all users:
//     H^-1 = Q^H M,  M = L^-1 (lower triangular);   Z_k = Q^H M_k  (columns of user k)
//     Z_k^H Z_k = M_k^H M_k = [(H H^H)^-1]_kk = (H_k P0_k H_k^H)^-1      (Schur complement)
// so with the thin SVD M_k = U S V^H (one-sided Jacobi on r <= 4 columns) the right singular vectors of
// the equivalent channel H_k V0_k are Q^H U and its singular values 1 / S.  Singular vectors are
// unique up to a phase per column; the largest entry of every precoder column is made real positive
// (oracle/bd.py: canonical_columns).  newH = H Ms has orthogonal columns inside each user's block, so
// pinv(newH) is its scaled conjugate transpose, with zero rows for streams the water-filling switched off
// (what numpy's pinv returns for a zero column).
#include "modem.hpp"
#include "philox.hpp"
#include "pkcx.hpp"
#include "pipe_common.hpp"
#include "totals.hpp"
#include "wave_draws.hpp"
#include "walk_f64.hpp"
#include "link_walk.hpp"
#include "bd_static.hpp"
#include "bd_extint.hpp"

namespace mcle {

__global__ __launch_bounds__(64) void k_waterfilling(const double* __restrict__ gains, int n, double total_power,
                                                     double nv, double* __restrict__ P, double* __restrict__ mu,
                                                     size_t batch) {
    for (size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x; b < batch; b += (size_t)gridDim.x * blockDim.x) {
        double g[kWfMaxN], p[kWfMaxN], level;
        for (int i = 0; i < n; ++i) g[i] = gains[b * n + i];
        bd_waterfill(g, n, total_power, nv, p, &level);
        for (int i = 0; i < n; ++i) P[b * n + i] = p[i];
        if (mu) mu[b] = level;
    }
}

__global__ __launch_bounds__(64) void k_block_diagonalize(const cd* __restrict__ Hin, int K, int r, double iPu, double nv,
                                                          int waterfill, cd* __restrict__ Ms_out,
                                                          cd* __restrict__ newH_out, cd* __restrict__ W_out,
                                                          double* __restrict__ sigma_out,
                                                          uint32_t* __restrict__ skipped, size_t batch) {
    const int n = K * r, nn = n * n;
    for (size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x; b < batch; b += (size_t)gridDim.x * blockDim.x) {
        cd H[kBdMaxN * kBdMaxN], Q[kBdMaxN * kBdMaxN], L[kBdMaxN * kBdMaxN], Ms[kBdMaxN * kBdMaxN];
        double sigma[kBdMaxN];
        for (int e = 0; e < nn; ++e) H[e] = Hin[b * nn + e];
        const bool ok = bd_solve(H, K, r, iPu, nv, waterfill, Q, L, Ms, sigma);
        if (Ms_out)
            for (int e = 0; e < nn; ++e) Ms_out[b * nn + e] = Ms[e];
        if (newH_out)
            for (int i = 0; i < n; ++i)
                for (int c = 0; c < n; ++c) {
                    cd acc = mk<double>(0, 0);
                    for (int m = 0; m < n; ++m) acc = cadd(acc, cmul(H[i * n + m], Ms[m * n + c]));
                    newH_out[b * nn + i * n + c] = acc;
                }
        if (W_out) {
            bd_receive_filter(H, Ms, K, r, Q);              // Q is free again
            for (int e = 0; e < nn; ++e) W_out[b * nn + e] = Q[e];
        }
        if (sigma_out)
            for (int j = 0; j < n; ++j) sigma_out[b * n + j] = sigma[j];
        if (skipped) skipped[b] = ok ? 0u : 1u;
    }
}

// np.linalg.pinv for small matrices: A [m x n] -> [n x m] = V diag(1/s) U^H over the singular values above
// rcond * max(s) (numpy's default cut-off 1e-15).  With A V = U S from the column Jacobi: pinv = V S^-2 (A V)^H.
__global__ __launch_bounds__(64) void k_pinv(const cd* __restrict__ Ain, int m, int n, double rcond,
                                             cd* __restrict__ out, size_t batch) {
    for (size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x; b < batch; b += (size_t)gridDim.x * blockDim.x) {
        cd A[kBdMaxN * kBdMaxN], V[kBdMaxN * kBdMaxN];
        double s2[kBdMaxN];
        for (int e = 0; e < m * n; ++e) A[e] = Ain[b * m * n + e];
        bd_jacobi(A, m, n, V);
        double top = 0.0;
        for (int c = 0; c < n; ++c) {
            double v = 0.0;
            for (int i = 0; i < m; ++i) v += bd_abs2(A[i * n + c]);
            s2[c] = v;
            top = fmax(top, v);
        }
        const double cut = rcond * rcond * top;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < m; ++j) {
                cd acc = mk<double>(0, 0);
                for (int c = 0; c < n; ++c)
                    if (s2[c] > cut && s2[c] > 0.0) acc = cadd(acc, cscale(cmulc(V[i * n + c], A[j * n + c]), 1.0 / s2[c]));
                out[b * n * m + i * m + j] = acc;
            }
    }
}

// Outputs per realization b and user k, zero padded: Ms [b][K][n][r] (the user's precoder MsPk: n x Ns),
// W [b][K][r][r] (receive filter, Ns x r), Ns [b][K], cand [b][K][r][r] (metric 4: row ns-1 = the SINRs with ns streams)
__global__ __launch_bounds__(64) void k_bd_extint(BdExtParams pp, const cd* __restrict__ bigH, cd* __restrict__ Ms_out,
                                                  cd* __restrict__ W_out, int32_t* __restrict__ ns_out,
                                                  double* __restrict__ cand_out, uint32_t* __restrict__ skipped,
                                                  size_t batch) {
    const int K = pp.K, r = pp.r, n = K * r, cols = n + pp.n_ext;
    for (size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x; b < batch; b += (size_t)gridDim.x * blockDim.x) {
        auto emit = [&](int k, const cd* MsPk, const cd* W, int ns) {     // MsPk [n x ns], W [ns x r]
            cd* mo = Ms_out + ((b * K + k) * (size_t)n) * r;
            cd* wo = W_out + ((b * K + k) * (size_t)r) * r;
            for (int m = 0; m < n; ++m)
                for (int c = 0; c < r; ++c) mo[m * r + c] = c < ns ? MsPk[m * ns + c] : mk<double>(0, 0);
            for (int i = 0; i < r; ++i)
                for (int c = 0; c < r; ++c) wo[i * r + c] = i < ns ? W[i * r + c] : mk<double>(0, 0);
            if (ns_out) ns_out[b * K + k] = ns;
        };
        const bool ok = bd_extint_lane(pp, bigH + b * (size_t)n * cols, emit, BdValueLog2(),
                                       cand_out ? cand_out + b * (size_t)K * r * r : nullptr);
        if (skipped) skipped[b] = ok ? 0u : 1u;
    }
}

struct BdParams {
    int K, r, n_symbols, waterfill, has_pathloss;
    double iPu, noise_var, bd_noise_var;
    double root_pl[16];
};

// Fused CoMP application: one wavefront per chunk of 64 realizations (as k_run_ia).  Phase 1: lane i draws the
// channel of realization i, block-diagonalises it in f64 and parks the receive side of the link in LDS: the
// user's block of W = pinv(H Ms) for each stream (R entries) and d_s = (W H Ms)_ss -- 1 on an active stream
// up to rounding, 0 on a stream the water-filling switched off.  The off-diagonal entries of W H Ms are the
// rounding residue of an exact block diagonalisation (<= 1e-15 |d|) and are not carried.  Phase 2: the wave runs
// the realization's symbol columns: est_s = d_s x_s + W_s . (sigma n_user), demodulate, count.
// R = antennas per user (compile time: every register index below is static).
// Two launches since round 2 (the same split as the IA pipeline, kernels_ia.hip): the per-lane solve keeps four n x n
// complex f64 work matrices in scratch and takes every register (one wave per SIMD), the symbol walk is light and wants
// many resident waves.  The record between them: d[n], W[n][R], flag.
template <typename T, int R>
__global__ __launch_bounds__(64) void k_bd_solve_links(BdParams pp, uint64_t seed, uint64_t first, uint64_t count,
                                                       cx<T>* __restrict__ recs) {
    const uint64_t rl = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (rl >= count) return;
    const int K = pp.K, n = K * R;
    const int stride = n * (R + 1) + 1;
    const Rng rng(seed, first + rl);
    cd H[kBdMaxN * kBdMaxN], Q[kBdMaxN * kBdMaxN], L[kBdMaxN * kBdMaxN], Ms[kBdMaxN * kBdMaxN];
    double sg[kBdMaxN];
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < n; ++c) {
            cd h = cn_sample<double>(rng, STREAM_CHAN, (uint64_t)(i * n + c), 1.0);
            if (pp.has_pathloss) h = cscale(h, pp.root_pl[(i / R) * K + c / R]);
            H[i * n + c] = h;
        }
    const bool ok = bd_solve(H, K, R, pp.iPu, pp.bd_noise_var, pp.waterfill, Q, L, Ms, sg);
    bd_receive_filter(H, Ms, K, R, Q);               // W in Q
    cx<T>* rec = recs + rl * stride;
    for (int s = 0; s < n; ++s) {
        const int r0 = (s / R) * R;
        cd d = mk<double>(0, 0);                     // (W H Ms)_ss
        for (int a = 0; a < R; ++a) {
            cd hm = mk<double>(0, 0);
            for (int m = 0; m < n; ++m) hm = cadd(hm, cmul(H[(r0 + a) * n + m], Ms[m * n + s]));
            d = cadd(d, cmul(Q[s * n + r0 + a], hm));
            rec[n + s * R + a] = mk<T>((T)Q[s * n + r0 + a].x, (T)Q[s * n + r0 + a].y);
        }
        rec[s] = mk<T>((T)d.x, (T)d.y);
    }
    rec[n * (R + 1)] = mk<T>(ok ? (T)1 : (T)0, (T)0);
}

// The same record from the compile-time-sized solve of bd_static.hpp (K R <= 6): every matrix in registers, no scratch.
template <typename T, int K, int R>
__global__ __launch_bounds__(64) void k_bd_solve_links_static(BdParams pp, uint64_t seed, uint64_t first, uint64_t count,
                                                              cx<T>* __restrict__ recs) {
    constexpr int n = K * R, stride = n * (R + 1) + 1;
    const uint64_t rl = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (rl >= count) return;
    const Rng rng(seed, first + rl);
    cd Q[n][n];
#pragma unroll
    for (int i = 0; i < n; ++i)
#pragma unroll
        for (int c = 0; c < n; ++c) {
            cd h = cn_sample<double>(rng, STREAM_CHAN, (uint64_t)(i * n + c), 1.0);
            if (pp.has_pathloss) h = cscale(h, pp.root_pl[(i / R) * K + c / R]);
            Q[i][c] = h;
        }
    cd d[n], Wb[n][R];
    const bool ok = bd_solve_link_static<K, R>(Q, pp.iPu, pp.bd_noise_var, pp.waterfill, d, Wb);
    cx<T>* rec = recs + rl * stride;
#pragma unroll
    for (int s = 0; s < n; ++s) {
        rec[s] = mk<T>((T)d[s].x, (T)d[s].y);
#pragma unroll
        for (int a = 0; a < R; ++a) rec[n + s * R + a] = mk<T>((T)Wb[s][a].x, (T)Wb[s][a].y);
    }
    rec[n * (R + 1)] = mk<T>(ok ? (T)1 : (T)0, (T)0);
}

// Register budget of the walk: four waves per SIMD (128 VGPRs, 45 of them spilled by the lockstep search) measured against
// three (168 VGPRs, nothing spilled) on the round-3 box: 1.266 vs 1.355-1.365 ms per 131 072 realizations -- the fourth
// wave hides more latency than the spills cost; kept at four.
// Round 4: KC = the number of users as a compile-time constant (0: run-time, arrays and loops sized for kBdMaxN) and MODE = the
// demodulator path chosen by the host (0: demod_one per stream -- slicer, certificate, grid or sweep; 1: the R streams of a
// user swept in lockstep, M <= 8; 2: lockstep through the certificate / candidate grid).  With all three paths and
// eight-entry arrays in one body the complex64 form spilled 45-52 registers at its 128-register bound (profiles/r03:
// VALU busy 0.97 on the draw ledger plus spill traffic).
template <typename T, int R, int KC = 0, int MODE = 0>
// (round 6: workgroups of FOUR independent wavefronts, one flush of the counters -- totals.hpp: wg_flush_waves)
__global__ __launch_bounds__(256, (sizeof(T) == 4 || KC) ? 3 : 2) void k_bd_link(ModemParams<T> mp, BdParams pp, uint64_t seed,
                                                                        uint64_t first, uint64_t count, int per_wave,
                                                                        const cx<T>* __restrict__ recs,
                                                                        mcle_counters* counters,
                                                                        uint32_t* __restrict__ sym_out,
                                                                        uint32_t* __restrict__ bit_out) {
    constexpr int KMAX = KC ? KC : kBdMaxN / R, NMAX = KC ? KC * R : kBdMaxN;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int K = KC ? KC : pp.K, n = K * R;
    const int stride = n * (R + 1) + 1;
    unsigned long long* s_grid = reinterpret_cast<unsigned long long*>(smem);
    __shared__ cx<T> s_table[256];
    __shared__ float4 s_tab4[sizeof(T) == 4 ? 256 : 1];     // {re, im, |c|^2 / 2, 0}: the lockstep searches of modem.hpp
    __shared__ WgTotals totals_all[4];
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    WgTotals& totals = totals_all[wv];
    __shared__ double s_bm[sizeof(T) == 8 ? kBmLdsDoubles : 1];   // complex128 Box-Muller tables (bm_f64.hpp)
    link_prologue(mp, s_table, s_tab4, s_grid, s_bm);
    const int lane = threadIdx.x & 63;
    const T sigma = (T)sqrt(pp.noise_var);
    const uint32_t mask = (uint32_t)(mp.M - 1);
    const int NS = pp.n_symbols;
    // f32, min-distance: the R streams of a user searched in lockstep -- directly for constellations of <= 8 points,
    // through the candidate grid otherwise (same decisions as demod_one, one LDS round trip per candidate for all R)
    if (lane == 0) wg_zero(totals);
    __syncthreads();
    const uint64_t n_chunks = (count + per_wave - 1) / per_wave;
    for (uint64_t ch = (uint64_t)blockIdx.x * 4 + wv; ch < n_chunks; ch += (uint64_t)gridDim.x * 4) {
        const uint64_t r_end = (ch + 1) * per_wave < count ? (ch + 1) * per_wave : count;
        for (uint64_t rl = ch * per_wave; rl < r_end; ++rl) {
            const Rng rng(seed, first + rl);
            const cx<T>* D = recs + rl * stride;     // wave-uniform record: scalar loads
            const cx<T>* W = D + n;
            const bool ok = D[n * (R + 1)].x != (T)0;
            unsigned se = 0, be = 0;
            // one symbol column
            auto column = [&](const int (&tx)[NMAX], const cx<T> (&nz)[NMAX]) {
#pragma unroll
                for (int k = 0; k < KMAX; ++k)
                    if (KC || k < K) {
                        cx<T> est[R];
#pragma unroll
                        for (int jj = 0; jj < R; ++jj) {
                            const int s = k * R + jj;
                            if constexpr (sizeof(T) == 4) {          // explicit packed forms (pkcx.hpp): 2 + 2 R instructions
                                pk2 e = pk_cmul(to_pk(D[s]), to_pk(s_table[tx[s]]));
#pragma unroll
                                for (int a = 0; a < R; ++a) e = pk_cfma(to_pk(W[s * R + a]), to_pk(nz[k * R + a]), e);
                                est[jj] = from_pk(e);
                            } else {
                                est[jj] = cmul(D[s], s_table[tx[s]]);
#pragma unroll
                                for (int a = 0; a < R; ++a) est[jj] = cfma4(W[s * R + a], nz[k * R + a], est[jj]);
                            }
                        }
                        int dec[R];
                        if constexpr (sizeof(T) == 4 && MODE == 1) {
                            demod_mindist_multi<R>(s_tab4, mp.M, est, dec);
                        } else if constexpr (sizeof(T) == 4 && MODE == 2) {
                            demod_multi_cert(mp, est, dec, [&](int (&d_)[R]) { demod_grid4_multi<R>(s_tab4, s_grid, mp.grid, mp.M, est, d_); });
                        } else {
#pragma unroll
                            for (int jj = 0; jj < R; ++jj) dec[jj] = demod_one(mp, s_table, s_grid, est[jj]);
                        }
#pragma unroll
                        for (int jj = 0; jj < R; ++jj) {
                            const unsigned x = (unsigned)(tx[k * R + jj] ^ dec[jj]);
                            se += (x != 0u);
                            be += __popc(x);
                        }
                    }
            };
            if ((NS & 1) == 0) {
                // two columns per lane and pass: whole Philox blocks, symbol blocks shared across the wave
                for (int t0 = 0; t0 < NS; t0 += kPairCols) {
                    const int t = t0 + 2 * lane;
                    int ta[NMAX], tb[NMAX];
                    wave_symbol_pairs<NMAX>(rng, n, (uint32_t)NS, (uint32_t)t0, mask, lane, ta, tb);
                    if (t < NS) {
                        if constexpr (sizeof(T) == 8) {
                            // complex128: user by user -- the noise of ONE user's R antennas (both columns), its estimates, its
                            // decisions -- instead of all K R antennas' draws first: 8 R live noise registers instead of 8 K R,
                            // so that the registers can be bounded for three wavefronts per SIMD (round 5; k_ia_link alike)
#pragma unroll
                            for (int k = 0; k < KMAX; ++k)
                                if (KC || k < K) {
                                    cx<T> za[R], zb[R];
#pragma unroll
                                    for (int a = 0; a < R; ++a)
                                        cn_pair_lds(rng, STREAM_NOISE, ((uint32_t)(k * R + a) * (uint32_t)NS + (uint32_t)t) >> 1, sigma,
                                                    za[a], zb[a], s_bm);
#pragma unroll
                                    for (int jj = 0; jj < R; ++jj) {
                                        const int s = k * R + jj;
                                        cx<T> ea = cmul(D[s], s_table[ta[s]]), eb = cmul(D[s], s_table[tb[s]]);
#pragma unroll
                                        for (int a = 0; a < R; ++a) {
                                            ea = cfma4(W[s * R + a], za[a], ea);
                                            eb = cfma4(W[s * R + a], zb[a], eb);
                                        }
                                        const unsigned da = (unsigned)(ta[s] ^ demod_one(mp, s_table, s_grid, ea));
                                        const unsigned db = (unsigned)(tb[s] ^ demod_one(mp, s_table, s_grid, eb));
                                        se += (da != 0u) + (db != 0u);
                                        be += __popc(da) + __popc(db);
                                    }
                                }
                        } else {
                            cx<T> za[NMAX], zb[NMAX];
#pragma unroll
                            for (int a = 0; a < NMAX; ++a)
                                if (KC || a < n)
                                    cn_pair_lds(rng, STREAM_NOISE, ((uint32_t)a * (uint32_t)NS + (uint32_t)t) >> 1, sigma,
                                                za[a], zb[a], s_bm);
                            column(ta, za);
                            column(tb, zb);
                        }
                    }
                }
            } else {
                for (int t = lane; t < NS; t += 64) {
                    int tx[NMAX];
                    cx<T> nz[NMAX];
#pragma unroll
                    for (int a = 0; a < NMAX; ++a)
                        if (KC || a < n) {
                            tx[a] = (int)symbol_at(rng, (uint64_t)a * NS + t, mask);   // randint(0, M, [n, NSymbs])
                            nz[a] = cn_sample<T>(rng, STREAM_NOISE, (uint64_t)a * NS + t, sigma);
                        }
                    column(tx, nz);
                }
            }
            link_account(totals, se, be, !ok, rl, lane, sym_out, bit_out);
        }
    }
    wg_flush_waves<4>(totals_all, counters, (unsigned long long)n * NS, (unsigned long long)n * NS * mp.bits);
}

template <typename T, int R>
static int launch_run_bd(mcle_ctx* ctx, const mcle_bd_cfg* cfg, const BdParams& pp, uint64_t seed, uint64_t first,
                         uint64_t count, mcle_counters* d_counters, uint32_t* d_sym_err, uint32_t* d_bit_err) {
    const int n = cfg->K * R;
    const ModemParams<T> mp = pipe_modem<T>(ctx, cfg->demod_method);
    const uint64_t kSlice = 1ull << 20;          // realizations per solve + walk pair: bounds the record buffer
    const size_t stride = (size_t)(n * (R + 1) + 1);
    const size_t lds = (size_t)mp.grid.G * mp.grid.G * sizeof(unsigned long long);
    const int per_wave = 8;
    // (complex128: three wavefronts per SIMD where the user count is a compile-time constant -- 168 registers, nothing spilled --
    //  two for the run-time-sized form, which spills 18 - 58 registers at that bound)
    const bool kc = R <= 2 && (cfg->K == 2 || cfg->K == 3) && cfg->K * R <= kBdMaxN;
    // demodulator path of the walk (compile-time in the kernel): complex64 min-distance in lockstep -- a sweep for M <= 8,
    // certificate / candidate grid otherwise; everything else one demod_one per stream
    // (round 5: a constellation WITH a certificate -- square QAM, QPSK -- goes through it whatever its size: the application's
    //  own 4-PSK was swept point by point in lockstep, ~20 instructions per decision where the quadrant certificate takes 6)
    const int mode = (sizeof(T) == 4 && mp.method == MCLE_DEMOD_MINDIST)
                         ? ((mp.cert && mp.grid.G > 0) ? 2 : (mp.M <= 8 ? 1 : (mp.grid.G > 0 ? 2 : 0))) : 0;
    return launch_sliced(
        ctx, first, count, kSlice, stride * sizeof(cx<T>), d_sym_err, d_bit_err,
        [&](void* recs, uint64_t at, uint64_t m) {
            const dim3 sgrid((unsigned)((m + 63) / 64));
#define MCLE_BD_STATIC(K_)                                                                                                \
    if (cfg->K == K_ && K_ * R <= 6) {                                                                                    \
        hipLaunchKernelGGL((k_bd_solve_links_static<T, K_, (K_ * R <= 6 ? R : 1)>), sgrid, dim3(64), 0, ctx->stream, pp, seed,  \
                           at, m, (cx<T>*)recs);                                                                          \
        return;                                                                                                           \
    }
            if (!ctx->opt[MCLE_OPT_BD_RUNTIME_SOLVE]) {       // compile-time-sized solve (registers) where n = K R <= 6
                MCLE_BD_STATIC(2) MCLE_BD_STATIC(3) MCLE_BD_STATIC(4) MCLE_BD_STATIC(5) MCLE_BD_STATIC(6)
            }
#undef MCLE_BD_STATIC
            hipLaunchKernelGGL((k_bd_solve_links<T, R>), sgrid, dim3(64), 0, ctx->stream, pp, seed, at, m, (cx<T>*)recs);
        },
        [&](void* recs, uint64_t at, uint64_t m, uint32_t* sym, uint32_t* bit) {
            if constexpr (R <= 2) {
                // two or three users, an even number of columns >= 128: the packed walk of walk_f64.hpp (round 6; complex64 since its last day)
                if (kc && link_walk_f64_fits(cfg->n_symbols) && !ctx->opt[MCLE_OPT_WALK_LEGACY]) {
#define MCLE_BD_PACKED(KC_, ABL_)                                                                                             \
    if (cfg->K == KC_) {                                                                                                      \
        launch_link_walk<T, BdWalk<KC_, R>, ABL_>(ctx, mp, cfg->n_symbols, pp.noise_var, seed, at, m, (const cx<T>*)recs,     \
                                                   d_counters, sym, bit);                                                    \
        return;                                                                                                               \
    }
#ifdef MCLE_EXPERIMENTS
                    if constexpr (R == 2 && sizeof(T) == 8) {
                        switch ((int)ctx->opt[MCLE_OPT_F64_VARIANT]) {
                            case 1: MCLE_BD_PACKED(3, 1) break;
                            case 2: MCLE_BD_PACKED(3, 2) break;
                            case 4: MCLE_BD_PACKED(3, 4) break;
                            case 6: MCLE_BD_PACKED(3, 6) break;
                            case 8: MCLE_BD_PACKED(3, 8) break;
                            case 16: MCLE_BD_PACKED(3, 16) break;
                            case 31: MCLE_BD_PACKED(3, 31) break;
                            default: break;
                        }
                    }
#endif
                    MCLE_BD_PACKED(2, 0) MCLE_BD_PACKED(3, 0)
#undef MCLE_BD_PACKED
                }
            }
            // the resident set: the wavefronts per SIMD of k_bd_link's __launch_bounds__ (3 for complex64 and the compile-time user
            // counts, 2 otherwise) -- rounds 4-5 sized the complex64 grid for four and ran a partial second wave of workgroups
            // (a chunk is 8-16 realizations; one chunk per workgroup measured 1.5 x slower)
            const unsigned grid = walk_grid(ctx, (sizeof(T) == 4 || kc) ? 3 : 2, m, per_wave, 2);
#define MCLE_BD_WALK(KC_, MODE_)                                                                                          \
    if ((KC_ == 0 || (cfg->K == KC_ && KC_ * R <= kBdMaxN)) && mode == MODE_) {                                             \
        hipLaunchKernelGGL((k_bd_link<T, R, (KC_ * R <= kBdMaxN ? KC_ : 0), (sizeof(T) == 4 ? MODE_ : 0)>), dim3(grid), dim3(256), lds, \
                           ctx->stream, mp, pp, seed, at, m, per_wave, (const cx<T>*)recs, d_counters, sym, bit);          \
        return;                                                                                                           \
    }
            if constexpr (R <= 2) {                    // users as a compile-time count where the arrays then shrink: K = 2, 3
                MCLE_BD_WALK(2, 0) MCLE_BD_WALK(2, 1) MCLE_BD_WALK(2, 2) MCLE_BD_WALK(3, 0) MCLE_BD_WALK(3, 1) MCLE_BD_WALK(3, 2)
            }
            MCLE_BD_WALK(0, 0) MCLE_BD_WALK(0, 1) MCLE_BD_WALK(0, 2)
#undef MCLE_BD_WALK
        });
}

static int check_bd_dims(int K, int r) {
    MCLE_REQUIRE(K >= 1 && r >= 1 && r <= kBdMaxR && K * r <= kBdMaxN,
                 "block diagonalisation supports num_users * antennas <= %d with at most %d antennas per user "
                 "(got %d users x %d)", kBdMaxN, kBdMaxR, K, r);
    return MCLE_OK;
}

}  // namespace mcle

using namespace mcle;

extern "C" {

int mcle_waterfilling(mcle_ctx* ctx, const double* d_gains, int n, double total_power, double noise_var,
                      double* d_powers, double* d_mu, size_t batch) {
    MCLE_REQUIRE(ctx != nullptr && (batch == 0 || (d_gains != nullptr && d_powers != nullptr)), "null argument");
    MCLE_REQUIRE(n >= 1 && n <= kWfMaxN, "number of parallel channels must be in [1, %d] (got %d)", kWfMaxN, n);
    MCLE_REQUIRE(total_power > 0.0 && noise_var >= 0.0, "total power must be positive and the noise variance "
                                                        "non-negative");
    if (batch == 0) return MCLE_OK;
    int rc = ctx->bind();
    if (rc) return rc;
    hipLaunchKernelGGL(k_waterfilling, dim3(grid_for(ctx, batch, 64, 16)), dim3(64), 0, ctx->stream, d_gains, n,
                       total_power, noise_var, d_powers, d_mu, batch);
    MCLE_LAUNCH_CHECK();
    return MCLE_OK;
}

int mcle_block_diagonalize(mcle_ctx* ctx, const void* d_H, int num_users, int n_rx_per_user, double iPu,
                           double noise_var, int waterfilling, void* d_Ms, void* d_newH, void* d_W, double* d_sigma,
                           uint32_t* d_skipped, size_t batch) {
    MCLE_REQUIRE(ctx != nullptr && (batch == 0 || d_H != nullptr), "null argument");
    int rc = check_bd_dims(num_users, n_rx_per_user);
    if (rc) return rc;
    MCLE_REQUIRE(iPu > 0.0, "the power per user must be positive");
    MCLE_REQUIRE(noise_var >= 0.0, "noise variance must be non-negative");
    if (batch == 0) return MCLE_OK;
    if ((rc = ctx->bind())) return rc;
    hipLaunchKernelGGL(k_block_diagonalize, dim3(grid_for(ctx, batch, 64, 16)), dim3(64), 0, ctx->stream,
                       (const double2*)d_H, num_users, n_rx_per_user, iPu, noise_var, waterfilling ? 1 : 0,
                       (double2*)d_Ms, (double2*)d_newH, (double2*)d_W, d_sigma, d_skipped, batch);
    MCLE_LAUNCH_CHECK();
    return MCLE_OK;
}

int mcle_pinv(mcle_ctx* ctx, const void* d_A, int m, int n, double rcond, void* d_out, size_t batch) {
    MCLE_REQUIRE(ctx != nullptr && (batch == 0 || (d_A != nullptr && d_out != nullptr)), "null argument");
    MCLE_REQUIRE(m >= 1 && n >= 1 && m <= kBdMaxN && n <= kBdMaxN, "pinv supports matrices up to %d x %d (got %d x %d)",
                 kBdMaxN, kBdMaxN, m, n);
    MCLE_REQUIRE(rcond >= 0.0, "rcond must be non-negative");
    if (batch == 0) return MCLE_OK;
    int rc = ctx->bind();
    if (rc) return rc;
    hipLaunchKernelGGL(k_pinv, dim3(grid_for(ctx, batch, 64, 16)), dim3(64), 0, ctx->stream, (const double2*)d_A, m, n,
                       rcond, (double2*)d_out, batch);
    MCLE_LAUNCH_CHECK();
    return MCLE_OK;
}

int mcle_bd_extint(mcle_ctx* ctx, const mcle_bd_extint_cfg* cfg, const void* d_bigH, void* d_Ms, void* d_W,
                   int32_t* d_ns, double* d_cand_sinr, uint32_t* d_skipped, size_t batch) {
    MCLE_REQUIRE(ctx != nullptr && cfg != nullptr && d_bigH != nullptr && d_Ms != nullptr && d_W != nullptr, "null argument");
    MCLE_REQUIRE(cfg->num_users >= 1 && cfg->num_users <= 4 && cfg->n_ant_per_user >= 1 && cfg->n_ant_per_user <= kBdMaxR &&
                     cfg->num_users * cfg->n_ant_per_user <= kBdMaxN,
                 "block diagonalisation covers up to 4 users x 4 antennas with at most %d antennas in total", kBdMaxN);
    MCLE_REQUIRE(cfg->n_ext >= 0 && cfg->n_ext <= 8, "at most 8 external-interference antennas");
    MCLE_REQUIRE(cfg->method == 0 || cfg->method == 1, "method: 0 = WhiteningBD, 1 = EnhancedBD");
    MCLE_REQUIRE(cfg->metric >= 0 && cfg->metric <= 5, "metric must be in [0, 5]");
    MCLE_REQUIRE(cfg->iPu > 0.0 && cfg->noise_var >= 0.0 && cfg->pe >= 0.0, "iPu must be positive, noise_var and pe non-negative");
    MCLE_REQUIRE(cfg->method == 1 || cfg->noise_var > 0.0 || cfg->n_ext >= cfg->n_ant_per_user,
                 "whitening needs a positive definite interference-plus-noise covariance");
    if (cfg->method == 1 && (cfg->metric == 1 || cfg->metric == 2))
        MCLE_REQUIRE(cfg->num_streams >= 1 && cfg->num_streams <= cfg->n_ant_per_user,
                     "num_streams must be in [1, %d]", cfg->n_ant_per_user);
    if (cfg->method == 1 && cfg->metric == 5)
        for (int k = 0; k < cfg->num_users; ++k)
            MCLE_REQUIRE(cfg->ns_user[k] >= 1 && cfg->ns_user[k] <= cfg->n_ant_per_user, "ns_user[%d] out of range", k);
    MCLE_REQUIRE(cfg->metric != 4 || d_cand_sinr != nullptr, "metric 4 reports the candidate SINRs: d_cand_sinr is required");
    if (batch == 0) return MCLE_OK;
    int rc = ctx->bind();
    if (rc) return rc;
    BdExtParams pp;
    pp.K = cfg->num_users;
    pp.r = cfg->n_ant_per_user;
    pp.n_ext = cfg->n_ext;
    pp.method = cfg->method;
    pp.metric = cfg->metric;
    pp.num_streams = cfg->num_streams;
    for (int k = 0; k < 4; ++k) pp.ns_user[k] = cfg->ns_user[k];
    pp.iPu = cfg->iPu;
    pp.nv = cfg->noise_var;
    pp.pe = cfg->pe;
    if (d_cand_sinr)
        MCLE_HIP(hipMemsetAsync(d_cand_sinr, 0, batch * (size_t)pp.K * pp.r * pp.r * sizeof(double), ctx->stream));
    hipLaunchKernelGGL(k_bd_extint, dim3(grid_for(ctx, batch, 64, 16)), dim3(64), 0, ctx->stream, pp, (const cd*)d_bigH,
                       (cd*)d_Ms, (cd*)d_W, d_ns, d_cand_sinr, d_skipped, batch);
    MCLE_LAUNCH_CHECK();
    return MCLE_OK;
}

int mcle_run_bd(mcle_ctx* ctx, int dtype, const mcle_bd_cfg* cfg, uint64_t seed, uint64_t first, uint64_t count,
                mcle_counters* d_counters, uint32_t* d_sym_err, uint32_t* d_bit_err) {
    int rc = check_pipe(ctx, dtype, cfg ? cfg->demod_method : 0, cfg);
    if (rc) return rc;
    if ((rc = check_bd_dims(cfg->K, cfg->nr))) return rc;
    MCLE_REQUIRE(cfg->n_symbols >= 1, "n_symbols must be positive");
    MCLE_REQUIRE(cfg->iPu > 0.0, "the power per user must be positive");
    MCLE_REQUIRE(cfg->noise_var >= 0.0 && cfg->bd_noise_var >= 0.0, "noise variances must be non-negative");
    if ((rc = check_link_draws((uint64_t)(cfg->K * cfg->nr), cfg->n_symbols, count))) return rc;
    BdParams pp;
    pp.K = cfg->K;
    pp.r = cfg->nr;
    pp.n_symbols = cfg->n_symbols;
    pp.waterfill = cfg->waterfilling ? 1 : 0;
    pp.has_pathloss = cfg->has_pathloss ? 1 : 0;
    pp.iPu = cfg->iPu;
    pp.noise_var = cfg->noise_var;
    pp.bd_noise_var = cfg->bd_noise_var;
    for (int i = 0; i < 16; ++i) {
        const bool used = pp.has_pathloss && i < cfg->K * cfg->K;      // [K][K] row-major: rx user, tx user
        if (used) MCLE_REQUIRE(cfg->pathloss[i] >= 0.0, "path loss must be non-negative");
        pp.root_pl[i] = used ? std::sqrt(cfg->pathloss[i]) : 1.0;
    }
    if (count == 0) return MCLE_OK;
    if ((rc = ctx->bind())) return rc;
    switch (cfg->nr * 2 + (dtype == MCLE_F64)) {
        case 2: return launch_run_bd<float, 1>(ctx, cfg, pp, seed, first, count, d_counters, d_sym_err, d_bit_err);
        case 3: return launch_run_bd<double, 1>(ctx, cfg, pp, seed, first, count, d_counters, d_sym_err, d_bit_err);
        case 4: return launch_run_bd<float, 2>(ctx, cfg, pp, seed, first, count, d_counters, d_sym_err, d_bit_err);
        case 5: return launch_run_bd<double, 2>(ctx, cfg, pp, seed, first, count, d_counters, d_sym_err, d_bit_err);
        case 6: return launch_run_bd<float, 3>(ctx, cfg, pp, seed, first, count, d_counters, d_sym_err, d_bit_err);
        case 7: return launch_run_bd<double, 3>(ctx, cfg, pp, seed, first, count, d_counters, d_sym_err, d_bit_err);
        case 8: return launch_run_bd<float, 4>(ctx, cfg, pp, seed, first, count, d_counters, d_sym_err, d_bit_err);
        default: return launch_run_bd<double, 4>(ctx, cfg, pp, seed, first, count, d_counters, d_sym_err, d_bit_err);
    }
}

}  // extern "C"
