// pipeline_mimo_large_pilot.hip -- the large-array Blast link of pipeline_mimo_large.hip (1 <= Nt <= 8, Nt <= Nr <= 16, on the
// matrix cores) with pilot-estimated channel state next to perfect channel state: the experiment of pipeline_mimo_pilot.hip
// (channel_estimation/estimators.py:12-61 compute_ls_estimation, :100-174 compute_mmse_estimation, Fodor et al. 2014, in front of
// mimo/mimo.py:463-660 Blast) at the array sizes the estimators were written for.  Per realization
//     H = alpha L W,   Y_p = H s + sqrt(noise_var) N_p,   H^ = Y_p s^H (s s^H)^-1   (LS)
//                                                         h^ = B (Y_p s^H) P / |s|^2 (MMSE, nt = 1; B formed by the caller)
// then the Blast filter of H^ (counter block 0) and of H (counter block 1) and ONE walk over the data: every symbol and every
// noise sample is drawn once and multiplied through both filters.
//
// Draw ledger (mcle-philox-v1), the pilot link's word for word: CHAN sample r nt + a = W[r][a]; DATA symbol n = t nt + a; NOISE
// sample r n_symbols + t; PHASE uniform a P + p (random pilots only); PILOT sample 2 ceil(P / 2) r + p.  So up to 4 x 4 this is
// mcle_run_mimo_pilot_link on the same realizations, and with L = I, alpha = 1 block 1 is mcle_run_mimo_large at every shape.
//
// Two launches, the decomposition of pipeline_mimo_large.hip.  k_mimo_large_pilot_setup (always f64): one realization per row of
// 16 lanes, lane j owns receive antenna j -- row j of W, of H, of R = Y_p s^H and of H^; the pilot block is walked one pilot at a
// time; both filters by the Gram -> Cholesky -> own column of G -> A = G H / sqrt(Nt) sequence of k_mimo_large_setup, A with the
// TRUE channel both times (A_est = G^ H / sqrt(Nt): what the filter of the estimate does to the symbols that were sent).  Two
// records per realization in the operand order of mimo_large_entry, estimated then perfect, and one flag word.
// k_mimo_large_pilot_link: the walk of k_mimo_large_link with two left operands and two pairs of accumulators.
#include <cmath>
#include <complex>
#include <vector>

#include "cb_tile.hpp"
#include "mimo.hpp"
#include "mimo_large_map.hpp"
#include "modem.hpp"
#include "philox.hpp"
#include "pipe_common.hpp"
#include "totals.hpp"
#include "wave_draws.hpp"
#include "link_walk.hpp"

namespace mcle {

constexpr int kLpSlots = kLargeMaxNt + kLargeMaxNr;            // columns of [A | G] in LDS: A at 0 .. 7, G at 8 .. 23
constexpr int kLpMaxPilots = 256;
// a Gram pivot at or below this share of the Gram matrix's trace counts as singular (host and device alike): the pilot link's
constexpr double kLpPivotFloor = 1e-12;

struct LargePilotSetup {
    int nr, P, half;                            // half = ceil(P / 2)
    int random_pilots, mmse_est, gram_ok, f64;  // f64: the arithmetic of the records
    double amp, sigma, alpha, filter_nv;        // sqrt(pilot_power), sqrt(noise_var)
    double2 ginv[kLargeMaxNt * kLargeMaxNt];    // fixed pilots: (s s^H)^-1, entry [a][b] at a * kLargeMaxNt + b
};

// The Blast filter of the channel whose rows lie in s_src (lane j holds its own row in `own`), into s_m: G at columns
// kLargeMaxNt + r, A = G H / sqrt(Nt) at columns 0 .. NT - 1 with H from s_true.  Statement by statement the filter part of
// k_mimo_large_setup (pipeline_mimo_large.hip), so that with s_src == s_true the record is the one that kernel writes.
// Every thread of the workgroup calls it (two barriers).
template <int NT>
__device__ __forceinline__ bool large_pilot_filter(const double2 (*s_src)[NT], const double2 (*s_true)[NT], const double2 (&own)[NT],
                                                   double2 (*s_m)[kLpSlots], int nr, double filter_nv, int j) {
    const double2 zero = mk<double>(0, 0);
    double2 L[NT][NT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int k = 0; k <= i; ++k) L[i][k] = zero;
    for (int r = 0; r < nr; ++r) {
        double2 hr[NT];
#pragma unroll
        for (int a = 0; a < NT; ++a) hr[a] = s_src[r][a];
#pragma unroll
        for (int k = 0; k < NT; ++k)
#pragma unroll
            for (int i = k; i < NT; ++i) L[i][k] = cadd(L[i][k], cmulc(hr[k], hr[i]));     // conj(H[r][i]) * H[r][k]
    }
    double invd[NT];
    bool ok = true;
#pragma unroll
    for (int c = 0; c < NT; ++c) {
#pragma unroll
        for (int i = c; i < NT; ++i) {
            double2 a = L[i][c];
            if (i == c) a.x += filter_nv;
#pragma unroll
            for (int k = 0; k < c; ++k) a = csub(a, cmulc(L[i][k], L[c][k]));
            if (i == c) {
                ok = ok && (a.x > 1e-300);
                L[c][c] = mk<double>(sqrt(a.x), 0.0);
                invd[c] = 1.0 / L[c][c].x;
            } else {
                L[i][c] = cscale(a, invd[c]);
            }
        }
    }
    {
        // G[:, j]: L z = H^H[:, j], L^H w = z, x sqrt(Nt)
        const double root_nt = sqrt((double)NT);
        double2 z[NT];
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            double2 v = cconj(own[i]);
#pragma unroll
            for (int k = 0; k < i; ++k) v = csub(v, cmul(L[i][k], z[k]));
            z[i] = cscale(v, invd[i]);
        }
#pragma unroll
        for (int i = NT - 1; i >= 0; --i) {
            double2 v = z[i];
#pragma unroll
            for (int k = i + 1; k < NT; ++k) v = csub(v, cmul(cconj(L[k][i]), z[k]));
            z[i] = cscale(v, invd[i]);
        }
        // a filter that is not positive definite leaves zeros, not NaNs: the realization is marked and the link skips it
#pragma unroll
        for (int i = 0; i < NT; ++i) s_m[i][kLargeMaxNt + j] = (ok && j < nr) ? cscale(z[i], root_nt) : zero;
    }
    __syncthreads();
    {
        // A = G (H / sqrt(Nt)): entry e = i NT + a, sixteen entries at a time over the row's lanes
        const double wgt = 1.0 / sqrt((double)NT);
#pragma unroll
        for (int e0 = 0; e0 < NT * NT; e0 += 16) {
            const int e = e0 + j;
            if (e < NT * NT) {
                const int i = e / NT, a = e % NT;
                double2 acc = zero;
                for (int r = 0; r < nr; ++r) acc = cadd(acc, cmul(s_m[i][kLargeMaxNt + r], cscale(s_true[r][a], wgt)));
                s_m[i][a] = acc;
            }
        }
    }
    __syncthreads();
    return ok;
}

// one value of a 16-lane row's lane `src` to all of its lanes
__device__ __forceinline__ double2 row_bcast(double2 v, int src) {
    return mk<double>(__shfl(v.x, src, 16), __shfl(v.y, src, 16));
}

template <int NT>
__global__ __launch_bounds__(64) void k_mimo_large_pilot_setup(LargePilotSetup p, const double2* __restrict__ pilots,
                                                               const double2* __restrict__ Lm, const double2* __restrict__ Bm,
                                                               uint64_t seed, uint64_t first, uint64_t count,
                                                               void* __restrict__ recs, uint32_t* __restrict__ flags,
                                                               double* __restrict__ err_out, double* __restrict__ pow_out) {
    __shared__ double2 s_h[4][kLargeMaxNr][NT];             // [realization of the wavefront][r][a]: the true channel
    __shared__ double2 s_e[4][kLargeMaxNr][NT];             // W while H is formed, then the estimate
    __shared__ double2 s_m[2][4][NT][kLpSlots];             // [estimated | perfect][realization][stream][A | G]
    __shared__ double2 s_L[kLargeMaxNr * kLargeMaxNr];      // the channel factor, once per workgroup
    __shared__ double2 s_r[4][kLargeMaxNr];                 // MMSE: R; then {err, pow} of a row's lanes
    const int lane = threadIdx.x, w = lane >> 4, j = lane & 15, nr = p.nr;
    const uint64_t rl = (uint64_t)blockIdx.x * 4 + w;
    const bool live = rl < count, row = live && j < nr;
    const Rng rng(seed, first + rl);
    const double2 zero = mk<double>(0, 0);
    // ---- H = alpha L W: lane j draws row j of W
    double2 h[NT];
#pragma unroll
    for (int a = 0; a < NT; ++a) h[a] = row ? cn_sample<double>(rng, STREAM_CHAN, (uint64_t)(j * NT + a), 1.0) : zero;
    if (Lm) {
#pragma unroll
        for (int a = 0; a < NT; ++a) s_e[w][j][a] = h[a];
        for (int i = lane; i < nr * nr; i += 64) s_L[i] = Lm[i];
        __syncthreads();
        if (row) {
#pragma unroll
            for (int a = 0; a < NT; ++a) h[a] = zero;
            for (int c = 0; c < nr; ++c) {
                const double2 l = s_L[j * nr + c];
#pragma unroll
                for (int a = 0; a < NT; ++a) h[a] = cfma4(l, s_e[w][c][a], h[a]);
            }
        }
        __syncthreads();                                    // s_e is written again below
    }
#pragma unroll
    for (int a = 0; a < NT; ++a) {
        h[a] = cscale(h[a], p.alpha);                       // (alpha = 1: exact)
        s_h[w][j][a] = h[a];
    }
    // ---- the pilot block, one pilot at a time: R[j][:] = sum_p y_j conj(s), Gram = s s^H (lower triangle, drawn pilots)
    double2 R[NT], Gm[NT][NT];
#pragma unroll
    for (int a = 0; a < NT; ++a) {
        R[a] = zero;
#pragma unroll
        for (int b = 0; b <= a; ++b) Gm[a][b] = zero;
    }
    for (int jj = 0; jj < p.half; ++jj) {
        double2 n[2] = {zero, zero};
        if (row && p.sigma != 0.0) cn_pair<double>(rng, STREAM_PILOT, (uint32_t)(j * p.half + jj), p.sigma, n[0], n[1]);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int pp = 2 * jj + e;
            if (pp >= p.P) break;
            double2 s[NT];
            if (p.random_pilots) {
                // lane a of the row draws the pilot of transmit antenna a; every lane then holds the same NT values
                const int a = j < NT ? j : 0;
                const double u = uniform_at(rng, STREAM_PHASE, (uint64_t)(a * p.P + pp));
                double sn, cs;
                sincospi(2.0 * u, &sn, &cs);
                const double2 mine = mk<double>(p.amp * cs, p.amp * sn);
#pragma unroll
                for (int b = 0; b < NT; ++b) s[b] = row_bcast(mine, b);
            } else {
#pragma unroll
                for (int b = 0; b < NT; ++b) s[b] = pilots[b * p.P + pp];
            }
            double2 y = n[e];
#pragma unroll
            for (int a = 0; a < NT; ++a) y = cfma4(h[a], s[a], y);
#pragma unroll
            for (int a = 0; a < NT; ++a) R[a] = cx_macc(R[a], y, s[a]);
            if (p.random_pilots) {
#pragma unroll
                for (int a = 0; a < NT; ++a)
#pragma unroll
                    for (int b = 0; b <= a; ++b) Gm[a][b] = cx_macc(Gm[a][b], s[a], s[b]);
            }
        }
    }
    // ---- H^[j][:] = R[j][:] Gram^-1
    double2 he[NT];
    bool ok = true;
    double inv_s2 = p.ginv[0].x;                            // nt = 1: 1 / |s|^2
    if (p.random_pilots) {
        double tr = 0.0;
#pragma unroll
        for (int a = 0; a < NT; ++a) tr += Gm[a][a].x;
        // Gram = C C^H, C lower triangular, in place
        double invd[NT];
#pragma unroll
        for (int c = 0; c < NT; ++c) {
#pragma unroll
            for (int i = c; i < NT; ++i) {
                double2 a = Gm[i][c];
#pragma unroll
                for (int k = 0; k < c; ++k) a = csub(a, cmulc(Gm[i][k], Gm[c][k]));
                if (i == c) {
                    ok = ok && (a.x > kLpPivotFloor * tr);
                    Gm[c][c] = mk<double>(sqrt(a.x), 0.0);
                    invd[c] = 1.0 / Gm[c][c].x;
                } else {
                    Gm[i][c] = cscale(a, invd[c]);
                }
            }
        }
        inv_s2 = invd[0] * invd[0];
        // x C C^H = R: y C^H = R forwards, x C = y backwards
#pragma unroll
        for (int c = 0; c < NT; ++c) {
            double2 v = R[c];
#pragma unroll
            for (int k = 0; k < c; ++k) v = csub(v, cmulc(he[k], Gm[c][k]));
            he[c] = cscale(v, invd[c]);
        }
#pragma unroll
        for (int c = NT - 1; c >= 0; --c) {
            double2 v = he[c];
#pragma unroll
            for (int k = c + 1; k < NT; ++k) v = csub(v, cmul(he[k], Gm[k][c]));
            he[c] = cscale(v, invd[c]);
        }
    } else {
        ok = p.gram_ok != 0;
#pragma unroll
        for (int b = 0; b < NT; ++b) {
            double2 acc = zero;
#pragma unroll
            for (int a = 0; a < NT; ++a) acc = cfma4(R[a], p.ginv[a * kLargeMaxNt + b], acc);
            he[b] = acc;
        }
    }
    if constexpr (NT == 1) {
        if (p.mmse_est) {                                   // h^ = B (Y_p s^H) P / |s|^2
            s_r[w][j] = R[0];
            __syncthreads();
            double2 acc = zero;
            if (row)
                for (int c = 0; c < nr; ++c) acc = cfma4(Bm[j * nr + c], s_r[w][c], acc);
            he[0] = cscale(acc, (double)p.P * inv_s2);
            __syncthreads();                                // s_r is written again below
        }
    }
    double err = 0.0, pw = 0.0;
#pragma unroll
    for (int a = 0; a < NT; ++a) {
        if (!row) he[a] = zero;
        s_e[w][j][a] = he[a];
        const double2 d = csub(he[a], h[a]);
        err += d.x * d.x + d.y * d.y;
        pw += h[a].x * h[a].x + h[a].y * h[a].y;
    }
    s_r[w][j] = mk<double>(err, pw);
    __syncthreads();
    if (live && j == 0) {                                   // the row's 16 lanes in ascending order
        double e = 0.0, q = 0.0;
        for (int r = 0; r < nr; ++r) {
            e += s_r[w][r].x;
            q += s_r[w][r].y;
        }
        if (err_out) err_out[rl] = e;
        if (pow_out) pow_out[rl] = q;
    }
    // ---- the two filters: of the estimate, of the channel; A with the true channel both times
    const bool ok_est = large_pilot_filter<NT>(s_e[w], s_h[w], he, s_m[0][w], nr, p.filter_nv, j);
    const bool ok_perf = large_pilot_filter<NT>(s_h[w], s_h[w], h, s_m[1][w], nr, p.filter_nv, j);
    ok = ok && ok_est && ok_perf;
    if (live && j == 0) flags[rl] = ok ? 1u : 0u;
    const int steps = mimo_large_steps(NT, nr);
    for (int ww = 0; ww < 4; ++ww) {
        const uint64_t r2 = (uint64_t)blockIdx.x * 4 + ww;
        if (r2 >= count) break;
        for (int set = 0; set < 2; ++set) {
            const size_t base = ((size_t)r2 * 2 + (size_t)set) * (size_t)(64 * steps);
            for (int s = 0; s < steps; ++s) {
                const MimoLargeEntry en = mimo_large_entry(p.f64 != 0, NT, nr, s, lane);
                double v = 0.0;
                if (en.src != LARGE_ZERO) {
                    const double2 m = s_m[set][ww][en.i][en.src == LARGE_A ? en.col : kLargeMaxNt + en.col];
                    v = (en.part ? m.y : m.x) * (double)en.sign;
                }
                if (p.f64) reinterpret_cast<double*>(recs)[base + (size_t)(s * 64 + lane)] = v;
                else reinterpret_cast<float*>(recs)[base + (size_t)(s * 64 + lane)] = (float)v;
            }
        }
    }
}

// The walk of k_mimo_large_link (the same tiles, column pairing, NOISE and DATA block sharing: pipeline_mimo_large.hip and the
// maps of mimo_large_map.hpp, whose agreement with this spelling is asserted there at compile time) through TWO left operands:
// every symbol and every noise sample is drawn once and multiplied into the accumulators of both filters.  The perfect-CSI
// products are issued in the order of k_mimo_large_link.
template <typename T>
__global__ __launch_bounds__(256, sizeof(T) == 4 ? 3 : 2) void k_mimo_large_pilot_link(
    ModemParams<T> mp, int nt, int nr, int n_symbols, double noise_var, uint64_t seed, uint64_t first, uint64_t count,
    int per_wave, const T* __restrict__ recs, const uint32_t* __restrict__ flags, mcle_counters* counters,
    uint32_t* __restrict__ sym_est, uint32_t* __restrict__ bit_est, uint32_t* __restrict__ sym_perf,
    uint32_t* __restrict__ bit_perf) {
    using Tile = CbTile<T>;
    using Acc = typename Tile::acc;
    __shared__ cx<T> s_table[256];
    extern __shared__ unsigned long long s_grid[];       // [G*G] candidate grid (min-distance demodulation)
    __shared__ double s_bm[sizeof(T) == 8 ? kBmLdsDoubles : 1];   // complex128 Box-Muller tables (bm_f64.hpp)
    link_prologue(mp, s_table, nullptr, s_grid, s_bm);     // (no lockstep table: demod_one per stream)
    const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const T sigma = (T)sqrt(noise_var);
    const uint32_t mask = (uint32_t)(mp.M - 1);
    const int ps = mimo_large_sym_pairs(nt), pn = mimo_large_noise_pairs(nr);
    const size_t set_len = (size_t)64 * (size_t)(2 * (ps + pn));
    __shared__ WgTotals totals_all[2][4];                  // [estimated | perfect CSI][wavefront]
    if (lane == 0) {
        wg_zero(totals_all[0][wv]);
        wg_zero(totals_all[1][wv]);
    }
    __syncthreads();
    const uint64_t n_chunks = (count + per_wave - 1) / per_wave;
    for (uint64_t ch = (uint64_t)blockIdx.x * 4 + wv; ch < n_chunks; ch += (uint64_t)gridDim.x * 4) {
        const uint64_t r_end = (ch + 1) * per_wave < count ? (ch + 1) * per_wave : count;
        for (uint64_t rl = ch * per_wave; rl < r_end; ++rl) {
            const Rng rng(seed, first + rl);
            const T* rec = recs + rl * 2 * set_len + lane;
            // the left operands: one value per lane, K-step and filter (symbol steps, then noise steps)
            T as[2][4], an[2][8];
#pragma unroll
            for (int f = 0; f < 2; ++f) {
#pragma unroll
                for (int s = 0; s < 4; ++s) as[f][s] = s < 2 * ps ? rec[f * set_len + s * 64] : (T)0;
#pragma unroll
                for (int s = 0; s < 8; ++s) an[f][s] = s < 2 * pn ? rec[f * set_len + (2 * ps + s) * 64] : (T)0;
            }
            unsigned se[2] = {0u, 0u}, be[2] = {0u, 0u};
            for (int t0 = 0; t0 < n_symbols; t0 += 32) {
                const int t = t0 + 2 * n;                 // this lane's column of the even tile; t + 1 in the odd one
                Acc acc0[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, acc1[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
                int tx0[2] = {0, 0}, tx1[2] = {0, 0};
#pragma unroll
                for (int p = 0; p < 2; ++p)
                    if (p < ps) {
                        const int a = 4 * p + g;
                        cx<T> x0 = mk<T>(0, 0), x1 = mk<T>(0, 0);
                        if (a < nt && t < n_symbols) {
                            const uint32_t n0 = (uint32_t)t * (uint32_t)nt + (uint32_t)a, n1 = n0 + (uint32_t)nt;
                            const Words4 b0 = rng.block(STREAM_DATA, n0 >> 4);
                            tx0[p] = block_symbol(b0, n0, mask);
                            x0 = s_table[tx0[p]];
                            if (t + 1 < n_symbols) {
                                Words4 b1 = b0;
                                if ((n1 >> 4) != (n0 >> 4)) b1 = rng.block(STREAM_DATA, n1 >> 4);
                                tx1[p] = block_symbol(b1, n1, mask);
                                x1 = s_table[tx1[p]];
                            }
                        }
#pragma unroll
                        for (int f = 0; f < 2; ++f) {
                            acc0[f] = Tile::mma(as[f][2 * p], x0.x, acc0[f]);
                            acc1[f] = Tile::mma(as[f][2 * p], x1.x, acc1[f]);
                            acc0[f] = Tile::mma(as[f][2 * p + 1], x0.y, acc0[f]);
                            acc1[f] = Tile::mma(as[f][2 * p + 1], x1.y, acc1[f]);
                        }
                    }
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    if (p < pn) {
                        const int r = 4 * p + g;
                        cx<T> z0 = mk<T>(0, 0), z1 = mk<T>(0, 0);
                        if (r < nr && t < n_symbols) {
                            const uint32_t i0 = (uint32_t)r * (uint32_t)n_symbols + (uint32_t)t;
                            if ((i0 & 1u) == 0u) {       // samples t and t + 1 of the row are one block
                                cn_pair_lds(rng, STREAM_NOISE, i0 >> 1, sigma, z0, z1, s_bm);
                            } else {                     // an odd row of an odd number of columns: the pair straddles two blocks
                                z0 = cn_sample<T>(rng, STREAM_NOISE, (uint64_t)i0, sigma);
                                if (t + 1 < n_symbols) z1 = cn_sample<T>(rng, STREAM_NOISE, (uint64_t)i0 + 1u, sigma);
                            }
                        }
#pragma unroll
                        for (int f = 0; f < 2; ++f) {
                            acc0[f] = Tile::mma(an[f][2 * p], z0.x, acc0[f]);
                            acc1[f] = Tile::mma(an[f][2 * p], z1.x, acc1[f]);
                            acc0[f] = Tile::mma(an[f][2 * p + 1], z0.y, acc0[f]);
                            acc1[f] = Tile::mma(an[f][2 * p + 1], z1.y, acc1[f]);
                        }
                    }
                // result h + 2 part of the lane: part of stream g + 4 h (mimo_large_output), of either filter
#pragma unroll
                for (int f = 0; f < 2; ++f)
#pragma unroll
                    for (int hh = 0; hh < 2; ++hh)
                        if (g + 4 * hh < nt) {
                            if (t < n_symbols) {
                                const unsigned xr =
                                    (unsigned)(tx0[hh] ^ demod_one(mp, s_table, s_grid, mk<T>(acc0[f][hh], acc0[f][hh + 2])));
                                se[f] += (xr != 0u);
                                be[f] += __popc(xr);
                            }
                            if (t + 1 < n_symbols) {
                                const unsigned xr =
                                    (unsigned)(tx1[hh] ^ demod_one(mp, s_table, s_grid, mk<T>(acc1[f][hh], acc1[f][hh + 2])));
                                se[f] += (xr != 0u);
                                be[f] += __popc(xr);
                            }
                        }
            }
            const bool skipped = flags[rl] == 0u;
            link_account(totals_all[0][wv], se[0], be[0], skipped, rl, lane, sym_est, bit_est);
            link_account(totals_all[1][wv], se[1], be[1], skipped, rl, lane, sym_perf, bit_perf);
        }
    }
    // one flush phase per workgroup: block 0, then block 1
    const unsigned long long n_sym = (unsigned long long)nt * n_symbols;
    wg_flush_waves<4>(totals_all[0], counters, n_sym, n_sym * mp.bits);
    wg_flush_waves<4>(totals_all[1], counters ? counters + 1 : nullptr, n_sym, n_sym * mp.bits);
}

typedef std::complex<double> lp_zc;

// (s s^H)^-1 of the fixed pilots s [nt][P] by Gauss-Jordan with partial pivoting, complex128; false: numerically singular.  The
// pilot link's routine at this envelope's size.
static bool large_pilot_gram_inverse(const lp_zc* s, int nt, int P, double2* ginv) {
    lp_zc g[kLargeMaxNt][kLargeMaxNt], inv[kLargeMaxNt][kLargeMaxNt];
    double tr = 0.0;
    for (int a = 0; a < nt; ++a)
        for (int b = 0; b < nt; ++b) {
            lp_zc acc(0.0, 0.0);
            for (int p = 0; p < P; ++p) acc += s[a * P + p] * std::conj(s[b * P + p]);
            g[a][b] = acc;
            inv[a][b] = a == b ? lp_zc(1.0, 0.0) : lp_zc(0.0, 0.0);
            if (a == b) tr += acc.real();
        }
    if (!std::isfinite(tr) || !(tr > 0.0)) return false;
    for (int k = 0; k < nt; ++k) {
        int piv = k;
        for (int i = k + 1; i < nt; ++i)
            if (std::abs(g[i][k]) > std::abs(g[piv][k])) piv = i;
        if (!(std::abs(g[piv][k]) > kLpPivotFloor * tr)) return false;
        for (int j = 0; j < nt; ++j) {
            std::swap(g[k][j], g[piv][j]);
            std::swap(inv[k][j], inv[piv][j]);
        }
        const lp_zc d = 1.0 / g[k][k];
        for (int j = 0; j < nt; ++j) {
            g[k][j] *= d;
            inv[k][j] *= d;
        }
        for (int i = 0; i < nt; ++i) {
            if (i == k) continue;
            const lp_zc f = g[i][k];
            for (int j = 0; j < nt; ++j) {
                g[i][j] -= f * g[k][j];
                inv[i][j] -= f * inv[k][j];
            }
        }
    }
    for (int a = 0; a < nt; ++a)
        for (int b = 0; b < nt; ++b) ginv[a * kLargeMaxNt + b] = make_double2(inv[a][b].real(), inv[a][b].imag());
    return true;
}

template <typename T>
static int run_mimo_large_pilot(mcle_ctx* ctx, const mcle_mimo_pilot_cfg* cfg, LargePilotSetup p, uint64_t seed, uint64_t first,
                                uint64_t count, const double* d_pilots, const double* d_L, const double* d_B,
                                mcle_counters* d_counters, uint32_t* d_sym_err, uint32_t* d_bit_err, double* d_err,
                                double* d_pow) {
    const int nt = cfg->nt, nr = cfg->nr, steps = mimo_large_steps(nt, nr);
    const int per_wave = 16;
    const ModemParams<T> mp = pipe_modem<T>(ctx, cfg->demod_method);
    const size_t lds = (size_t)mp.grid.G * mp.grid.G * sizeof(unsigned long long);
    p.f64 = sizeof(T) == 8;
    // two records of k_mimo_large_link's length per realization, then one flag word -- at most 12 KiB (8 x 16, complex128), so
    // the slice is sized by bytes: at most 128 MiB of records
    const size_t rec_bytes = 2 * (size_t)mimo_large_record_len(nt, nr) * sizeof(T);
    const uint64_t k_slice = ((uint64_t)128 << 20) / rec_bytes;
    const uint64_t slice = count < k_slice ? count : k_slice;
    int rc = launch_sliced(
        ctx, first, count, k_slice, rec_bytes, d_sym_err, d_bit_err,
        [&](void* recs, uint64_t at, uint64_t m) {
            uint32_t* flags = reinterpret_cast<uint32_t*>(static_cast<char*>(recs) + (size_t)slice * rec_bytes);
            const uint64_t off = at - first;
            double* e_out = d_err ? d_err + off : nullptr;
            double* p_out = d_pow ? d_pow + off : nullptr;
            const unsigned sgrid = (unsigned)((m + 3) / 4);
#define MCLE_LPS(NT_)                                                                                                            \
    case NT_:                                                                                                                    \
        hipLaunchKernelGGL(k_mimo_large_pilot_setup<NT_>, dim3(sgrid), dim3(64), 0, ctx->stream, p, (const double2*)d_pilots,    \
                           (const double2*)d_L, (const double2*)d_B, seed, at, m, recs, flags, e_out, p_out);                    \
        break;
            switch (nt) {
                MCLE_LPS(1) MCLE_LPS(2) MCLE_LPS(3) MCLE_LPS(4) MCLE_LPS(5) MCLE_LPS(6) MCLE_LPS(7) MCLE_LPS(8)
            }
#undef MCLE_LPS
        },
        [&](void* recs, uint64_t at, uint64_t m, uint32_t* se, uint32_t* be) {   // the perfect-CSI block follows the estimated one
            const uint32_t* flags = reinterpret_cast<const uint32_t*>(static_cast<char*>(recs) + (size_t)slice * rec_bytes);
            hipLaunchKernelGGL(k_mimo_large_pilot_link<T>, dim3(walk_grid(ctx, sizeof(T) == 4 ? 3 : 2, m, per_wave)), dim3(256), lds,
                               ctx->stream, mp, nt, nr, cfg->n_symbols, cfg->noise_var, seed, at, m, per_wave, (const T*)recs, flags,
                               d_counters, se, be, se ? se + count : nullptr, be ? be + count : nullptr);
        },
        sizeof(uint32_t));
    if (rc) return rc;
    ctx->set_kernel("mimo_large_pilot_link %s %dx%d s%d %s", sizeof(T) == 8 ? "f64" : "f32", nr, nt, steps,
                    cfg->estimator ? "mmse" : "ls");
    return MCLE_OK;
}

}  // namespace mcle

using namespace mcle;

extern "C" int mcle_run_mimo_large_pilot(mcle_ctx* ctx, int dtype, const mcle_mimo_pilot_cfg* cfg, uint64_t seed, uint64_t first,
                                         uint64_t count, const double* d_pilots, const double* d_chan_factor,
                                         const double* d_mmse_matrix, mcle_counters* d_counters, uint32_t* d_sym_err,
                                         uint32_t* d_bit_err, double* d_err, double* d_pow) {
    if (ctx) ctx->last_kernel[0] = 0;
    int rc = check_pipe(ctx, dtype, cfg ? cfg->demod_method : 0, cfg);
    if (rc) return rc;
    const int nt = cfg->nt, nr = cfg->nr, P = cfg->n_pilots;
    MCLE_REQUIRE(nt >= 1 && nt <= kLargeMaxNt && nr >= nt && nr <= kLargeMaxNr,
                 "antenna counts must satisfy 1 <= nt <= %d, nt <= nr <= %d (got nt %d, nr %d)", kLargeMaxNt, kLargeMaxNr, nt, nr);
    MCLE_REQUIRE(P >= nt && P <= kLpMaxPilots, "n_pilots must be in [nt, %d] (got %d pilots, nt %d)", kLpMaxPilots, P, nt);
    MCLE_REQUIRE(cfg->n_symbols >= 1, "n_symbols must be positive");
    MCLE_REQUIRE(cfg->estimator == 0 || cfg->estimator == 1, "estimator must be 0 (LS) or 1 (MMSE) (got %d)", cfg->estimator);
    MCLE_REQUIRE(cfg->random_pilots == 0 || cfg->random_pilots == 1, "random_pilots must be 0 or 1 (got %d)", cfg->random_pilots);
    MCLE_REQUIRE(cfg->mmse_filter == 0 || cfg->mmse_filter == 1, "mmse_filter must be 0 or 1 (got %d)", cfg->mmse_filter);
    MCLE_REQUIRE(std::isfinite(cfg->noise_var) && cfg->noise_var >= 0.0, "Noise variance must be a non-negative value.");
    MCLE_REQUIRE(std::isfinite(cfg->pilot_power) && cfg->pilot_power > 0.0, "pilot_power must be finite and positive");
    MCLE_REQUIRE(std::isfinite(cfg->alpha), "alpha must be finite");
    MCLE_REQUIRE(cfg->random_pilots || d_pilots != nullptr, "null d_pilots with random_pilots = 0");
    MCLE_REQUIRE(cfg->estimator == 0 || nt == 1, "the MMSE estimator needs nt = 1 (got %d)", nt);
    MCLE_REQUIRE(cfg->estimator == 0 || d_mmse_matrix != nullptr, "the MMSE estimator needs d_mmse_matrix (from a covariance)");
    if ((rc = check_link_draws((uint64_t)nr, cfg->n_symbols, count))) return rc;
    if (count == 0) return MCLE_OK;
    MCLE_REQUIRE(d_counters != nullptr, "null d_counters");
    if ((rc = ctx->bind())) return rc;
    LargePilotSetup p{};
    p.nr = nr, p.P = P, p.half = (P + 1) / 2;
    p.random_pilots = cfg->random_pilots, p.mmse_est = cfg->estimator, p.gram_ok = 1;
    p.amp = std::sqrt(cfg->pilot_power), p.sigma = std::sqrt(cfg->noise_var), p.alpha = cfg->alpha;
    p.filter_nv = cfg->mmse_filter ? cfg->noise_var : 0.0;
    if (!cfg->random_pilots) {
        // the fixed block's inverse Gram matrix, once, on the host
        std::vector<lp_zc> s((size_t)nt * P);
        MCLE_HIP(hipMemcpyAsync(s.data(), d_pilots, s.size() * sizeof(lp_zc), hipMemcpyDeviceToHost, ctx->stream));
        MCLE_HIP(hipStreamSynchronize(ctx->stream));
        p.gram_ok = large_pilot_gram_inverse(s.data(), nt, P, p.ginv) ? 1 : 0;
    }
    return dtype == MCLE_F32
               ? run_mimo_large_pilot<float>(ctx, cfg, p, seed, first, count, d_pilots, d_chan_factor, d_mmse_matrix, d_counters,
                                             d_sym_err, d_bit_err, d_err, d_pow)
               : run_mimo_large_pilot<double>(ctx, cfg, p, seed, first, count, d_pilots, d_chan_factor, d_mmse_matrix, d_counters,
                                              d_sym_err, d_bit_err, d_err, d_pow);
}
