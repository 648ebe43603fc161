// pipeline_mimo_pilot.hip -- the flat MIMO (Blast) link with pilot-estimated channel state, next to perfect channel state.
// Reference: channel_estimation/estimators.py:12-61 compute_ls_estimation, :100-174 compute_mmse_estimation (Fodor et al. 2014)
// in front of mimo/mimo.py:463-660 Blast.  Per realization
//     H = alpha L W,   Y_p = H s + sqrt(noise_var) N_p,   H^ = Y_p s^H (s s^H)^-1   (LS)
//                                                         h^ = B (Y_p s^H) P / |s|^2 (MMSE, nt = 1; B formed by the caller)
// then the Blast receive filter from H^ (counter block 0) and from H (counter block 1), and ONE walk over the data symbols:
// both filters see the same symbols and the same noise samples, so the two error counts differ by the estimation error alone
// and the complex128 Box-Muller is paid once.
//
// Two launches, as pipeline_mimo_flat.hip: k_mimo_pilot_setup, one realization per lane, everything in f64 (the channel, the
// pilot block accumulated pilot by pilot -- nothing of size P stays live --, an nt x nt Hermitian Cholesky of the Gram matrix, two
// Blast filters); k_mimo_pilot_link, four independent wavefronts per workgroup, each walking the symbol columns of a chunk of
// realizations from their records.  Record per realization, rounded to the link's arithmetic:
//     A_est = G^ H / sqrt(nt) [4][4], G^ [4][4], A_perf = G H / sqrt(nt) [4][4], G [4][4], {ok, 0}.
// |H^ - H|_F^2 and |H|_F^2 leave the set-up kernel as f64 whatever the link's arithmetic.
//
// Draw ledger (mcle-philox-v1), realization first + r of `seed`:
//     W[r][a]               CHAN (2)    CN sample r nt + a                      as mcle_run_mimo_flat
//     data symbol           DATA (0)    n = t nt + a                            as mcle_run_mimo_flat
//     data noise (r, t)     NOISE (1)   CN sample r n_symbols + t               as mcle_run_mimo_flat
//     pilot phase (a, p)    PHASE (3)   uniform a P + p                         random pilots only
//     pilot noise (r, p)    PILOT (4)   CN sample 2 ceil(P / 2) r + p           (a Philox block = pilots 2 j, 2 j + 1 of one antenna)
// With L = I and alpha = 1 counter block 1 is mcle_run_mimo_flat(MCLE_MIMO_BLAST) on the same (seed, realization).
#include "mimo.hpp"
#include "modem.hpp"
#include "philox.hpp"
#include "pilot_block.hpp"
#include "pipe_common.hpp"
#include "qam_pack.hpp"
#include "totals.hpp"
#include "wave_draws.hpp"
#include "link_walk.hpp"

namespace mcle {

constexpr int kPilotMax = 4;                                   // antennas per side
constexpr int kPilotSet = 2 * kPilotMax * kPilotMax;           // A [4][4] then G [4][4] of one filter
constexpr int kPilotRec = 2 * kPilotSet + 1;                   // estimated CSI, perfect CSI, {ok, 0}

template <typename T, int NT, int NR>
__global__ __launch_bounds__(64) void k_mimo_pilot_setup(PilotSetup<kPilotMax> p, const double2* __restrict__ pilots,
                                                         const double2* __restrict__ Lm, const double2* __restrict__ Bm,
                                                         uint64_t seed, uint64_t first, uint64_t count,
                                                         cx<T>* __restrict__ recs, double* __restrict__ err_out,
                                                         double* __restrict__ pow_out) {
    const uint64_t rl = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (rl >= count) return;
    const Rng rng(seed, first + rl);
    const double2 zero = mk<double>(0, 0);
    // ---- H = alpha L W
    double2 H[NR][NT];
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int a = 0; a < NT; ++a) H[r][a] = cn_sample<double>(rng, STREAM_CHAN, (uint64_t)(r * NT + a), 1.0);
    if (Lm) {
        double2 W[NR][NT];
#pragma unroll
        for (int r = 0; r < NR; ++r)
#pragma unroll
            for (int a = 0; a < NT; ++a) W[r][a] = H[r][a];
#pragma unroll
        for (int r = 0; r < NR; ++r)
#pragma unroll
            for (int a = 0; a < NT; ++a) {
                double2 acc = zero;
#pragma unroll
                for (int k = 0; k < NR; ++k) acc = cfma4(Lm[r * NR + k], W[k][a], acc);
                H[r][a] = acc;
            }
    }
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int a = 0; a < NT; ++a) H[r][a] = cscale(H[r][a], p.alpha);      // (alpha = 1: exact)
    // ---- the pilot block, two pilots (one PILOT block per antenna) a trip: R = Y_p s^H, Gram = s s^H (lower triangle)
    double2 R[NR][NT], Gm[NT][NT];
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int a = 0; a < NT; ++a) R[r][a] = zero;
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b) Gm[a][b] = zero;
    for (int j = 0; j < p.half; ++j) {
        double2 n[2][NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            n[0][r] = n[1][r] = zero;
            if (p.sigma != 0.0) cn_pair<double>(rng, STREAM_PILOT, (uint32_t)(r * p.half + j), p.sigma, n[0][r], n[1][r]);
        }
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int pp = 2 * j + e;
            if (pp >= p.P) break;
            double2 s[NT];
#pragma unroll
            for (int a = 0; a < NT; ++a) {
                if (p.random_pilots) {
                    const double u = uniform_at(rng, STREAM_PHASE, (uint64_t)(a * p.P + pp));
                    double sn, cs;
                    sincospi(2.0 * u, &sn, &cs);
                    s[a] = mk<double>(p.amp * cs, p.amp * sn);
                } else {
                    s[a] = pilots[a * p.P + pp];
                }
            }
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                double2 y = n[e][r];
#pragma unroll
                for (int a = 0; a < NT; ++a) y = cfma4(H[r][a], s[a], y);
#pragma unroll
                for (int a = 0; a < NT; ++a) R[r][a] = cx_macc(R[r][a], y, s[a]);
            }
            if (p.random_pilots) {
#pragma unroll
                for (int a = 0; a < NT; ++a)
#pragma unroll
                    for (int b = 0; b <= a; ++b) Gm[a][b] = cx_macc(Gm[a][b], s[a], s[b]);
            }
        }
    }
    // ---- H^ = R Gram^-1
    double2 Hest[NR][NT];
    bool ok = true;
    double inv_s2 = p.ginv[0].x;                 // nt = 1: 1 / |s|^2
    if (p.random_pilots) {
        double invd[NT];
        ok = pilot_gram_factor<NT>(Gm, invd);
        inv_s2 = invd[0] * invd[0];
#pragma unroll
        for (int r = 0; r < NR; ++r) pilot_row_solve<NT>(Gm, invd, R[r], Hest[r]);
    } else {
        ok = p.gram_ok != 0;
#pragma unroll
        for (int r = 0; r < NR; ++r)
#pragma unroll
            for (int b = 0; b < NT; ++b) {
                double2 acc = zero;
#pragma unroll
                for (int a = 0; a < NT; ++a) acc = cfma4(R[r][a], p.ginv[a * kPilotMax + b], acc);
                Hest[r][b] = acc;
            }
    }
    if constexpr (NT == 1) {
        if (p.mmse_est) {                        // h^ = B (Y_p s^H) P / |s|^2
            const double scale = (double)p.P * inv_s2;
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                double2 acc = zero;
#pragma unroll
                for (int k = 0; k < NR; ++k) acc = cfma4(Bm[r * NR + k], R[k][0], acc);
                Hest[r][0] = cscale(acc, scale);
            }
        }
    }
    double err = 0.0, pw = 0.0;
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int a = 0; a < NT; ++a) {
            const double2 d = csub(Hest[r][a], H[r][a]);
            err += d.x * d.x + d.y * d.y;
            pw += H[r][a].x * H[r][a].x + H[r][a].y * H[r][a].y;
        }
    if (err_out) err_out[rl] = err;
    if (pow_out) pow_out[rl] = pw;
    // ---- the two filters and the record: A = G (H / sqrt(nt)), the association of k_mimo_flat_setup
    cx<T>* rec = recs + rl * kPilotRec;
    const double w = 1.0 / sqrt((double)NT);
    double2 HW[NR][NT];
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int a = 0; a < NT; ++a) HW[r][a] = cmul(H[r][a], mk<double>(w, 0.0));
#pragma unroll
    for (int set = 0; set < 2; ++set) {
        double2 G[NT][NR];
        const bool fok = set == 0 ? blast_filter<NT, NR>(Hest, p.filter_nv, G) : blast_filter<NT, NR>(H, p.filter_nv, G);
        ok = ok && fok;
        cx<T>* out = rec + set * kPilotSet;
#pragma unroll
        for (int i = 0; i < kPilotMax; ++i)
#pragma unroll
            for (int l = 0; l < kPilotMax; ++l) {
                double2 acc = zero, g = zero;
                if (i < NT && l < NT) {
#pragma unroll
                    for (int r = 0; r < NR; ++r) acc = cadd(acc, cmul(G[i < NT ? i : 0][r], HW[r][l < NT ? l : 0]));
                }
                if (i < NT && l < NR) g = G[i < NT ? i : 0][l < NR ? l : 0];
                out[i * kPilotMax + l] = mk<T>((T)acc.x, (T)acc.y);
                out[kPilotMax * kPilotMax + i * kPilotMax + l] = mk<T>((T)g.x, (T)g.y);
            }
    }
    rec[2 * kPilotSet] = mk<T>(ok ? (T)1 : (T)0, (T)0);
}

// COLS symbol columns of one lane through both filters: est = A d + G n per filter, in the association of k_mimo_flat_link; an
// entry of the record (the wavefront's LDS copy) is read once and serves every column
template <typename T, int COLS>
__device__ __forceinline__ void pilot_columns(const LinkDecide<T>& w, int nr, const cx<T>* s_rec, const int (&tx)[COLS][kPilotMax],
                                              const cx<T> (&nz)[COLS][kPilotMax], unsigned (&se)[2], unsigned (&be)[2]) {
    cx<T> d[COLS][kPilotMax];
#pragma unroll
    for (int c = 0; c < COLS; ++c)
#pragma unroll
        for (int l = 0; l < kPilotMax; ++l) d[c][l] = l < w.layers ? w.s_table[tx[c][l]] : mk<T>(0, 0);
#pragma unroll
    for (int set = 0; set < 2; ++set) {
        const cx<T>* A = s_rec + set * kPilotSet;
        const cx<T>* G = A + kPilotMax * kPilotMax;
        cx<T> est[COLS][kPilotMax];
#pragma unroll
        for (int l = 0; l < kPilotMax; ++l) {
#pragma unroll
            for (int c = 0; c < COLS; ++c) est[c][l] = mk<T>(0, 0);
            if (l < w.layers) {
#pragma unroll
                for (int k = 0; k < kPilotMax; ++k) {
                    if (k < w.layers) {
                        const cx<T> a = A[l * kPilotMax + k];
#pragma unroll
                        for (int c = 0; c < COLS; ++c) est[c][l] = cfma4(a, d[c][k], est[c][l]);
                    }
                    if (k < nr) {
                        const cx<T> g = G[l * kPilotMax + k];
#pragma unroll
                        for (int c = 0; c < COLS; ++c) est[c][l] = cfma4(g, nz[c][k], est[c][l]);
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < COLS; ++c) link_decide<T, kPilotMax>(w, est[c], tx[c], se[set], be[set]);
    }
}

// wavefronts per SIMD the walk's registers are bounded for: complex64 three (at the four of k_mimo_flat_link the two sets of
// estimates spill 17 registers), complex128 two
template <typename T> constexpr int pilot_walk_waves() { return sizeof(T) == 4 ? 3 : 2; }

template <typename T>
__global__ __launch_bounds__(256, pilot_walk_waves<T>()) void k_mimo_pilot_link(
    ModemParams<T> mp, int nt, int nr, int n_symbols, double noise_var, uint64_t seed, uint64_t first, uint64_t count,
    int per_wave, const cx<T>* __restrict__ recs, mcle_counters* counters, uint32_t* __restrict__ sym_est,
    uint32_t* __restrict__ bit_est, uint32_t* __restrict__ sym_perf, uint32_t* __restrict__ bit_perf) {
    __shared__ cx<T> s_table[256];
    __shared__ float4 s_tab4[sizeof(T) == 4 ? 256 : 1];     // {re, im, |c|^2 / 2, 0}: the lockstep searches of modem.hpp
    extern __shared__ unsigned long long s_grid[];          // [G*G] candidate grid (min-distance demodulation)
    __shared__ double s_bm[sizeof(T) == 8 ? kBmLdsDoubles : 1];   // complex128 Box-Muller tables (bm_f64.hpp)
    __shared__ cx<T> s_rec_all[4][kPilotRec + 1];           // each wavefront's current record
    __shared__ WgTotals totals_all[2][4];                   // [estimated | perfect CSI][wavefront]
    link_prologue(mp, s_table, s_tab4, s_grid, s_bm);
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const T sigma = (T)sqrt(noise_var);
    const uint32_t mask = (uint32_t)(mp.M - 1);
    const LinkDecide<T> w = link_decide_for(mp, s_table, s_tab4, s_grid, nt);
    cx<T>* s_rec = s_rec_all[wv];
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
            const cx<T>* rec = recs + rl * kPilotRec;
            for (int i = lane; i < kPilotRec; i += 64) s_rec[i] = rec[i];
            wave_lds_sync();
            unsigned se[2] = {0u, 0u}, be[2] = {0u, 0u};
            if ((n_symbols & 1) == 0) {
                for (int t0 = 0; t0 < n_symbols; t0 += kPairCols) {
                    // (the record is read where it is used, every pass: hoisted out of the loop its 128 complex values would
                    //  not fit the registers)
                    asm volatile("" ::: "memory");
                    const int t = t0 + 2 * lane;
                    if (t < n_symbols) {
                        int tx[2][kPilotMax];
#pragma unroll
                        for (int l = 0; l < kPilotMax; ++l) tx[0][l] = tx[1][l] = 0;
                        fortran_symbol_pair<kPilotMax>(rng, nt, (uint32_t)t, mask, tx[0], tx[1]);
                        cx<T> nz[2][kPilotMax];
#pragma unroll
                        for (int r = 0; r < kPilotMax; ++r) {
                            nz[0][r] = nz[1][r] = mk<T>(0, 0);
                            if (r < nr)
                                cn_pair_lds(rng, STREAM_NOISE, ((uint32_t)r * (uint32_t)n_symbols + (uint32_t)t) >> 1, sigma,
                                            nz[0][r], nz[1][r], s_bm);
                        }
                        pilot_columns<T, 2>(w, nr, s_rec, tx, nz, se, be);
                    }
                }
            } else {
                for (int t = lane; t < n_symbols; t += 64) {
                    asm volatile("" ::: "memory");
                    int tx[1][kPilotMax];
                    cx<T> nz[1][kPilotMax];
#pragma unroll
                    for (int l = 0; l < kPilotMax; ++l) tx[0][l] = l < nt ? (int)symbol_at(rng, (uint64_t)t * nt + l, mask) : 0;
#pragma unroll
                    for (int r = 0; r < kPilotMax; ++r)
                        nz[0][r] = r < nr ? cn_sample<T>(rng, STREAM_NOISE, (uint64_t)r * n_symbols + t, sigma) : mk<T>(0, 0);
                    pilot_columns<T, 1>(w, nr, s_rec, tx, nz, se, be);
                }
            }
            const bool skipped = s_rec[2 * kPilotSet].x == (T)0;
#pragma unroll
            for (int set = 0; set < 2; ++set) {
                link_account(totals_all[set][wv], se[set], be[set], skipped, rl, lane, set == 0 ? sym_est : sym_perf,
                             set == 0 ? bit_est : bit_perf);
            }
            wave_lds_sync();                    // the record's readers, before the next one overwrites it
        }
    }
    // one flush phase per workgroup: block 0, then block 1
    const unsigned long long n_sym = (unsigned long long)nt * n_symbols;
    wg_flush_waves<4>(totals_all[0], counters, n_sym, n_sym * mp.bits);
    wg_flush_waves<4>(totals_all[1], counters ? counters + 1 : nullptr, n_sym, n_sym * mp.bits);
}

template <typename T, int NT, int NR>
static void launch_pilot_setup(mcle_ctx* ctx, const PilotSetup<kPilotMax>& p, const double* d_pilots, const double* d_L, const double* d_B,
                               uint64_t seed, uint64_t first, uint64_t m, void* recs, double* d_err, double* d_pow) {
    hipLaunchKernelGGL((k_mimo_pilot_setup<T, NT, NR>), dim3((unsigned)((m + 63) / 64)), dim3(64), 0, ctx->stream, p,
                       (const double2*)d_pilots, (const double2*)d_L, (const double2*)d_B, seed, first, m, (cx<T>*)recs, d_err,
                       d_pow);
}

template <typename T>
static int run_mimo_pilot_link(mcle_ctx* ctx, const mcle_mimo_pilot_cfg* cfg, const PilotSetup<kPilotMax>& p, uint64_t seed, uint64_t first,
                               uint64_t count, const double* d_pilots, const double* d_L, const double* d_B,
                               mcle_counters* d_counters, uint32_t* d_sym_err, uint32_t* d_bit_err, double* d_err,
                               double* d_pow) {
    const int nt = cfg->nt, nr = cfg->nr;
    const ModemParams<T> mp = pipe_modem<T>(ctx, cfg->demod_method);
    const size_t lds = (size_t)mp.grid.G * mp.grid.G * sizeof(unsigned long long);
    const int per_wave = 16;
    // records of a slice of realizations, then their walk: at most 512 MiB of records per pair of launches, less on a crowded
    // device (down to 64 realizations: launch_sliced's floor)
    const size_t one = (size_t)kPilotRec * sizeof(cx<T>);
    // A unit is four chunks = 64 realizations of 2 nt (nt + nr) n_symbols complex multiply-adds each; the workgroup's one flush
    // phase is twelve atomics (pipe_common.hpp: flush_min_units, the estimate of pipeline_ia_general.hip)
    const uint64_t min_units = flush_min_units(2, 1u << 14, 2ull * nt * (nt + nr) * (uint64_t)cfg->n_symbols);
    const int rc = launch_sliced(
        ctx, first, count, ((size_t)512 << 20) / one, one, d_sym_err, d_bit_err,
        [&](void* recs, uint64_t at, uint64_t m) {
            const uint64_t off = at - first;
            double* e_out = d_err ? d_err + off : nullptr;
            double* p_out = d_pow ? d_pow + off : nullptr;
#define MCLE_PS(NT_, NR_) \
    if (nt == NT_ && nr == NR_) launch_pilot_setup<T, NT_, NR_>(ctx, p, d_pilots, d_L, d_B, seed, at, m, recs, e_out, p_out);
            MCLE_PS(1, 1) MCLE_PS(1, 2) MCLE_PS(1, 3) MCLE_PS(1, 4) MCLE_PS(2, 2) MCLE_PS(2, 3) MCLE_PS(2, 4) MCLE_PS(3, 3)
            MCLE_PS(3, 4) MCLE_PS(4, 4)
#undef MCLE_PS
        },
        [&](void* recs, uint64_t at, uint64_t m, uint32_t* se, uint32_t* be) {   // the perfect-CSI block follows the estimated one
            hipLaunchKernelGGL(k_mimo_pilot_link<T>, dim3(walk_grid(ctx, pilot_walk_waves<T>(), m, per_wave, min_units)), dim3(256), lds,
                               ctx->stream, mp, nt, nr, cfg->n_symbols, cfg->noise_var, seed, at, m, per_wave, (const cx<T>*)recs,
                               d_counters, se, be, se ? se + count : nullptr, be ? be + count : nullptr);
        },
        0, 64);
    if (rc) return rc;
    ctx->set_kernel("mimo_pilot_link %s %s", sizeof(T) == 8 ? "f64" : "f32", cfg->estimator ? "mmse" : "ls");
    return MCLE_OK;
}

}  // namespace mcle

using namespace mcle;

extern "C" int mcle_run_mimo_pilot_link(mcle_ctx* ctx, int dtype, const mcle_mimo_pilot_cfg* cfg, uint64_t seed, uint64_t first,
                                        uint64_t count, const double* d_pilots, const double* d_chan_factor,
                                        const double* d_mmse_matrix, mcle_counters* d_counters, uint32_t* d_sym_err,
                                        uint32_t* d_bit_err, double* d_err, double* d_pow) {
    if (ctx) ctx->last_kernel[0] = 0;
    int rc = check_pipe(ctx, dtype, cfg ? cfg->demod_method : 0, cfg);
    if (rc) return rc;
    const int nt = cfg->nt, nr = cfg->nr;
    MCLE_REQUIRE(nt >= 1 && nt <= nr && nr <= kPilotMax, "antenna counts must satisfy 1 <= nt <= nr <= %d (got nt %d, nr %d)", kPilotMax,
                 nt, nr);
    if ((rc = check_pilot_cfg(cfg, d_pilots, d_mmse_matrix, count))) return rc;
    if (count == 0) return MCLE_OK;
    PilotSetup<kPilotMax> p;
    if ((rc = pilot_setup_fill(ctx, cfg, d_pilots, d_counters, p))) return rc;
    return dtype == MCLE_F32 ? run_mimo_pilot_link<float>(ctx, cfg, p, seed, first, count, d_pilots, d_chan_factor, d_mmse_matrix,
                                                          d_counters, d_sym_err, d_bit_err, d_err, d_pow)
                             : run_mimo_pilot_link<double>(ctx, cfg, p, seed, first, count, d_pilots, d_chan_factor, d_mmse_matrix,
                                                           d_counters, d_sym_err, d_bit_err, d_err, d_pow);
}
