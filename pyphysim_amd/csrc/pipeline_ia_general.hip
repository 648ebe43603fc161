// pipeline_ia_general.hip -- the fused interference-alignment link on general geometries (mcle_run_ia_general): 2 <= K <= 4
// users of up to 6 x 6 antennas, per-user stream counts, with the greedy / brute-force stream selection of the solver.
//
// Reference: apps/ia/simulate_ia.py:94-245 (Nr, Nt, Ns as parameters), apps/ia/IA_Results_NrxNt(Ns).py:130-133 (K = 3, 5 x 3,
// Ns = 2), apps/ia/simulate_greedy_ia.py:300-430 (3 x 3 with Ns = 3 under GreedStreamIASolver; 'NoPathLoss' is this link with
// P = 1, noise_var = 1 / SNR); ia/iabase.py:188-327 (full_F, full_W_H), :538-540 (randomizeF); channels/multiuser.py:1003-1044,
// 1179-1262 (randomize / corrupt_data).
//
// Four launches per slice, the shape of run_ia_impl (kernels_ia.hip): draw -> solve -> record -> walk.
//   k_iagl_draw    big_H [K nr][K nt] and the padded random start [4][D][D], f64 for either dtype (the solver is f64 only)
//   k_ia_general   the operator's own kernel on those buffers (ia_general.hpp): bit-identical to mcle_ia_solve_general
//   k_iagl_record  one lane per realization: the end-to-end link of the KEPT streams, rounded once to the call's dtype
//   k_iagl_link    the symbol walk: est_s = sum_a U[s][a] n_a + sum_t G[s][t] x_t, demodulate, count per stream slot
//
// Record (cx<T>, stride 1 + S0^2 + S0 nr with S0 = sum of the CONFIGURED stream counts; kept streams numbered
// q = 0, 1, .. in user order, S = sum of the kept counts <= S0):
//   [0]                   (1 | 0: flagged by the solver, ns_0 + 8 ns_1 + 64 ns_2 + 512 ns_3: the kept counts)
//   [1 + q S0 + t]        G[q][t] = (U_k H_kl F_l)[j][j'], q = (k, j), t = (l, j'); q, t < S
//   [1 + S0^2 + q nr + a] U_k[j][a]: the stream's row of full_W_H
#include "modem.hpp"
#include "philox.hpp"
#include "pipe_common.hpp"
#include "totals.hpp"
#include "wave_draws.hpp"
#include "link_walk.hpp"
#include "ia_general.hpp"

namespace mcle {

constexpr int kIaglSlots = 6;       // stream slots per user of the [count][4][6] outputs

struct IaglShape {
    int K, nr, nt, D;               // D: padding of the solver's arrays (4 or 6)
    int ns[kIagUsers];              // configured stream counts (0 beyond K)
    int S0;                         // their sum
    int n_symbols;
    int draw_start;                 // MCLE_IA_INIT_GIVEN: the random start is drawn
};

// One thread per entry of big_H, one per (realization, user) for the start: F_k = randn_c(nt, ns[k]) / |.|_F in the top-left
// corner of the user's D x D block (iabase.py:538-540), zeros around it.
__global__ __launch_bounds__(256) void k_iagl_draw(IaglShape sh, uint64_t seed, uint64_t first, uint64_t n,
                                                   double2* __restrict__ bigH, double2* __restrict__ F_init) {
    const uint64_t hn = (uint64_t)(sh.K * sh.nr) * (uint64_t)(sh.K * sh.nt);
    const uint64_t n_h = n * hn, total = n_h + (sh.draw_start ? n * kIagUsers : 0);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        if (i < n_h) {
            const uint64_t rl = i / hn, e = i - rl * hn;
            bigH[i] = cn_sample<double>(Rng(seed, first + rl), STREAM_CHAN, e, 1.0);
            continue;
        }
        const uint64_t u = i - n_h, rl = u / kIagUsers;
        const int k = (int)(u - rl * kIagUsers), D = sh.D;
        double2* blk = F_init + (rl * kIagUsers + k) * (uint64_t)(D * D);
        for (int e = 0; e < D * D; ++e) blk[e] = mk<double>(0.0, 0.0);
        if (k >= sh.K) continue;
        const Rng rng(seed, first + rl);
        int before = 0;
        for (int kk = 0; kk < k; ++kk) before += sh.ns[kk];
        const int nsk = sh.ns[k], base = sh.nt * before;
        double norm2 = 0.0;
        for (int e = 0; e < sh.nt * nsk; ++e) {
            const double2 z = cn_sample<double>(rng, STREAM_PHASE, (uint64_t)(base + e), 1.0);
            norm2 += z.x * z.x + z.y * z.y;
            blk[(e / nsk) * D + (e % nsk)] = z;
        }
        const double norm = sqrt(norm2);
        for (int e = 0; e < sh.nt * nsk; ++e) {
            double2& z = blk[(e / nsk) * D + (e % nsk)];
            z.x /= norm;
            z.y /= norm;
        }
    }
}

// One lane per realization: the record above from the solver's padded F and U.
template <typename T>
__global__ __launch_bounds__(64) void k_iagl_record(IaglShape sh, const double2* __restrict__ bigH,
                                                    const double2* __restrict__ F, const double2* __restrict__ U,
                                                    const int32_t* __restrict__ ns, const uint32_t* __restrict__ skipped,
                                                    const double* __restrict__ sinr, cx<T>* __restrict__ recs,
                                                    double* __restrict__ sinr_out /* [n][4][6] or NULL */, uint64_t n) {
    const uint64_t rl = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (rl >= n) return;
    const int K = sh.K, nr = sh.nr, nt = sh.nt, D = sh.D, S0 = sh.S0, cols = K * nt;
    const double2* H = bigH + rl * (uint64_t)(K * nr) * (uint64_t)cols;
    const double2* Fr = F + rl * (uint64_t)(kIagUsers * D * D);
    const double2* Ur = U + rl * (uint64_t)(kIagUsers * D * D);
    cx<T>* rec = recs + rl * (uint64_t)(1 + S0 * S0 + S0 * nr);
    int nsu[kIagUsers];
    bool ok = skipped[rl] == 0u;
    for (int k = 0; k < kIagUsers; ++k) {
        nsu[k] = k < K ? ns[rl * kIagUsers + k] : 0;
        if (nsu[k] < 0 || nsu[k] > sh.ns[k]) ok = false;       // (the solver only ever lowers a count)
    }
    if (sinr_out)                                            // the solver's [4][D] in the entry point's [4][6]
        for (int k = 0; k < kIagUsers; ++k)
            for (int j = 0; j < kIaglSlots; ++j)
                sinr_out[(rl * kIagUsers + k) * kIaglSlots + j] = j < D ? sinr[(rl * kIagUsers + k) * D + j] : 0.0;
    if (!ok)
        for (int k = 0; k < kIagUsers; ++k) nsu[k] = 0;
    rec[0] = mk<T>(ok ? (T)1 : (T)0, (T)(nsu[0] | (nsu[1] << 3) | (nsu[2] << 6) | (nsu[3] << 9)));
    int q = 0;
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < nsu[k]; ++j, ++q) {
            const double2* u = Ur + (k * D + j) * D;         // row j of U_k
            int t = 0;
            for (int l = 0; l < K; ++l) {
                double2 v[6];                                // u H_kl, 1 x nt
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    v[c] = mk<double>(0.0, 0.0);
                    if (c < nt)
                        for (int a = 0; a < nr; ++a) v[c] = cfma4(u[a], H[(k * nr + a) * cols + l * nt + c], v[c]);
                }
                for (int jj = 0; jj < nsu[l]; ++jj, ++t) {
                    double2 g = mk<double>(0.0, 0.0);
#pragma unroll
                    for (int c = 0; c < 6; ++c)
                        if (c < nt) g = cfma4(v[c], Fr[(l * D + c) * D + jj], g);
                    rec[1 + q * S0 + t] = mk<T>((T)g.x, (T)g.y);
                }
            }
            for (int a = 0; a < nr; ++a) rec[1 + S0 * S0 + q * nr + a] = mk<T>((T)u[a].x, (T)u[a].y);
        }
}

// The symbol walk: workgroups of four independent wavefronts, each taking chunks of per_wave consecutive realizations; the
// lanes of a wavefront take the symbol columns of one realization -- two adjacent columns each where n_symbols is even (PAIR:
// the two samples of one Philox block per noise draw, the data blocks shared across the wave), one otherwise.
// D: the capacity of the antenna count and of a user's stream count (4 or 6, the solver's classes); every register array is
// unrolled to it with wave-uniform predicates, so none is indexed at run time.
// The record is wave-uniform.  Its header is a scalar load; G and U are staged in the wavefront's own LDS region once per
// realization and read by broadcast (every lane the same address): as scalar loads the unrolled G reads were hoisted into
// more SGPRs than the wavefront has (135-238 of them spilled to VGPR lanes).
// Receiver by receiver, in a rolled loop: live per column are one user's <= D noise samples and <= D accumulators, the labels
// of all <= 4 D streams packed as bytes, and one looked-up x_t.  The per-slot counts live in LDS (a register array would be
// indexed by the rolled user loop): one wave sum of (symbol errors | bit errors << 16) per stream and pass.
// Dynamic LDS: the candidate grid, then 4 x (stride rounded up to 2) cx<T>.
template <typename T, int D, bool PAIR>
__global__ __launch_bounds__(256) void k_iagl_link(ModemParams<T> mp, IaglShape sh, double noise_var, uint64_t seed,
                                                   uint64_t first, uint64_t count, int per_wave,
                                                   const cx<T>* __restrict__ recs, mcle_counters* counters,
                                                   uint32_t* __restrict__ sym_out, uint32_t* __restrict__ bit_out,
                                                   uint32_t* __restrict__ ssym_out, uint32_t* __restrict__ sbit_out) {
    constexpr int SMAX = kIagUsers * D, W = SMAX / 4, COLS = PAIR ? 2 : 1, SLOTS = kIagUsers * kIaglSlots;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned long long* s_grid = reinterpret_cast<unsigned long long*>(smem);
    __shared__ cx<T> s_table[256];
    __shared__ WgTotals totals_all[4];
    __shared__ unsigned s_cnt_all[4][2][SLOTS];                   // per wavefront: symbol / bit errors by stream slot
    __shared__ double s_bm[sizeof(T) == 8 ? kBmLdsDoubles : 1];   // complex128 Box-Muller tables (bm_f64.hpp)
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    WgTotals& totals = totals_all[wv];
    unsigned(&s_cnt)[2][SLOTS] = s_cnt_all[wv];
    link_prologue(mp, s_table, nullptr, s_grid, s_bm);     // (no lockstep table: demod_one per stream)
    const int lane = threadIdx.x & 63;
    const int K = sh.K, nr = sh.nr, S0 = sh.S0;
    const int stride = 1 + S0 * S0 + S0 * nr, stride_lds = (stride + 1) & ~1;
    const size_t grid_bytes = ((size_t)mp.grid.G * mp.grid.G * sizeof(unsigned long long) + 15) & ~(size_t)15;
    cx<T>* s_rec = reinterpret_cast<cx<T>*>(smem + grid_bytes) + (size_t)wv * stride_lds;
    const cx<T>* sG = s_rec + 1;
    const cx<T>* sU = sG + S0 * S0;
    const T sigma = (T)sqrt(noise_var);
    const uint32_t mask = (uint32_t)(mp.M - 1);
    const uint32_t NS = (uint32_t)sh.n_symbols;
    if (lane == 0) wg_zero(totals);
    if (lane < SLOTS) s_cnt[0][lane] = s_cnt[1][lane] = 0u;
    __syncthreads();
    const uint64_t n_chunks = (count + per_wave - 1) / per_wave;
    for (uint64_t ch = (uint64_t)blockIdx.x * 4 + wv; ch < n_chunks; ch += (uint64_t)gridDim.x * 4) {
        const uint64_t r_end = (ch + 1) * per_wave < count ? (ch + 1) * per_wave : count;
        for (uint64_t rl = ch * per_wave; rl < r_end; ++rl) {
            const Rng rng(seed, first + rl);
            const cx<T>* rec = recs + rl * (size_t)stride;
            const cx<T> head = rec[0];                   // wave-uniform: a scalar load
            const bool ok = head.x != (T)0;
            const int kept = (int)head.y;                // 3 bits per user
            const int S = (kept & 7) + ((kept >> 3) & 7) + ((kept >> 6) & 7) + ((kept >> 9) & 7);
            if (ok) {
                const int n_g = 1 + S0 * S;              // the header and rows q < S of G, then rows q < S of U
                for (int i = lane; i < n_g + S * nr; i += 64) {
                    const int at = i < n_g ? i : i - n_g + 1 + S0 * S0;
                    s_rec[at] = rec[at];
                }
            }
            wave_lds_sync();
            for (uint32_t t0 = 0; ok && t0 < NS; t0 += 64u * COLS) {
                const uint32_t t = t0 + (uint32_t)COLS * (uint32_t)lane;
                // a lane beyond the last column of the ragged last pass walks on (draws at positions nobody reads, a valid label)
                // and counts nothing: every lane takes part in the wave sums below
                const bool live = t < NS;
                uint32_t lab[COLS][W];                   // the labels of the S streams, bytes
#pragma unroll
                for (int w = 0; w < W; ++w) lab[0][w] = lab[COLS - 1][w] = 0u;
                if constexpr (PAIR) {
                    // the Philox blocks of the data are shared across the wave (wave_draws.hpp; every lane takes part)
                    int ta[SMAX], tb[SMAX];
                    wave_symbol_pairs<SMAX>(rng, S, NS, t0, mask, lane, ta, tb);
#pragma unroll
                    for (int q = 0; q < SMAX; ++q)
                        if (q < S) {
                            lab[0][q >> 2] |= (uint32_t)ta[q] << ((q & 3) * 8);
                            lab[COLS - 1][q >> 2] |= (uint32_t)tb[q] << ((q & 3) * 8);
                        }
                } else {
#pragma unroll
                    for (int q = 0; q < SMAX; ++q)
                        if (q < S) lab[0][q >> 2] |= symbol_at(rng, (uint32_t)q * NS + t, mask) << ((q & 3) * 8);
                }
                int q0 = 0;                              // kept streams before this user
#pragma unroll 1
                for (int k = 0; k < K; ++k) {
                    const int nsk = (kept >> (3 * k)) & 7;
                    cx<T> nz[COLS][D], acc[COLS][D];
                    // the user's own labels by stream, bytes: picked up where the walk over all streams passes them (a label
                    // read from `lab` at the run-time index q0 + j puts `lab` into scratch)
                    unsigned long long own[COLS];
                    own[0] = own[COLS - 1] = 0ull;
#pragma unroll
                    for (int a = 0; a < D; ++a)
                        if (a < nr) {
                            const uint32_t pos = (uint32_t)(k * nr + a) * NS + t;
                            if constexpr (PAIR) cn_pair_lds(rng, STREAM_NOISE, pos >> 1, sigma, nz[0][a], nz[COLS - 1][a], s_bm);
                            else nz[0][a] = cn_one_lds(rng, STREAM_NOISE, pos, sigma, s_bm);
                        }
#pragma unroll
                    for (int j = 0; j < D; ++j)
                        if (j < nsk) {
#pragma unroll
                            for (int c = 0; c < COLS; ++c) acc[c][j] = mk<T>((T)0, (T)0);
#pragma unroll
                            for (int a = 0; a < D; ++a)
                                if (a < nr) {
                                    const cx<T> u = sU[(q0 + j) * nr + a];
#pragma unroll
                                    for (int c = 0; c < COLS; ++c) acc[c][j] = cfma4(u, nz[c][a], acc[c][j]);
                                }
                        }
#pragma unroll
                    for (int tt = 0; tt < SMAX; ++tt)
                        if (tt < S) {
                            cx<T> x[COLS];
                            const bool mine = (unsigned)(tt - q0) < (unsigned)nsk;    // stream tt is this user's stream tt - q0
#pragma unroll
                            for (int c = 0; c < COLS; ++c) {
                                const uint32_t label = (lab[c][tt >> 2] >> ((tt & 3) * 8)) & 0xFFu;
                                x[c] = s_table[label];
                                if (mine) own[c] |= (unsigned long long)label << (8 * (tt - q0));
                            }
#pragma unroll
                            for (int j = 0; j < D; ++j)
                                if (j < nsk) {
                                    const cx<T> g = sG[(q0 + j) * S0 + tt];
#pragma unroll
                                    for (int c = 0; c < COLS; ++c) acc[c][j] = cfma4(g, x[c], acc[c][j]);
                                }
                        }
#pragma unroll
                    for (int j = 0; j < D; ++j)
                        if (j < nsk) {
                            unsigned e = 0;              // symbol errors | bit errors << 16 of this lane's columns
#pragma unroll
                            for (int c = 0; c < COLS; ++c) {
                                const int sent = (int)((own[c] >> (8 * j)) & 0xFFu);
                                const unsigned x = (unsigned)(sent ^ demod_one(mp, s_table, s_grid, acc[c][j]));
                                e += (x != 0u) + ((unsigned)__popc(x) << 16);
                            }
                            e = wave_sum_u32(live ? e : 0u);     // <= 128 symbols and <= 1024 bits per pass
                            if (lane == 0) {
                                s_cnt[0][k * kIaglSlots + j] += e & 0xFFFFu;
                                s_cnt[1][k * kIaglSlots + j] += e >> 16;
                            }
                        }
                    q0 += nsk;
                }
            }
            wave_lds_sync();
            unsigned se = 0, be = 0;
            if (lane < SLOTS) {
                se = s_cnt[0][lane];
                be = s_cnt[1][lane];
                s_cnt[0][lane] = s_cnt[1][lane] = 0u;
                if (ssym_out) ssym_out[rl * SLOTS + lane] = se;
                if (sbit_out) sbit_out[rl * SLOTS + lane] = be;
            }
            link_account(totals, se, be, !ok, rl, lane, sym_out, bit_out);
            wave_lds_sync();
        }
    }
    wg_flush_waves<4>(totals_all, counters, (unsigned long long)S0 * NS, (unsigned long long)S0 * NS * mp.bits);
}

constexpr size_t kIaglScratchMax = (size_t)1 << 30;     // H, starts, solutions and records of one slice
constexpr uint64_t kIaglSliceMax = 1ull << 18;

struct IaglOut {
    uint32_t *sym, *bit, *ssym, *sbit;
    int32_t* ns;
    double *sinr, *cap;
    uint32_t* iters;
    void *bigH, *F_init, *F, *U;
};

template <typename T>
static int launch_run_ia_general(mcle_ctx* ctx, const mcle_ia_general_cfg* cfg, const IaglShape& sh, int demod_method,
                                 uint64_t seed, uint64_t first, uint64_t count, mcle_counters* d_counters, const IaglOut& o) {
    const int K = cfg->K, D = sh.D;
    const ModemParams<T> mp = pipe_modem<T>(ctx, demod_method);
    const size_t hn = (size_t)(K * cfg->nr) * (size_t)(K * cfg->nt), pd = (size_t)kIagUsers * D * D;
    const size_t stride = (size_t)(1 + sh.S0 * sh.S0 + sh.S0 * cfg->nr);
    const size_t per_real = (hn + 3 * pd) * sizeof(double2) + stride * sizeof(cx<T>) + ((size_t)kIagUsers * D + 1) * sizeof(double) +
                            kIagUsers * sizeof(int32_t) + 2 * sizeof(uint32_t);
    uint64_t slice = kIaglScratchMax / per_real;            // >= 37 000 at the largest geometry
    if (slice > kIaglSliceMax) slice = kIaglSliceMax;
    if (slice > count) slice = count;
    int rc;
    void* base = nullptr;
    if ((rc = ctx->scratch((size_t)slice * per_real, &base))) return rc;
    // widest elements first, so every array is aligned to its element
    double2* s_H = static_cast<double2*>(base);
    double2* s_Fi = s_H + slice * hn;
    double2* s_F = s_Fi + slice * pd;
    double2* s_U = s_F + slice * pd;
    cx<T>* s_rec = reinterpret_cast<cx<T>*>(s_U + slice * pd);
    double* s_sinr = reinterpret_cast<double*>(s_rec + slice * stride);
    double* s_cap = s_sinr + slice * kIagUsers * D;
    int32_t* s_ns = reinterpret_cast<int32_t*>(s_cap + slice);
    uint32_t* s_it = reinterpret_cast<uint32_t*>(s_ns + slice * kIagUsers);
    uint32_t* s_sk = s_it + slice;
    // dynamic LDS: the candidate grid, then each of the four wavefronts' record (at most 46 KB: S0 = 24, nr = 6, complex128)
    const size_t lds = (((size_t)mp.grid.G * mp.grid.G * sizeof(unsigned long long) + 15) & ~(size_t)15) +
                       4 * ((stride + 1) & ~(size_t)1) * sizeof(cx<T>);
    const int per_wave = 8;
    const bool pair = (sh.n_symbols & 1) == 0;
    // A unit is four chunks = 32 realizations of S0 (nr + S0) n_symbols complex multiply-adds each.  The workgroup's one flush
    // of the counters is ~54 ns of the whole chip (pipe_common.hpp); at an ESTIMATED ~1 ps of the chip per multiply-add with
    // its share of the draws (not measured), ten flushes' worth of work is 5.4e5 of them = 2^14 per realization of a unit.
    const uint64_t min_units = flush_min_units(2, 1u << 14, (uint64_t)sh.S0 * (cfg->nr + sh.S0) * (uint64_t)sh.n_symbols);
    auto copy_out = [&](void* dst, const void* src, size_t elem_bytes, uint64_t off, uint64_t m) -> hipError_t {
        if (!dst) return hipSuccess;
        return hipMemcpyAsync(static_cast<char*>(dst) + off * elem_bytes, src, m * elem_bytes, hipMemcpyDeviceToDevice, ctx->stream);
    };
    for (uint64_t off = 0; off < count; off += slice) {
        const uint64_t m = count - off < slice ? count - off : slice;
        const uint64_t draws = m * (hn + (sh.draw_start ? kIagUsers : 0));
        hipLaunchKernelGGL(k_iagl_draw, dim3((unsigned)grid_for(ctx, draws, 256, 16)), dim3(256), 0, ctx->stream, sh, seed,
                           first + off, m, s_H, s_Fi);
        MCLE_LAUNCH_CHECK();
        if (!sh.draw_start) MCLE_HIP(hipMemsetAsync(s_Fi, 0, m * pd * sizeof(double2), ctx->stream));
        if ((rc = ia_general_launch(ctx, cfg, s_H, s_Fi, s_F, s_U, s_sinr, s_cap, s_it, s_ns, s_sk, nullptr, m))) return rc;
        hipLaunchKernelGGL(k_iagl_record<T>, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, ctx->stream, sh, s_H, s_F, s_U, s_ns,
                           s_sk, s_sinr, s_rec, o.sinr ? o.sinr + off * (kIagUsers * kIaglSlots) : nullptr, m);
        MCLE_LAUNCH_CHECK();
        const unsigned grid = walk_grid(ctx, 2, m, per_wave, min_units);
        uint32_t* se = o.sym ? o.sym + off : nullptr;
        uint32_t* be = o.bit ? o.bit + off : nullptr;
        uint32_t* sse = o.ssym ? o.ssym + off * (kIagUsers * kIaglSlots) : nullptr;
        uint32_t* sbe = o.sbit ? o.sbit + off * (kIagUsers * kIaglSlots) : nullptr;
#define MCLE_IAGL_WALK(D_, P_)                                                                                            \
    do {                                                                                                                  \
        if (lds > 32 * 1024)                                                                                              \
            MCLE_HIP(hipFuncSetAttribute((const void*)k_iagl_link<T, D_, P_>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                                         (int)lds));                                                                      \
        hipLaunchKernelGGL((k_iagl_link<T, D_, P_>), dim3(grid), dim3(256), lds, ctx->stream, mp, sh, cfg->noise_var,     \
                           seed, first + off, m, per_wave, (const cx<T>*)s_rec, d_counters, se, be, sse, sbe);            \
    } while (0)
        if (D == 4) {
            if (pair) MCLE_IAGL_WALK(4, true);
            else MCLE_IAGL_WALK(4, false);
        } else {
            if (pair) MCLE_IAGL_WALK(6, true);
            else MCLE_IAGL_WALK(6, false);
        }
#undef MCLE_IAGL_WALK
        MCLE_LAUNCH_CHECK();
        MCLE_HIP(copy_out(o.bigH, s_H, hn * sizeof(double2), off, m));
        MCLE_HIP(copy_out(o.F_init, s_Fi, pd * sizeof(double2), off, m));
        MCLE_HIP(copy_out(o.F, s_F, pd * sizeof(double2), off, m));
        MCLE_HIP(copy_out(o.U, s_U, pd * sizeof(double2), off, m));
        MCLE_HIP(copy_out(o.cap, s_cap, sizeof(double), off, m));
        MCLE_HIP(copy_out(o.ns, s_ns, kIagUsers * sizeof(int32_t), off, m));
        MCLE_HIP(copy_out(o.iters, s_it, sizeof(uint32_t), off, m));
    }
    ctx->set_kernel("ia_general_link %s D%d %s", sizeof(T) == 8 ? "f64" : "f32", D, pair ? "pairs" : "single");
    return MCLE_OK;
}

}  // namespace mcle

using namespace mcle;

extern "C" {

int mcle_run_ia_general(mcle_ctx* ctx, int dtype, const mcle_ia_general_cfg* cfg, int n_symbols, int demod_method,
                        uint64_t seed, uint64_t first, uint64_t count, mcle_counters* d_counters, uint32_t* d_sym_err,
                        uint32_t* d_bit_err, uint32_t* d_stream_sym_err, uint32_t* d_stream_bit_err, int32_t* d_ns,
                        double* d_sinr, double* d_capacity, uint32_t* d_iterations, void* d_bigH, void* d_F_init, void* d_F,
                        void* d_U) {
    if (ctx) ctx->last_kernel[0] = 0;
    int rc = check_pipe(ctx, dtype, demod_method, cfg);
    if (rc) return rc;
    if ((rc = ia_general_check(cfg, true))) return rc;     // the start of MCLE_IA_INIT_GIVEN is drawn here
    MCLE_REQUIRE(n_symbols >= 1, "n_symbols must be positive");
    IaglShape sh;
    sh.K = cfg->K, sh.nr = cfg->nr, sh.nt = cfg->nt, sh.D = ia_general_capacity(cfg);
    sh.S0 = 0;
    for (int k = 0; k < kIagUsers; ++k) {
        sh.ns[k] = k < cfg->K ? cfg->ns[k] : 0;
        sh.S0 += sh.ns[k];
    }
    sh.n_symbols = n_symbols;
    sh.draw_start = cfg->initialize_with == MCLE_IA_INIT_GIVEN;
    // rows: the S0 streams' data, the K nr receive antennas' noise
    if ((rc = check_link_draws((uint64_t)(sh.S0 > cfg->K * cfg->nr ? sh.S0 : cfg->K * cfg->nr), n_symbols, count))) return rc;
    if (count == 0) return MCLE_OK;
    if ((rc = ctx->bind())) return rc;
    const IaglOut o{d_sym_err, d_bit_err, d_stream_sym_err, d_stream_bit_err, d_ns, d_sinr, d_capacity, d_iterations,
                    d_bigH,    d_F_init,  d_F,              d_U};
    return dtype == MCLE_F32 ? launch_run_ia_general<float>(ctx, cfg, sh, demod_method, seed, first, count, d_counters, o)
                             : launch_run_ia_general<double>(ctx, cfg, sh, demod_method, seed, first, count, d_counters, o);
}

}  // extern "C"
