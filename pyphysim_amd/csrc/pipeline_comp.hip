// pipeline_comp.hip -- the fused CoMP link with an external interferer and per-realization stream reduction.
//
// Reference: apps/comp_BD/simulate_comp.py:311-621 (_run_simulation, __simulate_for_one_metric) and its script form
// simulate_comp_with_ext_int_simple.py; comm/blockdiagonalization.py:666-1469 (WhiteningBD, EnhancedBD);
// channels/multiuser.py:2011-2807 (MultiUserChannelMatrixExtInt: big_H, path loss, corrupt_concatenated_data,
// calc_JP_SINR); modulators/fundamental.py (calcTheoreticalBER / PER of PSK, BPSK, QAM).
//
// Two launches, the shape of mcle_run_bd (kernels_bd.hip): k_comp_solve_links -- one lane per realization, f64 for
// either dtype -- draws big_H [K r][K r + n_ext] with its path loss, runs the variant through bd_extint_lane (the body
// the operator k_bd_extint runs), choosing every user's stream count inside the lane for 'capacity' and
// 'effective_throughput', and writes one record per realization; k_comp_link walks the records' symbol columns.
//
// Record (cx<T>, stride n (1 + R + n_ext) + 1 + K, n = K R, stream slot s = k R + j, all zero on an inactive slot):
//   [0, n)                 d_s = (W_k H_k MsPk_k)_jj
//   [n, n + n R)           W_s: the R entries of the stream's filter row
//   [.., + n n_ext)        g_{s,e} = sqrt(pe) (W_k H_ext,k)_{j,e}
//   [..]                   (1 | 0: numerically singular channel, 0)
//   [.., + K)              (stream count of user k, 0)
// Only the diagonal of D_k = W_k H_k MsPk_k is carried.  W_k = pinv(A) B with B H_k MsPk_k = A of full column rank in every
// variant (A = the whitened equivalent channel, or Pbar Heq_red), so D_k = pinv(A) A = I up to rounding, and the other
// users' streams arrive through an exact null (H_k MsPk_l = 0, l != k): what is dropped is <= ~1e-15 of a symbol, the
// argument k_bd_link makes for plain block diagonalisation.
#include "modem.hpp"
#include "philox.hpp"
#include "pipe_common.hpp"
#include "totals.hpp"
#include "wave_draws.hpp"
#include "link_walk.hpp"
#include "bd_extint.hpp"

namespace mcle {

constexpr int kCompMaxExt = 8;

struct CompParams {
    int K, r, n_ext, n_symbols;
    int method, metric, num_streams, packet_length;
    int mod_kind, M, bits;          // the context's constellation: the BER closed form of 'effective_throughput'
    double iPu, noise_var, pe, sinr_pe;
    double root_pl[16], root_pl_ext[32];
};

// Kb (1 - PER) of one stream at linear SINR s: PER = 1 - (1 - BER)^packet_length, BER the modulator's closed form
// (fundamental.py: PSK 2 Q(sqrt(2 s) sin(pi / M)) / Kb, BPSK Q(sqrt(2 s)), square QAM 2 P_sc / Kb with
// P_sc = 2 (1 - 1 / sqrt(M)) Q(sqrt(3 s / (M - 1)))); Q(x) = erfc(x / sqrt(2)) / 2
__device__ __forceinline__ double comp_stream_throughput(const CompParams& pp, double s) {
    auto qf = [](double x) { return 0.5 * erfc(x / 1.4142135623730951); };
    double ber;
    if (pp.mod_kind == MCLE_CONST_BPSK) {
        ber = qf(sqrt(2.0 * s));
    } else if (pp.mod_kind == MCLE_CONST_QAM) {
        const double psc = 2.0 * (1.0 - 1.0 / sqrt((double)pp.M)) * qf(sqrt(s * 3.0 / ((double)pp.M - 1.0)));
        ber = (2.0 * psc) / (double)pp.bits;
    } else {
        const double ser = 2.0 * qf(sqrt(2.0 * s) * sin(3.141592653589793 / (double)pp.M));
        ber = 1.0 / (double)pp.bits * ser;
    }
    const double per = 1.0 - pow(1.0 - ber, (double)pp.packet_length);
    return (double)pp.bits * (1.0 - per);
}

// pl (may be NULL): [count][K][K + n_ext] per-realization path loss (rx user; tx users, then interferer antennas);
// ns_out [count][K], sinr_out [count][K R] (may be NULL)
template <typename T, int R>
__global__ __launch_bounds__(64) void k_comp_solve_links(CompParams pp, uint64_t seed, uint64_t first, uint64_t count,
                                                         const double* __restrict__ pl, cx<T>* __restrict__ recs,
                                                         int32_t* __restrict__ ns_out, double* __restrict__ sinr_out) {
    const uint64_t rl = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (rl >= count) return;
    const int K = pp.K, n = K * R, E = pp.n_ext, cols = n + E;
    const int stride = n * (1 + R + E) + 1 + K;
    const Rng rng(seed, first + rl);
    cd Hb[kBdMaxN * (kBdMaxN + kCompMaxExt)];
    for (int i = 0; i < n; ++i) {
        const int k = i / R;
        const double* plk = pl ? pl + (rl * K + k) * (size_t)(K + E) : nullptr;
        for (int c = 0; c < n; ++c) {
            const cd h = cn_sample<double>(rng, STREAM_CHAN, (uint64_t)(i * n + c), 1.0);
            Hb[i * cols + c] = cscale(h, plk ? sqrt(plk[c / R]) : pp.root_pl[k * K + c / R]);
        }
        for (int e = 0; e < E; ++e) {
            const cd h = cn_sample<double>(rng, STREAM_CHAN, (uint64_t)(n * n + i * E + e), 1.0);
            Hb[i * cols + n + e] = cscale(h, plk ? sqrt(plk[K + e]) : pp.root_pl_ext[k * E + e]);
        }
    }
    BdExtParams bp;
    bp.K = K;
    bp.r = R;
    bp.n_ext = E;
    bp.method = pp.method;
    bp.metric = pp.metric;
    bp.num_streams = pp.num_streams;
    for (int k = 0; k < 4; ++k) bp.ns_user[k] = 0;
    bp.iPu = pp.iPu;
    bp.nv = pp.noise_var;
    bp.pe = pp.pe;
    cd Mf[kBdMaxN * kBdMaxN], Wf[kBdMaxN * R];      // the chosen precoder columns / filter rows by stream slot
    int nsu[4] = {0, 0, 0, 0};
    for (int e = 0; e < n * n; ++e) Mf[e] = mk<double>(0, 0);
    for (int e = 0; e < n * R; ++e) Wf[e] = mk<double>(0, 0);
    auto emit = [&](int k, const cd* MsPk, const cd* W, int ns) {
        for (int m = 0; m < n; ++m)
            for (int c = 0; c < ns; ++c) Mf[m * n + k * R + c] = MsPk[m * ns + c];
        for (int i = 0; i < ns; ++i)
            for (int a = 0; a < R; ++a) Wf[(k * R + i) * R + a] = W[i * R + a];
        nsu[k] = ns;
    };
    auto value_of = [&](double sinr) {
        return pp.metric == 3 ? log2(1.0 + sinr) : comp_stream_throughput(pp, sinr);
    };
    const bool ok = bd_extint_lane(bp, Hb, emit, value_of, nullptr);

    cx<T>* rec = recs + rl * stride;
    const double root_pe = sqrt(pp.pe);
    for (int k = 0; k < K; ++k) {
        cd HM[R * kBdMaxN];                          // H_k [Ms P_0 .. Ms P_{K-1}]: every stream's signal at user k's antennas
        for (int a = 0; a < R; ++a)
            for (int s = 0; s < n; ++s) {
                cd acc = mk<double>(0, 0);
                for (int m = 0; m < n; ++m) acc = cadd(acc, cmul(Hb[(k * R + a) * cols + m], Mf[m * n + s]));
                HM[a * n + s] = acc;
            }
        for (int j = 0; j < R; ++j) {
            const int s = k * R + j;
            const bool active = j < nsu[k];
            const cd* w = Wf + s * R;
            // calc_JP_SINR (multiuser.py:1901-2008, :2744-2807) with interferer power sinr_pe
            cd d = mk<double>(0, 0);
            double desired = 0.0, other = 0.0, wn2 = 0.0, ext = 0.0;
            for (int sp = 0; sp < n; ++sp) {
                cd t = mk<double>(0, 0);
                for (int a = 0; a < R; ++a) t = cadd(t, cmul(w[a], HM[a * n + sp]));
                if (sp == s) {
                    d = t;
                    desired = bd_abs2(t);
                } else {
                    other += bd_abs2(t);
                }
            }
            for (int a = 0; a < R; ++a) wn2 += bd_abs2(w[a]);
            for (int e = 0; e < E; ++e) {
                cd t = mk<double>(0, 0);
                for (int a = 0; a < R; ++a) t = cadd(t, cmul(w[a], Hb[(k * R + a) * cols + n + e]));
                ext += bd_abs2(t);
                const cd g = cscale(t, root_pe);
                rec[n + n * R + s * E + e] = mk<T>((T)g.x, (T)g.y);
            }
            rec[s] = mk<T>((T)d.x, (T)d.y);
            for (int a = 0; a < R; ++a) rec[n + s * R + a] = mk<T>((T)w[a].x, (T)w[a].y);
            if (sinr_out)
                sinr_out[rl * n + s] = active ? desired / (other + pp.sinr_pe * ext + pp.noise_var * wn2) : 0.0;
        }
        rec[n * (1 + R + E) + 1 + k] = mk<T>((T)nsu[k], (T)0);
        if (ns_out) ns_out[rl * K + k] = nsu[k];
    }
    rec[n * (1 + R + E)] = mk<T>(ok ? (T)1 : (T)0, (T)0);
}

// The symbol walk: workgroups of four independent wavefronts, each taking chunks of per_wave realizations; the lanes
// of a wavefront take the symbol columns of one realization -- two adjacent columns each where n_symbols is even (the
// two samples of one Philox block per noise / interferer draw, the data blocks shared across the wave), one otherwise.
// est_s = d_s x + sum_e g_{s,e} z_e + W_s . (sigma n_user), demodulate, count per stream.
// PAIR: n_symbols even.  R = antennas per user (every register index below is static).
template <typename T, int R, bool PAIR>
__global__ __launch_bounds__(256) void k_comp_link(ModemParams<T> mp, CompParams pp, uint64_t seed, uint64_t first,
                                                   uint64_t count, int per_wave, const cx<T>* __restrict__ recs,
                                                   mcle_counters* counters, uint32_t* __restrict__ sym_out,
                                                   uint32_t* __restrict__ bit_out, uint32_t* __restrict__ ssym_out,
                                                   uint32_t* __restrict__ sbit_out) {
    constexpr int KMAX = (kBdMaxN / R) < 4 ? (kBdMaxN / R) : 4, NMAX = KMAX * R;
    constexpr int COLS = PAIR ? 2 : 1;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int K = pp.K, n = K * R, E = pp.n_ext;
    const int stride = n * (1 + R + E) + 1 + K;
    unsigned long long* s_grid = reinterpret_cast<unsigned long long*>(smem);
    __shared__ cx<T> s_table[256];
    __shared__ WgTotals totals_all[4];
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    WgTotals& totals = totals_all[wv];
    __shared__ double s_bm[sizeof(T) == 8 ? kBmLdsDoubles : 1];   // complex128 Box-Muller tables (bm_f64.hpp)
    link_prologue(mp, s_table, nullptr, s_grid, s_bm);     // (no lockstep table: demod_one per stream)
    const int lane = threadIdx.x & 63;
    const T sigma = (T)sqrt(pp.noise_var);
    const uint32_t mask = (uint32_t)(mp.M - 1);
    const uint32_t NS = (uint32_t)pp.n_symbols;
    if (lane == 0) wg_zero(totals);
    __syncthreads();
    const uint64_t n_chunks = (count + per_wave - 1) / per_wave;
    for (uint64_t ch = (uint64_t)blockIdx.x * 4 + wv; ch < n_chunks; ch += (uint64_t)gridDim.x * 4) {
        const uint64_t r_end = (ch + 1) * per_wave < count ? (ch + 1) * per_wave : count;
        for (uint64_t rl = ch * per_wave; rl < r_end; ++rl) {
            const Rng rng(seed, first + rl);
            const cx<T>* D = recs + rl * stride;     // wave-uniform record
            const cx<T>* W = D + n;
            const cx<T>* G = W + n * R;
            const cx<T>* F = G + n * E;
            const bool ok = F[0].x != (T)0;
            unsigned se[NMAX], be[NMAX];
#pragma unroll
            for (int s = 0; s < NMAX; ++s) se[s] = be[s] = 0u;
            int q_all = 0;                           // active streams of the realization
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
                if (k < K) q_all += (int)F[1 + k].x;
            for (uint32_t t0 = 0; t0 < NS; t0 += 64u * COLS) {
                const uint32_t t = t0 + (uint32_t)COLS * (uint32_t)lane;
                // PAIR: the symbols of every active stream for this lane's two columns, the Philox blocks shared across the
                // wave (wave_draws.hpp; every lane takes part, so before the ragged last pass drops lanes)
                int ta[NMAX], tb[NMAX];
                if constexpr (PAIR) wave_symbol_pairs<NMAX>(rng, q_all, NS, t0, mask, lane, ta, tb);
                if (t >= NS) continue;
                cx<T> ze[COLS][kCompMaxExt];         // the interferers' symbols: sqrt(pe) CN(0, 1), STREAM_PHASE
#pragma unroll
                for (int e = 0; e < kCompMaxExt; ++e)
                    if (e < E) {
                        if constexpr (PAIR)
                            cn_pair_lds(rng, STREAM_PHASE, ((uint32_t)e * NS + t) >> 1, (T)1, ze[0][e], ze[COLS - 1][e], s_bm);
                        else
                            ze[0][e] = cn_one_lds(rng, STREAM_PHASE, (uint32_t)e * NS + t, (T)1, s_bm);
                    }
                int q0 = 0;                          // active streams before this user
#pragma unroll
                for (int k = 0; k < KMAX; ++k)
                    if (k < K) {
                        const int nsk = (int)F[1 + k].x;
                        cx<T> nz[COLS][R];
#pragma unroll
                        for (int a = 0; a < R; ++a) {
                            if constexpr (PAIR)
                                cn_pair_lds(rng, STREAM_NOISE, ((uint32_t)(k * R + a) * NS + t) >> 1, sigma, nz[0][a],
                                            nz[COLS - 1][a], s_bm);
                            else
                                nz[0][a] = cn_one_lds(rng, STREAM_NOISE, (uint32_t)(k * R + a) * NS + t, sigma, s_bm);
                        }
#pragma unroll
                        for (int jj = 0; jj < R; ++jj)
                            if (jj < nsk) {
                                const int s = k * R + jj;
                                const int q = q0 + jj;                // the stream's number among the active ones (wave-uniform)
                                int tx[COLS];
                                if constexpr (PAIR) {
                                    tx[0] = ta[0];
                                    tx[COLS - 1] = tb[0];
#pragma unroll
                                    for (int qq = 1; qq < NMAX; ++qq)         // (selects: a run-time index would park ta / tb in scratch)
                                        if (qq == q) {
                                            tx[0] = ta[qq];
                                            tx[COLS - 1] = tb[qq];
                                        }
                                } else {
                                    tx[0] = (int)symbol_at(rng, (uint32_t)q * NS + t, mask);
                                }
#pragma unroll
                                for (int c = 0; c < COLS; ++c) {
                                    cx<T> est = cmul(D[s], s_table[tx[c]]);
#pragma unroll
                                    for (int e = 0; e < kCompMaxExt; ++e)
                                        if (e < E) est = cfma4(G[s * E + e], ze[c][e], est);
#pragma unroll
                                    for (int a = 0; a < R; ++a) est = cfma4(W[s * R + a], nz[c][a], est);
                                    const unsigned x = (unsigned)(tx[c] ^ demod_one(mp, s_table, s_grid, est));
                                    se[s] += (x != 0u);
                                    be[s] += __popc(x);
                                }
                            }
                        q0 += nsk;
                    }
            }
            unsigned se_all = 0, be_all = 0;
#pragma unroll
            for (int s = 0; s < NMAX; ++s)
                if (s < n) {
                    const unsigned a = wave_sum_u32(se[s]), b = wave_sum_u32(be[s]);
                    se_all += a;
                    be_all += b;
                    if (lane == 0) {
                        if (ssym_out) ssym_out[rl * n + s] = ok ? a : 0xFFFFFFFFu;
                        if (sbit_out) sbit_out[rl * n + s] = ok ? b : 0xFFFFFFFFu;
                    }
                }
            if (lane == 0) wg_account(totals, se_all, be_all, !ok, rl, sym_out, bit_out);
        }
    }
    wg_flush_waves<4>(totals_all, counters, (unsigned long long)n * NS, (unsigned long long)n * NS * mp.bits);
}

template <typename T, int R>
static int launch_run_comp(mcle_ctx* ctx, const mcle_comp_cfg* cfg, const CompParams& pp, uint64_t seed, uint64_t first,
                           uint64_t count, const double* d_pathloss, mcle_counters* d_counters, uint32_t* d_sym_err,
                           uint32_t* d_bit_err, uint32_t* d_stream_sym_err, uint32_t* d_stream_bit_err, int32_t* d_ns,
                           double* d_sinr) {
    const int K = cfg->K, n = K * R, E = cfg->n_ext;
    const ModemParams<T> mp = pipe_modem<T>(ctx, cfg->demod_method);
    const uint64_t kSlice = 1ull << 18;          // realizations per solve + walk pair: bounds the record buffer
    const size_t stride = (size_t)(n * (1 + R + E) + 1 + K);
    const size_t lds = (size_t)mp.grid.G * mp.grid.G * sizeof(unsigned long long);
    const int per_wave = 8;
    const bool pair = (cfg->n_symbols & 1) == 0;
    const int rc = launch_sliced(
        ctx, first, count, kSlice, stride * sizeof(cx<T>), d_sym_err, d_bit_err,
        [&](void* recs, uint64_t at, uint64_t m) {
            const uint64_t off = at - first;
            hipLaunchKernelGGL((k_comp_solve_links<T, R>), dim3((unsigned)((m + 63) / 64)), dim3(64), 0, ctx->stream, pp, seed, at, m,
                               d_pathloss ? d_pathloss + off * (size_t)K * (K + E) : nullptr, (cx<T>*)recs,
                               d_ns ? d_ns + off * K : nullptr, d_sinr ? d_sinr + off * n : nullptr);
        },
        [&](void* recs, uint64_t at, uint64_t m, uint32_t* se, uint32_t* be) {
            const uint64_t off = at - first;
            const unsigned grid = walk_grid(ctx, 2, m, per_wave, 2);
            uint32_t* sse = d_stream_sym_err ? d_stream_sym_err + off * n : nullptr;
            uint32_t* sbe = d_stream_bit_err ? d_stream_bit_err + off * n : nullptr;
            if (pair)
                hipLaunchKernelGGL((k_comp_link<T, R, true>), dim3(grid), dim3(256), lds, ctx->stream, mp, pp, seed, at, m, per_wave,
                                   (const cx<T>*)recs, d_counters, se, be, sse, sbe);
            else
                hipLaunchKernelGGL((k_comp_link<T, R, false>), dim3(grid), dim3(256), lds, ctx->stream, mp, pp, seed, at, m, per_wave,
                                   (const cx<T>*)recs, d_counters, se, be, sse, sbe);
        });
    if (rc) return rc;
    ctx->set_kernel("comp_link %s r%d %s", sizeof(T) == 8 ? "f64" : "f32", R, pair ? "pairs" : "single");
    return MCLE_OK;
}

}  // namespace mcle

using namespace mcle;

extern "C" {

int mcle_run_comp(mcle_ctx* ctx, int dtype, const mcle_comp_cfg* cfg, uint64_t seed, uint64_t first, uint64_t count,
                  const double* d_pathloss, mcle_counters* d_counters, uint32_t* d_sym_err, uint32_t* d_bit_err,
                  uint32_t* d_stream_sym_err, uint32_t* d_stream_bit_err, int32_t* d_ns, double* d_sinr) {
    if (ctx) ctx->last_kernel[0] = 0;
    int rc = check_pipe(ctx, dtype, cfg ? cfg->demod_method : 0, cfg);
    if (rc) return rc;
    MCLE_REQUIRE(cfg->K >= 1 && cfg->K <= 4 && cfg->r >= 1 && cfg->r <= kBdMaxR && cfg->K * cfg->r <= kBdMaxN,
                 "block diagonalisation covers up to 4 users x 4 antennas with at most %d antennas in total", kBdMaxN);
    MCLE_REQUIRE(cfg->n_ext >= 0 && cfg->n_ext <= kCompMaxExt, "at most 8 external-interference antennas");
    MCLE_REQUIRE(cfg->method == 0 || cfg->method == 1, "method: 0 = WhiteningBD, 1 = EnhancedBD");
    MCLE_REQUIRE(cfg->metric >= 0 && cfg->metric <= 4, "metric must be in [0, 4]");
    MCLE_REQUIRE(cfg->n_symbols >= 1, "n_symbols must be positive");
    MCLE_REQUIRE(cfg->iPu > 0.0, "the power per user must be positive");
    MCLE_REQUIRE(cfg->noise_var >= 0.0 && cfg->pe >= 0.0 && cfg->sinr_pe >= 0.0,
                 "noise_var, pe and sinr_pe must be non-negative");
    MCLE_REQUIRE(cfg->method == 1 || cfg->noise_var > 0.0 || cfg->n_ext >= cfg->r,
                 "whitening needs a positive definite interference-plus-noise covariance");
    if (cfg->method == 1 && (cfg->metric == 1 || cfg->metric == 2))
        MCLE_REQUIRE(cfg->num_streams >= 1 && cfg->num_streams <= cfg->r, "num_streams must be in [1, %d]", cfg->r);
    if (cfg->method == 1 && cfg->metric == 4)
        MCLE_REQUIRE(cfg->packet_length >= 1, "packet_length must be positive");
    // rows: the users' K r antennas (noise, data), the interferers' n_ext antennas (their symbols)
    if ((rc = check_link_draws((uint64_t)(cfg->K * cfg->r > cfg->n_ext ? cfg->K * cfg->r : cfg->n_ext), cfg->n_symbols, count))) return rc;
    CompParams pp;
    pp.K = cfg->K;
    pp.r = cfg->r;
    pp.n_ext = cfg->n_ext;
    pp.n_symbols = cfg->n_symbols;
    pp.method = cfg->method;
    pp.metric = cfg->method == 1 ? cfg->metric : 0;
    pp.num_streams = cfg->num_streams;
    pp.packet_length = cfg->packet_length;
    pp.mod_kind = ctx->kind;
    pp.M = ctx->M;
    pp.bits = ctx->bits;
    pp.iPu = cfg->iPu;
    pp.noise_var = cfg->noise_var;
    pp.pe = cfg->pe;
    pp.sinr_pe = cfg->sinr_pe;
    const bool static_pl = cfg->has_pathloss && !d_pathloss;
    for (int i = 0; i < 16; ++i) {
        const bool used = static_pl && i < cfg->K * cfg->K;              // [K][K] row-major: rx user, tx user
        if (used) MCLE_REQUIRE(cfg->pathloss[i] >= 0.0, "path loss must be non-negative");
        pp.root_pl[i] = used ? std::sqrt(cfg->pathloss[i]) : 1.0;
    }
    for (int i = 0; i < 32; ++i) {
        const bool used = static_pl && i < cfg->K * cfg->n_ext;          // [K][n_ext] row-major: rx user, interferer antenna
        if (used) MCLE_REQUIRE(cfg->pathloss_ext[i] >= 0.0, "path loss must be non-negative");
        pp.root_pl_ext[i] = used ? std::sqrt(cfg->pathloss_ext[i]) : 1.0;
    }
    if (count == 0) return MCLE_OK;
    if ((rc = ctx->bind())) return rc;
#define MCLE_COMP_GO(T_, R_)                                                                                              \
    return launch_run_comp<T_, R_>(ctx, cfg, pp, seed, first, count, d_pathloss, d_counters, d_sym_err, d_bit_err,        \
                                   d_stream_sym_err, d_stream_bit_err, d_ns, d_sinr)
    switch (cfg->r * 2 + (dtype == MCLE_F64)) {
        case 2: MCLE_COMP_GO(float, 1);
        case 3: MCLE_COMP_GO(double, 1);
        case 4: MCLE_COMP_GO(float, 2);
        case 5: MCLE_COMP_GO(double, 2);
        case 6: MCLE_COMP_GO(float, 3);
        case 7: MCLE_COMP_GO(double, 3);
        case 8: MCLE_COMP_GO(float, 4);
        default: MCLE_COMP_GO(double, 4);
    }
#undef MCLE_COMP_GO
}

}  // extern "C"
