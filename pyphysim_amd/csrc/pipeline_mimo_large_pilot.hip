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
// time (its Gram factor and row solve: pilot_block.hpp, shared with the 4 x 4 link); both filters by large_filter, the one
// k_mimo_large_setup calls (mimo_large_link.hpp), A with the TRUE channel both times (A_est = G^ H / sqrt(Nt): what the filter of
// the estimate does to the symbols that were sent).  Two records per realization in the operand order of mimo_large_entry,
// estimated then perfect, and one flag word.  k_mimo_large_pilot_link: large_link_walk with two left operands.
#include "mimo.hpp"
#include "mimo_large_link.hpp"
#include "pilot_block.hpp"
#include "pipe_common.hpp"

namespace mcle {

// one value of a 16-lane row's lane `src` to all of its lanes
__device__ __forceinline__ double2 row_bcast(double2 v, int src) {
    return mk<double>(__shfl(v.x, src, 16), __shfl(v.y, src, 16));
}

template <int NT>
__global__ __launch_bounds__(64) void k_mimo_large_pilot_setup(PilotSetup<kLargeMaxNt> p, int nr, int f64,
                                                               const double2* __restrict__ pilots, const double2* __restrict__ Lm,
                                                               const double2* __restrict__ Bm, uint64_t seed, uint64_t first,
                                                               uint64_t count, void* __restrict__ recs,
                                                               uint32_t* __restrict__ flags, double* __restrict__ err_out,
                                                               double* __restrict__ pow_out) {
    __shared__ double2 s_h[4][kLargeMaxNr][NT];             // [realization of the wavefront][r][a]: the true channel
    __shared__ double2 s_e[4][kLargeMaxNr][NT];             // W while H is formed, then the estimate
    __shared__ double2 s_m[2][4][NT][kLargeSlots];          // [estimated | perfect][realization][stream][A | G]
    __shared__ double2 s_L[kLargeMaxNr * kLargeMaxNr];      // the channel factor, once per workgroup
    __shared__ double2 s_r[4][kLargeMaxNr];                 // MMSE: R; then {err, pow} of a row's lanes
    const int lane = threadIdx.x, w = lane >> 4, j = lane & 15;
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
        double invd[NT];
        ok = pilot_gram_factor<NT>(Gm, invd);
        inv_s2 = invd[0] * invd[0];
        pilot_row_solve<NT>(Gm, invd, R, he);
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
    const bool ok_est = large_filter<NT>(s_e[w], s_h[w], he, s_m[0][w], nr, p.filter_nv, j);
    const bool ok_perf = large_filter<NT>(s_h[w], s_h[w], h, s_m[1][w], nr, p.filter_nv, j);
    ok = ok && ok_est && ok_perf;
    if (live && j == 0) flags[rl] = ok ? 1u : 0u;
    large_write_records<NT, 2>(s_m, nr, f64, count, recs, lane);
}

// The walk of k_mimo_large_link through TWO left operands (mimo_large_link.hpp): block 0 the filter of the estimate, block 1 that
// of the channel
template <typename T>
__global__ __launch_bounds__(256, sizeof(T) == 4 ? 3 : 2) void k_mimo_large_pilot_link(
    ModemParams<T> mp, int nt, int nr, int n_symbols, double noise_var, uint64_t seed, uint64_t first, uint64_t count,
    int per_wave, const T* __restrict__ recs, const uint32_t* __restrict__ flags, mcle_counters* counters,
    uint32_t* __restrict__ sym_est, uint32_t* __restrict__ bit_est, uint32_t* __restrict__ sym_perf,
    uint32_t* __restrict__ bit_perf) {
    uint32_t* const sym[2] = {sym_est, sym_perf};
    uint32_t* const bit[2] = {bit_est, bit_perf};
    __shared__ cx<T> s_table[256];
    extern __shared__ unsigned long long s_grid[];       // [G*G] candidate grid (min-distance demodulation)
    __shared__ double s_bm[sizeof(T) == 8 ? kBmLdsDoubles : 1];   // complex128 Box-Muller tables (bm_f64.hpp)
    link_prologue(mp, s_table, nullptr, s_grid, s_bm);     // (no lockstep table: demod_one per stream)
    large_link_walk<T, 2>(mp, nt, nr, n_symbols, noise_var, seed, first, count, per_wave, recs, flags, counters, sym, bit, s_table,
                          s_grid, s_bm);
}

template <typename T>
static int run_mimo_large_pilot(mcle_ctx* ctx, const mcle_mimo_pilot_cfg* cfg, const PilotSetup<kLargeMaxNt>& p, uint64_t seed,
                                uint64_t first, uint64_t count, const double* d_pilots, const double* d_L, const double* d_B,
                                mcle_counters* d_counters, uint32_t* d_sym_err, uint32_t* d_bit_err, double* d_err,
                                double* d_pow) {
    const int nt = cfg->nt, nr = cfg->nr, steps = mimo_large_steps(nt, nr);
    const int per_wave = 16;
    const ModemParams<T> mp = pipe_modem<T>(ctx, cfg->demod_method);
    const size_t lds = (size_t)mp.grid.G * mp.grid.G * sizeof(unsigned long long);
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
        hipLaunchKernelGGL(k_mimo_large_pilot_setup<NT_>, dim3(sgrid), dim3(64), 0, ctx->stream, p, nr, (int)(sizeof(T) == 8),   \
                           (const double2*)d_pilots, (const double2*)d_L, (const double2*)d_B, seed, at, m, recs, flags, e_out,  \
                           p_out);                                                                                               \
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
    const int nt = cfg->nt, nr = cfg->nr;
    MCLE_REQUIRE(nt >= 1 && nt <= kLargeMaxNt && nr >= nt && nr <= kLargeMaxNr,
                 "antenna counts must satisfy 1 <= nt <= %d, nt <= nr <= %d (got nt %d, nr %d)", kLargeMaxNt, kLargeMaxNr, nt, nr);
    if ((rc = check_pilot_cfg(cfg, d_pilots, d_mmse_matrix, count))) return rc;
    if (count == 0) return MCLE_OK;
    PilotSetup<kLargeMaxNt> p;
    if ((rc = pilot_setup_fill(ctx, cfg, d_pilots, d_counters, p))) return rc;
    return dtype == MCLE_F32
               ? run_mimo_large_pilot<float>(ctx, cfg, p, seed, first, count, d_pilots, d_chan_factor, d_mmse_matrix, d_counters,
                                             d_sym_err, d_bit_err, d_err, d_pow)
               : run_mimo_large_pilot<double>(ctx, cfg, p, seed, first, count, d_pilots, d_chan_factor, d_mmse_matrix, d_counters,
                                              d_sym_err, d_bit_err, d_err, d_pow);
}
