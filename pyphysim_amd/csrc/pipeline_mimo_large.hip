// pipeline_mimo_large.hip -- the flat Blast link of pipeline_mimo_flat.hip (apps/mimo/simulate_mimo.py:68-142, mimo.Blast
// mimo/mimo.py:463-660; Nt = 1 is mimo.MRC :789-830) for arrays beyond 4 x 4: 1 <= Nt <= 8, Nt <= Nr <= 16.  Per realization
// H = randn_c(Nr, Nt), X = reshape(symbols, (Nt, -1), 'F') / sqrt(Nt), Y = H X + sqrt(noise_var) N, est = G Y with
// G = sqrt(Nt) (H^H H + nv I)^-1 H^H (nv = noise_var with mmse, else 0: zero forcing), demodulate, count.
// Draw ledger (mcle-philox-v1), the flat kernel's: CHAN sample r*Nt + a = H[r][a]; DATA symbol n = t*Nt + a; NOISE sample
// r*NSymbs + t.
//
// The 4 x 4 walk keeps A = G H / sqrt(Nt) and G wave-uniform in scalar registers; at 8 x 16 that is 192 complex values and does not
// fit.  Here est = A x + G n for 16 symbol columns is one real product on the matrix cores (mimo_large_map.hpp: the operand maps):
// the left operand costs a lane ONE value per K-step, at most 12.
//
// Two launches, both from what this link shares with pipeline_mimo_large_pilot.hip (mimo_large_link.hpp).  k_mimo_large_setup
// (always f64, mimo.hpp argues why): one realization per row of 16 lanes, lane r draws and owns row r of H and parks it in LDS;
// large_filter builds G and A = G H / sqrt(Nt) there, large_write_records writes the wavefront's four records in the link's
// operand order and arithmetic.  k_mimo_large_link: large_link_walk with one left operand.
#include "mimo_large_link.hpp"
#include "pipe_common.hpp"

namespace mcle {

template <int NT>
__global__ __launch_bounds__(64) void k_mimo_large_setup(int nr, double filter_nv, uint64_t seed, uint64_t first, uint64_t count,
                                                         int f64, void* __restrict__ recs, uint32_t* __restrict__ flags) {
    __shared__ double2 s_h[4][kLargeMaxNr][NT];             // [realization of the wavefront][r][a]
    __shared__ double2 s_m[1][4][NT][kLargeSlots];          // [one set][realization][stream][A | G]
    const int lane = threadIdx.x, w = lane >> 4, j = lane & 15;
    const uint64_t rl = (uint64_t)blockIdx.x * 4 + w;
    const bool live = rl < count;
    const Rng rng(seed, first + rl);
    double2 h[NT];
#pragma unroll
    for (int a = 0; a < NT; ++a) {
        h[a] = (live && j < nr) ? cn_sample<double>(rng, STREAM_CHAN, (uint64_t)(j * NT + a), 1.0) : mk<double>(0, 0);
        s_h[w][j][a] = h[a];
    }
    __syncthreads();
    // a realization that is not positive definite is marked and skipped by the link
    const bool ok = large_filter<NT>(s_h[w], s_h[w], h, s_m[0][w], nr, filter_nv, j);
    if (live && j == 0) flags[rl] = ok ? 1u : 0u;
    large_write_records<NT, 1>(s_m, nr, f64, count, recs, lane);
}

template <typename T>
__global__ __launch_bounds__(256, sizeof(T) == 4 ? 3 : 2) void k_mimo_large_link(
    ModemParams<T> mp, int nt, int nr, int n_symbols, double noise_var, uint64_t seed, uint64_t first, uint64_t count,
    int per_wave, const T* __restrict__ recs, const uint32_t* __restrict__ flags, mcle_counters* counters,
    uint32_t* __restrict__ sym_out, uint32_t* __restrict__ bit_out) {
    uint32_t* const sym[1] = {sym_out};
    uint32_t* const bit[1] = {bit_out};
    __shared__ cx<T> s_table[256];
    extern __shared__ unsigned long long s_grid[];       // [G*G] candidate grid (min-distance demodulation)
    __shared__ double s_bm[sizeof(T) == 8 ? kBmLdsDoubles : 1];   // complex128 Box-Muller tables (bm_f64.hpp)
    link_prologue(mp, s_table, nullptr, s_grid, s_bm);     // (no lockstep table: demod_one per stream)
    large_link_walk<T, 1>(mp, nt, nr, n_symbols, noise_var, seed, first, count, per_wave, recs, flags, counters, sym, bit, s_table,
                          s_grid, s_bm);
}

template <typename T>
static int run_mimo_large(mcle_ctx* ctx, const mcle_mimo_large_cfg* cfg, uint64_t seed, uint64_t first, uint64_t count,
                          mcle_counters* d_counters, uint32_t* d_sym_err, uint32_t* d_bit_err) {
    const int nt = cfg->nt, nr = cfg->nr, steps = mimo_large_steps(nt, nr);
    const double filter_nv = cfg->mmse ? cfg->noise_var : 0.0;
    const int per_wave = 16;
    const ModemParams<T> mp = pipe_modem<T>(ctx, cfg->demod_method);
    const size_t lds = (size_t)mp.grid.G * mp.grid.G * sizeof(unsigned long long);
    // record: 64 values of the link's arithmetic per K-step, then one flag word -- at most 6 KiB per realization (8 x 16,
    // complex128), so the slice is sized by bytes: at most 128 MiB of records
    const size_t rec_bytes = (size_t)mimo_large_record_len(nt, nr) * sizeof(T);
    const uint64_t k_slice = (((uint64_t)128 << 20) / rec_bytes) & ~(uint64_t)3;
    const uint64_t slice = count < k_slice ? count : k_slice;
    int rc = launch_sliced(
        ctx, first, count, k_slice, rec_bytes, d_sym_err, d_bit_err,
        [&](void* recs, uint64_t at, uint64_t m) {
            uint32_t* flags = reinterpret_cast<uint32_t*>(static_cast<char*>(recs) + (size_t)slice * rec_bytes);
            const unsigned sgrid = (unsigned)((m + 3) / 4);
#define MCLE_LS(NT_)                                                                                                             \
    case NT_:                                                                                                                    \
        hipLaunchKernelGGL(k_mimo_large_setup<NT_>, dim3(sgrid), dim3(64), 0, ctx->stream, nr, filter_nv, seed, at, m,           \
                           (int)(sizeof(T) == 8), recs, flags);                                                                  \
        break;
            switch (nt) {
                MCLE_LS(1) MCLE_LS(2) MCLE_LS(3) MCLE_LS(4) MCLE_LS(5) MCLE_LS(6) MCLE_LS(7) MCLE_LS(8)
            }
#undef MCLE_LS
        },
        [&](void* recs, uint64_t at, uint64_t m, uint32_t* se, uint32_t* be) {
            const uint32_t* flags = reinterpret_cast<const uint32_t*>(static_cast<char*>(recs) + (size_t)slice * rec_bytes);
            hipLaunchKernelGGL(k_mimo_large_link<T>, dim3(walk_grid(ctx, sizeof(T) == 4 ? 3 : 2, m, per_wave)), dim3(256), lds, ctx->stream,
                               mp, nt, nr, cfg->n_symbols, cfg->noise_var, seed, at, m, per_wave, (const T*)recs, flags, d_counters, se,
                               be);
        },
        sizeof(uint32_t));
    if (rc) return rc;
    ctx->set_kernel("mimo_large_link %s %dx%d s%d", sizeof(T) == 8 ? "f64" : "f32", nr, nt, steps);
    return MCLE_OK;
}

}  // namespace mcle

using namespace mcle;

extern "C" int mcle_run_mimo_large(mcle_ctx* ctx, int dtype, const mcle_mimo_large_cfg* cfg, uint64_t seed, uint64_t first,
                                   uint64_t count, mcle_counters* d_counters, uint32_t* d_sym_err, uint32_t* d_bit_err) {
    if (ctx) ctx->last_kernel[0] = 0;
    int rc = check_pipe(ctx, dtype, cfg ? cfg->demod_method : 0, cfg);
    if (rc) return rc;
    const int nt = cfg->nt, nr = cfg->nr;
    MCLE_REQUIRE(nt >= 1 && nt <= kLargeMaxNt && nr >= nt && nr <= kLargeMaxNr,
                 "antenna counts must satisfy 1 <= nt <= %d, nt <= nr <= %d (got nt %d, nr %d)", kLargeMaxNt, kLargeMaxNr, nt, nr);
    MCLE_REQUIRE(cfg->n_symbols >= 1, "n_symbols must be positive");
    MCLE_REQUIRE(cfg->noise_var >= 0.0 && cfg->noise_var <= 1.79e308, "Noise variance must be a non-negative value.");
    MCLE_REQUIRE(cfg->mmse == 0 || cfg->mmse == 1, "mmse must be 0 or 1 (got %d)", cfg->mmse);
    MCLE_REQUIRE(cfg->reserved == 0, "reserved must be 0");
    if ((rc = check_link_draws((uint64_t)nr, cfg->n_symbols, count))) return rc;
    if (count == 0) return MCLE_OK;
    if ((rc = ctx->bind())) return rc;
    return dtype == MCLE_F32 ? run_mimo_large<float>(ctx, cfg, seed, first, count, d_counters, d_sym_err, d_bit_err)
                             : run_mimo_large<double>(ctx, cfg, seed, first, count, d_counters, d_sym_err, d_bit_err);
}
