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
// Two launches.  k_mimo_large_setup (always f64, mimo.hpp argues why): one realization per row of 16 lanes, lane r draws and owns
// row r of H and parks it in LDS; every lane of the row sums the Gram matrix H^H H + nv I over the receive antennas in ascending
// order from LDS (a broadcast read: all 16 lanes hold bitwise the same matrix) and factors it -- the Cholesky of blast_filter_t
// with its positive-definiteness test --, lane r solves its own column G[:, r]; A = G H / sqrt(Nt) is summed from LDS in the
// association of k_mimo_flat_setup; the wavefront then writes its four records in the link's operand order and arithmetic.
// k_mimo_large_link: a wavefront per chunk of realizations; per pass 32 symbol columns as two 16-column tiles (even columns in
// one, odd in the other: one Philox NOISE block, samples t and t + 1 of a receive row, serves both).
#include "cb_tile.hpp"
#include "mimo_large_map.hpp"
#include "modem.hpp"
#include "philox.hpp"
#include "pipe_common.hpp"
#include "totals.hpp"
#include "wave_draws.hpp"
#include "link_walk.hpp"

namespace mcle {

constexpr int kLargeSlots = kLargeMaxNt + kLargeMaxNr;     // columns of [A | G] in LDS: A at 0 .. 7, G at 8 .. 23

template <int NT>
__global__ __launch_bounds__(64) void k_mimo_large_setup(int nr, double filter_nv, uint64_t seed, uint64_t first, uint64_t count,
                                                         int f64, void* __restrict__ recs, uint32_t* __restrict__ flags) {
    __shared__ double2 s_h[4][kLargeMaxNr][NT];             // [realization of the wavefront][r][a]
    __shared__ double2 s_m[4][NT][kLargeSlots];             // [realization][stream][A | G]
    const int lane = threadIdx.x, w = lane >> 4, j = lane & 15;
    const uint64_t rl = (uint64_t)blockIdx.x * 4 + w;
    const bool live = rl < count;
    const Rng rng(seed, first + rl);
    const double2 zero = mk<double>(0, 0);
    double2 h[NT];
#pragma unroll
    for (int a = 0; a < NT; ++a) {
        h[a] = (live && j < nr) ? cn_sample<double>(rng, STREAM_CHAN, (uint64_t)(j * NT + a), 1.0) : zero;
        s_h[w][j][a] = h[a];
    }
    __syncthreads();
    // L: the Gram matrix (lower triangle), then its Cholesky factor in place
    double2 L[NT][NT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int k = 0; k <= i; ++k) L[i][k] = zero;
    for (int r = 0; r < nr; ++r) {
        double2 hr[NT];
#pragma unroll
        for (int a = 0; a < NT; ++a) hr[a] = s_h[w][r][a];
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
            double2 v = cconj(h[i]);
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
        // a realization that is not positive definite is marked and skipped by the link: its record is zeros, not NaNs
#pragma unroll
        for (int i = 0; i < NT; ++i) s_m[w][i][kLargeMaxNt + j] = (ok && j < nr) ? cscale(z[i], root_nt) : zero;
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
                for (int r = 0; r < nr; ++r) acc = cadd(acc, cmul(s_m[w][i][kLargeMaxNt + r], cscale(s_h[w][r][a], wgt)));
                s_m[w][i][a] = acc;
            }
        }
    }
    __syncthreads();
    if (live && j == 0) flags[rl] = ok ? 1u : 0u;
    const int steps = mimo_large_steps(NT, nr);
    for (int ww = 0; ww < 4; ++ww) {
        const uint64_t r2 = (uint64_t)blockIdx.x * 4 + ww;
        if (r2 >= count) break;
        const size_t base = (size_t)r2 * (size_t)(64 * steps);
        for (int s = 0; s < steps; ++s) {
            const MimoLargeEntry en = mimo_large_entry(f64 != 0, NT, nr, s, lane);
            double v = 0.0;
            if (en.src != LARGE_ZERO) {
                const double2 m = s_m[ww][en.i][en.src == LARGE_A ? en.col : kLargeMaxNt + en.col];
                v = (en.part ? m.y : m.x) * (double)en.sign;
            }
            if (f64) reinterpret_cast<double*>(recs)[base + (size_t)(s * 64 + lane)] = v;
            else reinterpret_cast<float*>(recs)[base + (size_t)(s * 64 + lane)] = (float)v;
        }
    }
}

// k_mimo_large_link spells the input and output maps out (antenna 4 p + g of pair p, results hh and hh + 2 of stream g + 4 hh): the
// same statement as mimo_large_input / mimo_large_output over the whole envelope, checked at compile time
constexpr bool large_link_matches_map() {
    for (int nt = 1; nt <= kLargeMaxNt; ++nt)
        for (int nr = nt; nr <= kLargeMaxNr; ++nr) {
            const int ps = mimo_large_sym_pairs(nt), pn = mimo_large_noise_pairs(nr);
            for (int g = 0; g < 4; ++g)
                for (int part = 0; part < 2; ++part) {
                    for (int p = 0; p < ps; ++p) {
                        const MimoLargeInput in = mimo_large_input(nt, nr, 2 * p + part, g);
                        const int a = 4 * p + g;
                        if (in.part != part || in.kind != (a < nt ? LARGE_SYMBOL : LARGE_NONE) || (a < nt && in.idx != a)) return false;
                    }
                    for (int p = 0; p < pn; ++p) {
                        const MimoLargeInput in = mimo_large_input(nt, nr, 2 * (ps + p) + part, g);
                        const int r = 4 * p + g;
                        if (in.part != part || in.kind != (r < nr ? LARGE_NOISE : LARGE_NONE) || (r < nr && in.idx != r)) return false;
                    }
                    for (int hh = 0; hh < 2; ++hh) {
                        const MimoLargeOutput o = mimo_large_output(nt, 16 * g, hh + 2 * part);
                        if (o.part != part || o.stream != (g + 4 * hh < nt ? g + 4 * hh : -1)) return false;
                    }
                }
        }
    return true;
}
static_assert(large_link_matches_map(), "k_mimo_large_link and mimo_large_map.hpp disagree");

template <typename T>
__global__ __launch_bounds__(256, sizeof(T) == 4 ? 3 : 2) void k_mimo_large_link(
    ModemParams<T> mp, int nt, int nr, int n_symbols, double noise_var, uint64_t seed, uint64_t first, uint64_t count,
    int per_wave, const T* __restrict__ recs, const uint32_t* __restrict__ flags, mcle_counters* counters,
    uint32_t* __restrict__ sym_out, uint32_t* __restrict__ bit_out) {
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
    const size_t rec_len = (size_t)64 * (size_t)(2 * (ps + pn));
    __shared__ WgTotals totals_all[4];
    WgTotals& totals = totals_all[wv];
    if (lane == 0) wg_zero(totals);
    __syncthreads();
    const uint64_t n_chunks = (count + per_wave - 1) / per_wave;
    for (uint64_t ch = (uint64_t)blockIdx.x * 4 + wv; ch < n_chunks; ch += (uint64_t)gridDim.x * 4) {
        const uint64_t r_end = (ch + 1) * per_wave < count ? (ch + 1) * per_wave : count;
        for (uint64_t rl = ch * per_wave; rl < r_end; ++rl) {
            const Rng rng(seed, first + rl);
            const T* rec = recs + rl * rec_len + lane;
            // the left operand: one value per lane and K-step (symbol steps, then noise steps)
            T as[4], an[8];
#pragma unroll
            for (int s = 0; s < 4; ++s) as[s] = s < 2 * ps ? rec[s * 64] : (T)0;
#pragma unroll
            for (int s = 0; s < 8; ++s) an[s] = s < 2 * pn ? rec[(2 * ps + s) * 64] : (T)0;
            unsigned se = 0, be = 0;
            for (int t0 = 0; t0 < n_symbols; t0 += 32) {
                const int t = t0 + 2 * n;                 // this lane's column of the even tile; t + 1 in the odd one
                Acc acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
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
                        acc0 = Tile::mma(as[2 * p], x0.x, acc0);
                        acc1 = Tile::mma(as[2 * p], x1.x, acc1);
                        acc0 = Tile::mma(as[2 * p + 1], x0.y, acc0);
                        acc1 = Tile::mma(as[2 * p + 1], x1.y, acc1);
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
                        acc0 = Tile::mma(an[2 * p], z0.x, acc0);
                        acc1 = Tile::mma(an[2 * p], z1.x, acc1);
                        acc0 = Tile::mma(an[2 * p + 1], z0.y, acc0);
                        acc1 = Tile::mma(an[2 * p + 1], z1.y, acc1);
                    }
                // result h + 2 part of the lane: part of stream g + 4 h (mimo_large_output)
#pragma unroll
                for (int hh = 0; hh < 2; ++hh)
                    if (g + 4 * hh < nt) {
                        if (t < n_symbols) {
                            const unsigned xr = (unsigned)(tx0[hh] ^ demod_one(mp, s_table, s_grid, mk<T>(acc0[hh], acc0[hh + 2])));
                            se += (xr != 0u);
                            be += __popc(xr);
                        }
                        if (t + 1 < n_symbols) {
                            const unsigned xr = (unsigned)(tx1[hh] ^ demod_one(mp, s_table, s_grid, mk<T>(acc1[hh], acc1[hh + 2])));
                            se += (xr != 0u);
                            be += __popc(xr);
                        }
                    }
            }
            link_account(totals, se, be, flags[rl] == 0u, rl, lane, sym_out, bit_out);
        }
    }
    wg_flush_waves<4>(totals_all, counters, (unsigned long long)nt * n_symbols, (unsigned long long)nt * n_symbols * mp.bits);
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
