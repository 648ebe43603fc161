// mimo_large_link.hpp -- what the two large-array Blast links share (pipeline_mimo_large.hip: perfect channel state;
// pipeline_mimo_large_pilot.hip: pilot-estimated next to perfect): the filter build and the record writer of their set-up kernels
// and the whole body of their walk.  The pilot link's block 1 has to BE the large link realization by realization in either
// arithmetic (tests/test_gpu_large_pilot.py); it is, because both run the code below.
#pragma once
#include "cb_tile.hpp"
#include "link_walk.hpp"
#include "mimo_large_map.hpp"
#include "modem.hpp"
#include "philox.hpp"
#include "totals.hpp"
#include "wave_draws.hpp"

namespace mcle {

constexpr int kLargeSlots = kLargeMaxNt + kLargeMaxNr;     // columns of [A | G] in LDS: A at 0 .. 7, G at 8 .. 23

// The Blast filter of the channel whose rows lie in s_src (lane j of a row of 16 lanes holds its own row in `own`), into s_m: the
// Gram matrix s_src^H s_src + nv I summed over the receive antennas in ascending order from LDS (a broadcast read: all 16 lanes
// hold bitwise the same matrix), its Cholesky factor in place -- that of blast_filter_t with its positive-definiteness test --,
// lane j's own column G[:, j] at column kLargeMaxNt + j, then A = G H / sqrt(Nt) at columns 0 .. NT - 1 with H from s_true, in the
// association of k_mimo_flat_setup.  s_src must be visible to the row's lanes on entry; every thread of the workgroup calls it
// (two barriers).  False: not positive definite; the filter is zeros then, not NaNs, and the link skips the realization.
template <int NT>
__device__ __forceinline__ bool large_filter(const double2 (*s_src)[NT], const double2 (*s_true)[NT], const double2 (&own)[NT],
                                             double2 (*s_m)[kLargeSlots], int nr, double filter_nv, int j) {
    const double2 zero = mk<double>(0, 0);
    // L: the Gram matrix (lower triangle), then its Cholesky factor in place
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

// The records of the wavefront's four realizations from s_m [set][realization][stream][A | G]: SETS records per realization,
// each 64 values per K-step in the link's operand order (mimo_large_entry) and arithmetic, set `set` of realization r2 at
// (r2 * SETS + set) * 64 * steps.  After large_filter's last barrier.
template <int NT, int SETS>
__device__ __forceinline__ void large_write_records(const double2 (*s_m)[4][NT][kLargeSlots], int nr, int f64, uint64_t count,
                                                    void* __restrict__ recs, int lane) {
    const int steps = mimo_large_steps(NT, nr);
    for (int ww = 0; ww < 4; ++ww) {
        const uint64_t r2 = (uint64_t)blockIdx.x * 4 + ww;
        if (r2 >= count) break;
        for (int set = 0; set < SETS; ++set) {
            const size_t base = ((size_t)r2 * SETS + (size_t)set) * (size_t)(64 * steps);
            for (int s = 0; s < steps; ++s) {
                const MimoLargeEntry en = mimo_large_entry(f64 != 0, NT, nr, s, lane);
                double v = 0.0;
                if (en.src != LARGE_ZERO) {
                    const double2 m = s_m[set][ww][en.i][en.src == LARGE_A ? en.col : kLargeMaxNt + en.col];
                    v = (en.part ? m.y : m.x) * (double)en.sign;
                }
                if (f64) reinterpret_cast<double*>(recs)[base + (size_t)(s * 64 + lane)] = v;
                else reinterpret_cast<float*>(recs)[base + (size_t)(s * 64 + lane)] = (float)v;
            }
        }
    }
}

// large_link_walk spells the input and output maps out (antenna 4 p + g of pair p, results hh and hh + 2 of stream g + 4 hh): the
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
static_assert(large_link_matches_map(), "large_link_walk and mimo_large_map.hpp disagree");

// The body of a large-array link kernel (256 threads: four independent wavefronts) for F left operands, behind the kernel's
// link_prologue: the kernel declares the constellation, the candidate grid and the Box-Muller tables and fills them, as every walk
// of link_walk.hpp does.  (With the three arrays and the prologue in here the complex128 walk for F = 2 took 0.7 % longer per call
// than before the walk was shared -- a launch is one trip of 16 realizations per wavefront, so its opening counts -- and with them
// in the kernel it does not: profiles/r28/large_walk_ab.log.)  A wavefront per chunk of per_wave realizations; per pass 32 symbol columns as two 16-column tiles (even columns in one, odd in the other: one
// Philox NOISE block, samples t and t + 1 of a receive row, serves both).  Every symbol and every noise sample is drawn once and
// multiplied into the accumulators of all F filters, filter by filter in ascending f, each filter's products in one fixed order
// -- so the counts of a filter do not depend on how many others ride along.  Realization rl has F records of
// 64 * mimo_large_steps values at recs + rl * F * that, and one flag word (0: skipped).  Filter f books into counters + f and
// sym[f], bit[f]; one flush phase per filter, in ascending f.
template <typename T, int F>
__device__ __forceinline__ void large_link_walk(const ModemParams<T>& mp, int nt, int nr, int n_symbols, double noise_var, uint64_t seed,
                                                uint64_t first, uint64_t count, int per_wave, const T* __restrict__ recs,
                                                const uint32_t* __restrict__ flags, mcle_counters* counters,
                                                uint32_t* const (&sym)[F], uint32_t* const (&bit)[F], const cx<T>* s_table,
                                                const unsigned long long* s_grid, const double* s_bm) {
    using Tile = CbTile<T>;
    using Acc = typename Tile::acc;
    const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const T sigma = (T)sqrt(noise_var);
    const uint32_t mask = (uint32_t)(mp.M - 1);
    const int ps = mimo_large_sym_pairs(nt), pn = mimo_large_noise_pairs(nr);
    const size_t set_len = (size_t)64 * (size_t)(2 * (ps + pn));
    __shared__ WgTotals totals_all[F][4];                  // [filter][wavefront]
    if (lane == 0) {
#pragma unroll
        for (int f = 0; f < F; ++f) wg_zero(totals_all[f][wv]);
    }
    __syncthreads();
    const uint64_t n_chunks = (count + per_wave - 1) / per_wave;
    for (uint64_t ch = (uint64_t)blockIdx.x * 4 + wv; ch < n_chunks; ch += (uint64_t)gridDim.x * 4) {
        const uint64_t r_end = (ch + 1) * per_wave < count ? (ch + 1) * per_wave : count;
        for (uint64_t rl = ch * per_wave; rl < r_end; ++rl) {
            const Rng rng(seed, first + rl);
            const T* rec = recs + rl * F * set_len + lane;
            // the left operands: one value per lane, K-step and filter (symbol steps, then noise steps)
            T as[F][4], an[F][8];
#pragma unroll
            for (int f = 0; f < F; ++f) {
#pragma unroll
                for (int s = 0; s < 4; ++s) as[f][s] = s < 2 * ps ? rec[f * set_len + s * 64] : (T)0;
#pragma unroll
                for (int s = 0; s < 8; ++s) an[f][s] = s < 2 * pn ? rec[f * set_len + (2 * ps + s) * 64] : (T)0;
            }
            unsigned se[F], be[F];
#pragma unroll
            for (int f = 0; f < F; ++f) se[f] = be[f] = 0u;
            for (int t0 = 0; t0 < n_symbols; t0 += 32) {
                const int t = t0 + 2 * n;                 // this lane's column of the even tile; t + 1 in the odd one
                Acc acc0[F], acc1[F];
#pragma unroll
                for (int f = 0; f < F; ++f) acc0[f] = acc1[f] = Acc{0, 0, 0, 0};
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
                        for (int f = 0; f < F; ++f) {
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
                        for (int f = 0; f < F; ++f) {
                            acc0[f] = Tile::mma(an[f][2 * p], z0.x, acc0[f]);
                            acc1[f] = Tile::mma(an[f][2 * p], z1.x, acc1[f]);
                            acc0[f] = Tile::mma(an[f][2 * p + 1], z0.y, acc0[f]);
                            acc1[f] = Tile::mma(an[f][2 * p + 1], z1.y, acc1[f]);
                        }
                    }
                // result h + 2 part of the lane: part of stream g + 4 h (mimo_large_output), of every filter
#pragma unroll
                for (int f = 0; f < F; ++f)
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
#pragma unroll
            for (int f = 0; f < F; ++f) link_account(totals_all[f][wv], se[f], be[f], skipped, rl, lane, sym[f], bit[f]);
        }
    }
    const unsigned long long n_sym = (unsigned long long)nt * n_symbols;
#pragma unroll
    for (int f = 0; f < F; ++f) wg_flush_waves<4>(totals_all[f], counters ? counters + f : nullptr, n_sym, n_sym * mp.bits);
}

}  // namespace mcle
