// kernels_codebook.hip -- chordal distances of Grassmannian codebooks and the random codebook search built on them (reference:
// subspace/metrics.py:21-113 calc_principal_angles / calc_chordal_distance_from_principal_angles, apps/find_codebook.py:73-231
// CodebookFinder._generate_*_random_codebook, calc_min_chordal_dist, find_codebook).
//
// A codebook is K precoders C_k [Nt][Ns]; Q_k is an orthonormal basis of the column space of C_k (modified Gram-Schmidt with one
// re-orthogonalisation pass, in LDS).  For a pair
//     d^2(a, b) = Ns - sum_{s, s'} |q_{a,s}^H q_{b,s'}|^2      (= sum_i sin^2 theta_i of the principal angles), clamped at 0.
// All K Ns basis vectors of a codebook are the columns of one real matrix S = [Re Q; Im Q], [2 Nt][K Ns]; with S' = [-Im Q; Re Q]
//     Re (Q^H Q) = S^T S,     Im (Q^H Q) = S'^T S,
// two real products over an inner dimension of 2 Nt <= 16 (padded to a multiple of 4) on v_mfma_f64_16x16x4_f64 /
// v_mfma_f32_16x16x4_f32.
//
// Tile map.  The ROWS of the Gram matrix are taken a strip of PB = floor(16 / Ns) precoders at a time: the A operand of strip g is
// the 16 columns of S that start at column g PB Ns (not a multiple of 16 when Ns = 3), so that no precoder's Ns rows are split
// between two strips.  The B operands are the aligned 16-column tiles of S from the one that holds the strip's first column up to
// the last: only tiles on or above the diagonal.  |.|^2 of every tile goes (as f64) to a [16][NC] strip in LDS, and the Ns x Ns
// block sums are read from that strip -- a block that straddles a 16-column border is two tiles of the same strip row, nothing
// is padded.  Lane j of a candidate's lanes takes the pairs (a, b = a + 1 + j, a + 1 + j + lanes, ...) of the strip's a, sums a
// block in the fixed order (s, s'), and keeps its smallest (d^2, a, b) in that order; the lanes' minima meet in a butterfly.
//
// Packing.  A codebook of K Ns <= 8 columns leaves most of a tile empty: P = floor(16 / (K Ns)) candidates then share one
// wavefront trip, side by side in the columns of S.  An element of a matrix-core product depends on its own row of A and column
// of B alone (a k-ordered fma chain), and every sum above is taken in an order fixed by the shape, so no output depends on the
// packing, on the grid or on how the candidate range is split.
//
// Search.  One wavefront per workgroup walks groups of P candidates; nothing of a codebook is ever stored.  A wavefront keeps the
// best candidate of its trips (largest min d^2, then lowest index) and writes ONE record; k_codebook_pick picks among the records.
#include <cmath>

#include "cb_tile.hpp"
#include "philox.hpp"
#include "pipe_common.hpp"

namespace mcle {

constexpr int kCbMaxNt = 8;
constexpr int kCbMaxNs = 4;
constexpr int kCbMaxCols = 256;
constexpr size_t kCbLdsBudget = (size_t)160 * 1024;
enum { CB_COMPLEX = 0, CB_REAL = 1, CB_QEGT = 2, CB_INJECTED = 3 };

// (CbTile<T>, the 16 x 16 x 4 matrix-core step in either arithmetic: cb_tile.hpp)

struct CbParams {
    int K, Nt, Ns;
    int per;         // K Nt Ns: entries of a codebook
    int P;           // candidates per wavefront trip
    int lpc_shift;   // log2 of the lanes a candidate gets in the pair search
    int NC;          // P K Ns rounded up to a multiple of 16: columns of the strip
    int ld;          // NC + 16: leading dimension of S (the last strip's A operand may reach 15 columns past NC)
    int KP;          // 2 Nt rounded up to a multiple of 4
    int PB;          // precoders per strip
};

struct CbRecord {
    double d2;                   // min d^2 of the record's candidate; < 0: none
    unsigned long long index;
    int a, b;
};

inline CbParams cb_params(int K, int Nt, int Ns, bool pack) {
    CbParams p;
    p.K = K, p.Nt = Nt, p.Ns = Ns, p.per = K * Nt * Ns;
    const int ncol = K * Ns;
    p.P = (pack && ncol <= 8) ? 16 / ncol : 1;
    int lanes = 64 / p.P;
    p.lpc_shift = 0;
    while ((2 << p.lpc_shift) <= lanes) ++p.lpc_shift;
    p.NC = (p.P * ncol + 15) & ~15;
    p.ld = p.NC + 16;
    p.KP = (2 * Nt + 3) & ~3;
    p.PB = 16 / Ns;
    return p;
}
inline size_t cb_lds_S(const CbParams& p, size_t real_bytes) { return (size_t)p.KP * p.ld * real_bytes; }
inline size_t cb_lds_W(const CbParams& p) { return (size_t)16 * p.NC * sizeof(double); }

// column of S that holds column s of precoder k of the trip's candidate c
__device__ __forceinline__ int cb_col(const CbParams& p, int c, int k, int s) { return (c * p.K + k) * p.Ns + s; }

template <typename T> __device__ __forceinline__ void cb_put(const CbParams& p, T* S, int c, int i, T re, T im) {
    if (i >= p.per) return;
    const int k = i / (p.Nt * p.Ns), rem = i - k * (p.Nt * p.Ns), t = rem / p.Ns, s = rem - t * p.Ns;
    const int col = cb_col(p, c, k, s);
    S[t * p.ld + col] = re;
    S[(p.Nt + t) * p.ld + col] = im;
}

// The trip's candidates r0 .. r0 + P - 1 (those below `count`) into S, as they are before orthonormalisation.  Draws
// (mcle-philox-v1), flat entry index i = (k Nt + t) Ns + s, realization = candidate index:
//     complex: CN sample i of STREAM_CHAN;  real: sqrt(2) x the real (even i) / imaginary (odd i) part of CN sample i / 2 of
//     STREAM_CHAN;  both then divided by the precoder's Frobenius norm;  qegt: e^{j pi u_i}, u_i = uniform i of STREAM_PHASE.
// SRC = CB_INJECTED: read from `in` [count][K][Nt][Ns] instead.  A lane takes a whole Philox block.
template <typename T, int SRC>
__device__ __forceinline__ void cb_fill(const CbParams& p, T* S, const cx<T>* __restrict__ in, uint64_t seed, uint64_t first,
                                        uint64_t r0, uint64_t count, int lane) {
    if constexpr (SRC == CB_INJECTED) {
        for (int w = lane; w < p.P * p.per; w += 64) {
            const int c = w / p.per, i = w - c * p.per;
            if (r0 + c >= count) break;
            const cx<T> v = in[(r0 + c) * (uint64_t)p.per + i];
            cb_put<T>(p, S, c, i, v.x, v.y);
        }
        wave_lds_sync();
        return;
    } else {
        const int per_blk = SRC == CB_COMPLEX ? 2 : 4;
        const int nblk = (p.per + per_blk - 1) / per_blk;
        for (int w = lane; w < p.P * nblk; w += 64) {
            const int c = w / nblk, blk = w - c * nblk;
            if (r0 + c >= count) break;
            const Rng rng(seed, first + r0 + c);
            if constexpr (SRC == CB_QEGT) {
                const Words4 b = rng.block(STREAM_PHASE, (uint32_t)blk);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    double sn, cs;
                    sincospi((double)b.w[e] * 0x1p-32, &sn, &cs);
                    cb_put<T>(p, S, c, 4 * blk + e, (T)cs, (T)sn);
                }
            } else {
                // the sample is drawn in f64 whatever T and rounded once: a complex64 Box-Muller starts from a float uniform,
                // whose rounding (6e-8) alone moves sqrt(-ln u) by more than 1e-6 once u is within 1e-3 of 1
                double2 z0, z1;
                cn_pair<double>(rng, STREAM_CHAN, (uint32_t)blk, 1.0, z0, z1);
                if constexpr (SRC == CB_COMPLEX) {
                    cb_put<T>(p, S, c, 2 * blk, (T)z0.x, (T)z0.y);
                    cb_put<T>(p, S, c, 2 * blk + 1, (T)z1.x, (T)z1.y);
                } else {
                    const double r2 = 1.4142135623730951;
                    cb_put<T>(p, S, c, 4 * blk, (T)(r2 * z0.x), (T)0);
                    cb_put<T>(p, S, c, 4 * blk + 1, (T)(r2 * z0.y), (T)0);
                    cb_put<T>(p, S, c, 4 * blk + 2, (T)(r2 * z1.x), (T)0);
                    cb_put<T>(p, S, c, 4 * blk + 3, (T)(r2 * z1.y), (T)0);
                }
            }
        }
        wave_lds_sync();
        if constexpr (SRC != CB_QEGT) {
            // unit Frobenius norm per precoder: a lane per precoder, the sum in the order (t, s)
            for (int pk = lane; pk < p.P * p.K; pk += 64) {
                if (r0 + pk / p.K >= count) break;
                T n2 = 0;
                for (int t = 0; t < p.Nt; ++t)
                    for (int s = 0; s < p.Ns; ++s) {
                        const T re = S[t * p.ld + pk * p.Ns + s], im = S[(p.Nt + t) * p.ld + pk * p.Ns + s];
                        n2 = fma(re, re, n2);
                        n2 = fma(im, im, n2);
                    }
                const T inv = (T)1 / sqrt(n2);
                for (int t = 0; t < 2 * p.Nt; ++t)
                    for (int s = 0; s < p.Ns; ++s) S[t * p.ld + pk * p.Ns + s] *= inv;
            }
            wave_lds_sync();
        }
    }
}

// Modified Gram-Schmidt with one re-orthogonalisation pass, in place on the columns of S: a lane per precoder
template <typename T>
__device__ __forceinline__ void cb_orthonormalise(const CbParams& p, T* S, uint64_t r0, uint64_t count, int lane) {
    const int Nt = p.Nt, ld = p.ld;
    for (int pk = lane; pk < p.P * p.K; pk += 64) {
        if (r0 + pk / p.K >= count) break;
        for (int s = 0; s < p.Ns; ++s) {
            T* v = S + pk * p.Ns + s;
            for (int pass = 0; pass < 2; ++pass)
                for (int j = 0; j < s; ++j) {
                    const T* q = S + pk * p.Ns + j;
                    T rr = 0, ri = 0;                       // r = q^H v
                    for (int t = 0; t < Nt; ++t) {
                        const T qr = q[t * ld], qi = q[(Nt + t) * ld], vr = v[t * ld], vi = v[(Nt + t) * ld];
                        rr = fma(qr, vr, rr);
                        rr = fma(qi, vi, rr);
                        ri = fma(qr, vi, ri);
                        ri = fma(-qi, vr, ri);
                    }
                    for (int t = 0; t < Nt; ++t) {          // v -= r q
                        const T qr = q[t * ld], qi = q[(Nt + t) * ld];
                        T vr = v[t * ld], vi = v[(Nt + t) * ld];
                        vr = fma(-rr, qr, vr);
                        vr = fma(ri, qi, vr);
                        vi = fma(-rr, qi, vi);
                        vi = fma(-ri, qr, vi);
                        v[t * ld] = vr;
                        v[(Nt + t) * ld] = vi;
                    }
                }
            T n2 = 0;
            for (int t = 0; t < 2 * Nt; ++t) n2 = fma(v[t * ld], v[t * ld], n2);
            const T inv = (T)1 / sqrt(n2);
            for (int t = 0; t < 2 * Nt; ++t) v[t * ld] *= inv;
        }
    }
    wave_lds_sync();
}

// (d2, a, b) of `o` before that of `m` in the order smallest d^2, then itertools.combinations order of the pair
__device__ __forceinline__ bool cb_pair_before(double od2, int oa, int ob, double md2, int ma, int mb) {
    return od2 < md2 || (od2 == md2 && (oa < ma || (oa == ma && ob < mb)));
}
// candidate `o` better than `m`: largest min d^2, then lowest index
__device__ __forceinline__ bool cb_cand_better(double od2, unsigned long long oi, double md2, unsigned long long mi) {
    return od2 > md2 || (od2 == md2 && oi < mi);
}

// min_d2 [count], pair [count][2], d2_full [count][K][K] and recs [grid] are each optional
template <typename T, int SRC>
__global__ __launch_bounds__(64) void k_codebook(CbParams p, const cx<T>* __restrict__ in, uint64_t seed, uint64_t first,
                                                 uint64_t count, double* __restrict__ min_d2, int32_t* __restrict__ pair,
                                                 double* __restrict__ d2_full, CbRecord* __restrict__ recs) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* W = reinterpret_cast<double*>(smem);
    T* S = reinterpret_cast<T*>(W + 16 * p.NC);
    const int lane = threadIdx.x, c16 = lane & 15, kq = lane >> 4;
    const int K = p.K, Nt = p.Nt, Ns = p.Ns, ld = p.ld, NC = p.NC;
    const int lpc = 1 << p.lpc_shift, c = lane >> p.lpc_shift, j = lane & (lpc - 1);
    const int n_prec = p.P * K;
    for (int i = lane; i < p.KP * ld; i += 64) S[i] = 0;          // (the rows 2 Nt .. KP - 1 stay zero)
    wave_lds_sync();
    double best_d2 = -1.0;
    unsigned long long best_idx = 0;
    int best_a = 0, best_b = 0;
    const uint64_t groups = (count + p.P - 1) / p.P;
    for (uint64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const uint64_t r0 = grp * p.P;
        cb_fill<T, SRC>(p, S, in, seed, first, r0, count, lane);
        cb_orthonormalise<T>(p, S, r0, count, lane);
        const bool cand_ok = c < p.P && r0 + c < count;
        double md2 = INFINITY;
        int ma = 0, mb = 0;
        for (int g0 = 0; g0 < n_prec; g0 += p.PB) {
            const int ca = g0 * Ns;
            T a_re[4], a_im[4];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int k = 4 * jj + kq;
                a_re[jj] = 0, a_im[jj] = 0;
                if (k < 2 * Nt) {
                    a_re[jj] = S[k * ld + ca + c16];
                    a_im[jj] = k < Nt ? -S[(k + Nt) * ld + ca + c16] : S[(k - Nt) * ld + ca + c16];
                }
            }
            for (int n = ca >> 4; n < (NC >> 4); ++n) {
                typename CbTile<T>::acc re = {0, 0, 0, 0}, im = {0, 0, 0, 0};
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)
                    if (4 * jj < p.KP) {
                        const T b = S[(4 * jj + kq) * ld + 16 * n + c16];
                        re = CbTile<T>::mma(a_re[jj], b, re);
                        im = CbTile<T>::mma(a_im[jj], b, im);
                    }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double x = (double)re[i], y = (double)im[i];
                    W[CbTile<T>::row(lane, i) * NC + 16 * n + c16] = fma(x, x, y * y);
                }
            }
            wave_lds_sync();
            if (cand_ok) {
                const int a_lo = max(g0, c * K), a_hi = min(g0 + p.PB, (c + 1) * K);
                double* full = d2_full ? d2_full + (r0 + c) * (uint64_t)K * K : nullptr;
                for (int ag = a_lo; ag < a_hi; ++ag) {
                    const int a = ag - c * K;
                    const double* wrow = W + (ag - g0) * Ns * NC;
                    if (full && j == 0) full[a * K + a] = 0.0;
                    for (int b = a + 1 + j; b < K; b += lpc) {
                        const double* w = wrow + (c * K + b) * Ns;
                        double sum = 0.0;
                        for (int s = 0; s < Ns; ++s)
                            for (int s2 = 0; s2 < Ns; ++s2) sum += w[s * NC + s2];
                        const double d2 = fmax((double)Ns - sum, 0.0);
                        if (full) full[a * K + b] = d2, full[b * K + a] = d2;
                        if (d2 < md2) md2 = d2, ma = a, mb = b;
                    }
                }
            }
            wave_lds_sync();
        }
        for (int off = 1; off < lpc; off <<= 1) {
            const double od2 = __shfl_xor(md2, off, 64);
            const int oa = __shfl_xor(ma, off, 64), ob = __shfl_xor(mb, off, 64);
            if (cb_pair_before(od2, oa, ob, md2, ma, mb)) md2 = od2, ma = oa, mb = ob;
        }
        if (cand_ok && j == 0) {
            const uint64_t r = r0 + c;
            if (min_d2) min_d2[r] = md2;
            if (pair) pair[2 * r] = ma, pair[2 * r + 1] = mb;
            if (cb_cand_better(md2, first + r, best_d2, best_idx)) best_d2 = md2, best_idx = first + r, best_a = ma, best_b = mb;
        }
    }
    if (recs) {
        for (int off = 1; off < 64; off <<= 1) {
            const double od2 = __shfl_xor(best_d2, off, 64);
            const unsigned long long oi = __shfl_xor(best_idx, off, 64);
            const int oa = __shfl_xor(best_a, off, 64), ob = __shfl_xor(best_b, off, 64);
            if (cb_cand_better(od2, oi, best_d2, best_idx)) best_d2 = od2, best_idx = oi, best_a = oa, best_b = ob;
        }
        if (lane == 0) {
            CbRecord r;
            r.d2 = best_d2, r.index = best_idx, r.a = best_a, r.b = best_b;
            recs[blockIdx.x] = r;
        }
    }
}

// the last small step of the search: one wavefront picks among the n records, the result in out[0]
__global__ __launch_bounds__(64) void k_codebook_pick(const CbRecord* __restrict__ recs, unsigned n, CbRecord* __restrict__ out) {
    const int lane = threadIdx.x;
    double best_d2 = -1.0;
    unsigned long long best_idx = 0;
    int best_a = 0, best_b = 0;
    for (unsigned i = lane; i < n; i += 64) {
        const CbRecord r = recs[i];
        if (cb_cand_better(r.d2, r.index, best_d2, best_idx)) best_d2 = r.d2, best_idx = r.index, best_a = r.a, best_b = r.b;
    }
    for (int off = 1; off < 64; off <<= 1) {
        const double od2 = __shfl_xor(best_d2, off, 64);
        const unsigned long long oi = __shfl_xor(best_idx, off, 64);
        const int oa = __shfl_xor(best_a, off, 64), ob = __shfl_xor(best_b, off, 64);
        if (cb_cand_better(od2, oi, best_d2, best_idx)) best_d2 = od2, best_idx = oi, best_a = oa, best_b = ob;
    }
    if (lane == 0) {
        CbRecord r;
        r.d2 = best_d2, r.index = best_idx, r.a = best_a, r.b = best_b;
        out[0] = r;
    }
}

// the ledger's codebooks as they are before orthonormalisation: out [count][K][Nt][Ns]
template <typename T, int SRC>
__global__ __launch_bounds__(64) void k_codebook_generate(CbParams p, uint64_t seed, uint64_t first, uint64_t count,
                                                          cx<T>* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* S = reinterpret_cast<T*>(smem);
    const int lane = threadIdx.x;
    const uint64_t groups = (count + p.P - 1) / p.P;
    for (uint64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const uint64_t r0 = grp * p.P;
        cb_fill<T, SRC>(p, S, nullptr, seed, first, r0, count, lane);
        for (int w = lane; w < p.P * p.per; w += 64) {
            const int c = w / p.per, i = w - c * p.per;
            if (r0 + c >= count) break;
            const int k = i / (p.Nt * p.Ns), rem = i - k * (p.Nt * p.Ns), t = rem / p.Ns, s = rem - t * p.Ns;
            const int col = cb_col(p, c, k, s);
            out[(r0 + c) * (uint64_t)p.per + i] = mk<T>(S[t * p.ld + col], S[(p.Nt + t) * p.ld + col]);
        }
        wave_lds_sync();
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
static const char* const kCbTypeName[3] = {"complex", "real", "qegt"};

// the envelope every entry point shares; checked before the context so that a rule can be told without a device
inline int cb_check_shape(int dtype, int K, int Nt, int Ns) {
    MCLE_REQUIRE(dtype == MCLE_F32 || dtype == MCLE_F64, "dtype must be MCLE_F32 or MCLE_F64");
    MCLE_REQUIRE(Nt >= 2 && Nt <= kCbMaxNt, "Nt must be in [2, %d] (got %d)", kCbMaxNt, Nt);
    MCLE_REQUIRE(Ns >= 1 && Ns <= kCbMaxNs && Ns < Nt, "Ns must be in [1, min(Nt - 1, %d)] (got %d with Nt %d)", kCbMaxNs, Ns, Nt);
    MCLE_REQUIRE(K >= 2, "K must be at least 2 (got %d)", K);
    MCLE_REQUIRE((long long)K * Ns <= kCbMaxCols, "K * Ns must be at most %d (got %lld)", kCbMaxCols, (long long)K * Ns);
    return MCLE_OK;
}

inline unsigned cb_grid(const mcle_ctx* ctx, uint64_t groups, size_t lds) {
    uint64_t per_cu = lds > 0 ? kCbLdsBudget / lds : 8;
    if (per_cu > 8) per_cu = 8;
    if (per_cu < 1) per_cu = 1;
    const uint64_t resident = (uint64_t)(ctx->n_cu > 0 ? ctx->n_cu : 256) * per_cu;
    return (unsigned)oversubscribed_grid(ctx, resident, groups, 2);
}

template <typename K> inline int cb_allow_lds(K kernel, size_t lds) {
    // (the default limit covers 64 KiB)
    if (lds > 63 * 1024) MCLE_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return MCLE_OK;
}

template <typename T, int SRC>
int launch_codebook(mcle_ctx* ctx, const CbParams& p, const void* d_in, uint64_t seed, uint64_t first, uint64_t count,
                    double* d_min_d2, int32_t* d_pair, double* d_d2, CbRecord* d_recs, unsigned grid) {
    const size_t lds = cb_lds_W(p) + cb_lds_S(p, sizeof(T));
    auto kernel = k_codebook<T, SRC>;
    int rc;
    if ((rc = cb_allow_lds(kernel, lds))) return rc;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), lds, ctx->stream, p, (const cx<T>*)d_in, seed, first, count, d_min_d2, d_pair,
                       d_d2, d_recs);
    MCLE_LAUNCH_CHECK();
    return MCLE_OK;
}

template <typename T>
int dispatch_codebook(mcle_ctx* ctx, int src, const CbParams& p, const void* d_in, uint64_t seed, uint64_t first, uint64_t count,
                      double* d_min_d2, int32_t* d_pair, double* d_d2, CbRecord* d_recs, unsigned grid) {
    switch (src) {
        case CB_COMPLEX: return launch_codebook<T, CB_COMPLEX>(ctx, p, d_in, seed, first, count, d_min_d2, d_pair, d_d2, d_recs, grid);
        case CB_REAL: return launch_codebook<T, CB_REAL>(ctx, p, d_in, seed, first, count, d_min_d2, d_pair, d_d2, d_recs, grid);
        case CB_QEGT: return launch_codebook<T, CB_QEGT>(ctx, p, d_in, seed, first, count, d_min_d2, d_pair, d_d2, d_recs, grid);
        default: return launch_codebook<T, CB_INJECTED>(ctx, p, d_in, seed, first, count, d_min_d2, d_pair, d_d2, d_recs, grid);
    }
}

template <typename T, int SRC>
int launch_generate(mcle_ctx* ctx, const CbParams& p, uint64_t seed, uint64_t first, uint64_t count, void* d_out) {
    const size_t lds = cb_lds_S(p, sizeof(T));
    auto kernel = k_codebook_generate<T, SRC>;
    const unsigned grid = cb_grid(ctx, (count + p.P - 1) / p.P, lds);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), lds, ctx->stream, p, seed, first, count, (cx<T>*)d_out);
    MCLE_LAUNCH_CHECK();
    return MCLE_OK;
}

template <typename T>
int dispatch_generate(mcle_ctx* ctx, int type, const CbParams& p, uint64_t seed, uint64_t first, uint64_t count, void* d_out) {
    switch (type) {
        case CB_COMPLEX: return launch_generate<T, CB_COMPLEX>(ctx, p, seed, first, count, d_out);
        case CB_REAL: return launch_generate<T, CB_REAL>(ctx, p, seed, first, count, d_out);
        default: return launch_generate<T, CB_QEGT>(ctx, p, seed, first, count, d_out);
    }
}

}  // namespace mcle

using namespace mcle;

extern "C" {

int mcle_chordal_min_dist(mcle_ctx* ctx, int dtype, const void* d_codebooks, size_t n_codebooks, int K, int Nt, int Ns,
                          double* d_min_d2, int32_t* d_pair, double* d_d2) {
    if (ctx) ctx->last_kernel[0] = 0;
    int rc;
    if ((rc = cb_check_shape(dtype, K, Nt, Ns))) return rc;
    MCLE_REQUIRE(n_codebooks <= 0x7fffffffull, "n_codebooks must be at most 2^31-1");
    MCLE_REQUIRE(ctx != nullptr, "null context");
    if (n_codebooks == 0) return MCLE_OK;
    MCLE_REQUIRE(d_codebooks != nullptr, "null d_codebooks");
    MCLE_REQUIRE(d_min_d2 != nullptr, "null d_min_d2");
    MCLE_REQUIRE(d_pair != nullptr, "null d_pair");
    if ((rc = ctx->bind())) return rc;
    const CbParams p = cb_params(K, Nt, Ns, ctx->opt[MCLE_OPT_CODEBOOK_NO_PACK] == 0);
    const size_t lds = cb_lds_W(p) + cb_lds_S(p, dtype == MCLE_F64 ? 8 : 4);
    const unsigned grid = cb_grid(ctx, (n_codebooks + p.P - 1) / p.P, lds);
    rc = dtype == MCLE_F32 ? dispatch_codebook<float>(ctx, CB_INJECTED, p, d_codebooks, 0, 0, n_codebooks, d_min_d2, d_pair, d_d2, nullptr, grid)
                           : dispatch_codebook<double>(ctx, CB_INJECTED, p, d_codebooks, 0, 0, n_codebooks, d_min_d2, d_pair, d_d2, nullptr, grid);
    if (rc) return rc;
    ctx->set_kernel("chordal_min_dist %s p%d", dtype == MCLE_F64 ? "f64" : "f32", p.P);
    return MCLE_OK;
}

int mcle_codebook_generate(mcle_ctx* ctx, int dtype, int type, int K, int Nt, int Ns, uint64_t seed, uint64_t first, uint64_t count,
                           void* d_out) {
    if (ctx) ctx->last_kernel[0] = 0;
    int rc;
    if ((rc = cb_check_shape(dtype, K, Nt, Ns))) return rc;
    MCLE_REQUIRE(type >= CB_COMPLEX && type <= CB_QEGT, "type must be 0 (complex), 1 (real) or 2 (qegt) (got %d)", type);
    MCLE_REQUIRE(count <= 0x7fffffffull, "count must be at most 2^31-1");
    MCLE_REQUIRE(ctx != nullptr, "null context");
    if (count == 0) return MCLE_OK;
    MCLE_REQUIRE(d_out != nullptr, "null d_out");
    if ((rc = ctx->bind())) return rc;
    const CbParams p = cb_params(K, Nt, Ns, ctx->opt[MCLE_OPT_CODEBOOK_NO_PACK] == 0);
    rc = dtype == MCLE_F32 ? dispatch_generate<float>(ctx, type, p, seed, first, count, d_out)
                           : dispatch_generate<double>(ctx, type, p, seed, first, count, d_out);
    if (rc) return rc;
    ctx->set_kernel("codebook_generate %s %s p%d", dtype == MCLE_F64 ? "f64" : "f32", kCbTypeName[type], p.P);
    return MCLE_OK;
}

int mcle_run_codebook_search(mcle_ctx* ctx, int dtype, const mcle_codebook_cfg* cfg, uint64_t seed, uint64_t first, uint64_t count,
                             mcle_codebook_result* out, double* d_min_d2, int32_t* d_pair) {
    if (ctx) ctx->last_kernel[0] = 0;
    MCLE_REQUIRE(cfg != nullptr, "null cfg");
    int rc;
    if ((rc = cb_check_shape(dtype, cfg->K, cfg->Nt, cfg->Ns))) return rc;
    MCLE_REQUIRE(cfg->type >= CB_COMPLEX && cfg->type <= CB_QEGT, "type must be 0 (complex), 1 (real) or 2 (qegt) (got %d)", cfg->type);
    MCLE_REQUIRE(count <= 0x7fffffffull, "count must be at most 2^31-1");
    MCLE_REQUIRE(out != nullptr, "null out");
    MCLE_REQUIRE(ctx != nullptr, "null context");
    out->best_index = 0, out->best_min_d2 = 0.0, out->pair[0] = out->pair[1] = 0, out->n_candidates = 0;
    if (count == 0) return MCLE_OK;
    if ((rc = ctx->bind())) return rc;
    const CbParams p = cb_params(cfg->K, cfg->Nt, cfg->Ns, ctx->opt[MCLE_OPT_CODEBOOK_NO_PACK] == 0);
    const size_t lds = cb_lds_W(p) + cb_lds_S(p, dtype == MCLE_F64 ? 8 : 4);
    const unsigned grid = cb_grid(ctx, (count + p.P - 1) / p.P, lds);
    void* d_blk = nullptr;
    if ((rc = ctx->scratch(((size_t)grid + 1) * sizeof(CbRecord), &d_blk))) return rc;
    CbRecord* d_recs = (CbRecord*)d_blk + 1;        // [0]: the result, [1 ..]: one record per wavefront
    rc = dtype == MCLE_F32 ? dispatch_codebook<float>(ctx, cfg->type, p, nullptr, seed, first, count, d_min_d2, d_pair, nullptr, d_recs, grid)
                           : dispatch_codebook<double>(ctx, cfg->type, p, nullptr, seed, first, count, d_min_d2, d_pair, nullptr, d_recs, grid);
    if (rc) return rc;
    hipLaunchKernelGGL(k_codebook_pick, dim3(1), dim3(64), 0, ctx->stream, (const CbRecord*)d_recs, grid, (CbRecord*)d_blk);
    MCLE_LAUNCH_CHECK();
    CbRecord best;
    MCLE_HIP(hipMemcpyAsync(&best, d_blk, sizeof(best), hipMemcpyDeviceToHost, ctx->stream));
    MCLE_HIP(hipStreamSynchronize(ctx->stream));
    out->best_index = best.index, out->best_min_d2 = best.d2, out->pair[0] = best.a, out->pair[1] = best.b;
    out->n_candidates = count;
    ctx->set_kernel("codebook_search %s %s p%d", dtype == MCLE_F64 ? "f64" : "f32", kCbTypeName[cfg->type], p.P);
    return MCLE_OK;
}

}  // extern "C"
