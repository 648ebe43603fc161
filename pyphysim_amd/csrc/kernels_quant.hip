// kernels_quant.hip -- limited-feedback channel quantization: every link of a K-user interference channel is replaced by the
// nearest word of a vector codebook (reference: apps/ia/simple_maxsinr_quantized.py:40-154 calc_dist, calc_angle_dist,
// quant_small_matrix, my_quant_func).
//
// A link is the nr x nt block (k1, k2) of big_H, flattened row-major to v [dim = nr nt]; a codeword is a row c [dim] of the
// codebook.  With v^ = v / ||v||
//     metric 0 (calc_dist):        d = ||v^ - c||^2 = (1 + ||c||^2) - 2 Re(c^H v^)
//     metric 1 (calc_angle_dist):  d = 1 - |c^H v^|^2 / ||c||^2
// and the link takes the codeword of the smallest d, the lowest index on a tie (numpy.argmin).  A block whose entries are all
// zero takes codeword 0 with d = NaN (the reference's distances are all NaN there and argmin returns 0).
//
// Tile map.  Re(c^H v^) for 16 codewords x 16 links is one real product on v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32:
//     A [16 codewords][KP] = [Re c, Im c],   B [KP][16 links] = [Re v^; Im v^],   KP = 2 dim rounded up to a multiple of 4,
// and Im(c^H v^) is the SAME A against B' = [Im v^; -Re v^] (metric 1 only).  Columns are the links of consecutive
// realizations flattened, link = r K^2 + k1 K + k2: a strip of 16 columns straddles realizations when K^2 does not divide 16.
// A wavefront owns a strip: its B operands stay in registers while it walks the row tiles of the codebook in index order;
// a lane keeps the running (d, index) minimum of its four rows (strict <, rows and tiles ascending), and the four lane groups
// of a column meet once per strip (smaller d, then lower index).  A workgroup is four wavefronts = four strips; the codebook's
// operand matrix Sc [KP][ld] and one double per codeword (1 + ||c||^2 or 1 / ||c||^2) are staged in LDS once per workgroup,
// or chunk by chunk per group of strips when the codebook does not fit.  ld = chunk + 16 with chunk a multiple of 32: the
// lanes l and l + 16 of an A read (rows k and k + 1 of Sc) then fall on opposite halves of the bank row.
//
// An element of a matrix-core product depends on its own row of A and column of B alone (a k-ordered fma chain), ||v||^2 and
// ||c||^2 are summed in entry order, and the minimum is taken in index order: NO OUTPUT DEPENDS ON THE GRID, ON THE POSITION OF
// A LINK IN A STRIP, ON THE CHUNKING OR ON HOW A BATCH IS SPLIT, bit for bit.  |z|^2 is taken as fma(hi, hi, lo lo) of the
// larger and the smaller of |re|, |im|, so multiplying a link by j (which swaps the two products up to a sign, exactly) leaves
// metric 1 unchanged bit for bit; scaling big_H by a power of two leaves v^ unchanged (the norm is taken in f64).
#include <cmath>

#include "cb_tile.hpp"
#include "philox.hpp"
#include "pipe_common.hpp"
#include "quant.hpp"

namespace mcle {

constexpr int kQuantMaxK = 4, kQuantMaxAnt = 6, kQuantMaxWords = 4096;
constexpr int kQuantSteps = (2 * kQuantMaxAnt * kQuantMaxAnt + 3) / 4;     // 18 steps of 4 over the inner dimension
constexpr size_t kQuantOperandBudget = (size_t)48 * 1024;
enum { QUANT_INJECTED = 0, QUANT_DRAWN = 1 };

struct QuantParams {
    int K, nr, nt, dim;
    int KP;          // 2 dim rounded up to a multiple of 4
    int C;           // codewords
    int CH;          // codewords per LDS chunk, a multiple of 32
    int ld;          // CH + 16: leading dimension of Sc
    int n_chunks;
    uint64_t n_links;
};

inline QuantParams quant_params(int K, int nr, int nt, int C, uint64_t batch, size_t real_bytes) {
    QuantParams p;
    p.K = K, p.nr = nr, p.nt = nt, p.dim = nr * nt, p.C = C;
    p.KP = (2 * p.dim + 3) & ~3;
    int ch = (int)(kQuantOperandBudget / ((size_t)p.KP * real_bytes));
    ch = ((ch - 16) / 32) * 32;
    if (ch < 32) ch = 32;
    const int cr = (C + 31) & ~31;
    p.CH = ch < cr ? ch : cr;
    p.ld = p.CH + 16;
    p.n_chunks = (C + p.CH - 1) / p.CH;
    p.n_links = batch * (uint64_t)(K * K);
    return p;
}
inline size_t quant_lds(const QuantParams& p, size_t real_bytes) {
    return (size_t)p.CH * sizeof(double) + (size_t)p.KP * p.ld * real_bytes;
}

// |z|^2, the same value for (x, y), (y, x) and any signs
__device__ __forceinline__ double quant_abs2(double x, double y) {
    const double ax = fabs(x), ay = fabs(y);
    const double hi = fmax(ax, ay), lo = fmin(ax, ay);
    return fma(hi, hi, lo * lo);
}

// A chunk of the codebook into LDS: Sc[k][w] = Re c_w[k] (k < dim), Im c_w[k - dim] (k < 2 dim), 0 beyond and for w past the
// codebook; cw[w] = 1 + ||c_w||^2 (metric 0) or 1 / ||c_w||^2 (metric 1), the norm in f64 in entry order
template <typename T, int METRIC>
__device__ __forceinline__ void quant_stage(const QuantParams& p, const cx<T>* __restrict__ codebook, int w0, T* Sc, double* cw,
                                            int tid) {
    for (int i = tid; i < p.KP * p.ld; i += 256) Sc[i] = 0;
    __syncthreads();
    const int n = min(p.CH, p.C - w0);
    for (int i = tid; i < n * p.dim; i += 256) {
        const int w = i / p.dim, e = i - w * p.dim;
        const cx<T> c = codebook[(size_t)(w0 + w) * p.dim + e];
        Sc[e * p.ld + w] = c.x;
        Sc[(p.dim + e) * p.ld + w] = c.y;
    }
    for (int w = tid; w < p.CH; w += 256) {
        double n2 = 0.0;
        if (w < n)
            for (int e = 0; e < p.dim; ++e) {
                const cx<T> c = codebook[(size_t)(w0 + w) * p.dim + e];
                n2 += quant_abs2((double)c.x, (double)c.y);
            }
        cw[w] = METRIC == 0 ? 1.0 + n2 : 1.0 / n2;
    }
    __syncthreads();
}

// The B operands of this lane's column: b[jj] = B[4 jj + kq][column], b2 the same of B' = [Im v^; -Re v^].
// SRC = QUANT_INJECTED: the block (k1, k2) of bigH [batch][K nr][K nt];  QUANT_DRAWN (K = 3, 2 x 2): big_H of realization
// first + r as mcle_run_ia draws it, CN sample (2 k1 + i) 6 + 2 k2 + j of STREAM_CHAN in f64, rounded once to T.
template <typename T, int SRC>
__device__ __forceinline__ void quant_column(const QuantParams& p, const cx<T>* __restrict__ bigH, uint64_t seed, uint64_t first,
                                             uint64_t link, bool live, int kq, T (&b)[kQuantSteps], T (&b2)[kQuantSteps],
                                             bool& zero) {
#pragma unroll
    for (int jj = 0; jj < kQuantSteps; ++jj) b[jj] = 0, b2[jj] = 0;
    zero = false;
    if (!live) return;
    const int KK = p.K * p.K;
    const uint64_t r = link / (uint64_t)KK;
    const int l = (int)(link - r * (uint64_t)KK), k1 = l / p.K, k2 = l - k1 * p.K;
    if constexpr (SRC == QUANT_DRAWN) {
        const Rng rng(seed, first + r);
        double2 d0, d1, d2, d3;
        cn_pair<double>(rng, STREAM_CHAN, (uint32_t)(6 * k1 + k2), 1.0, d0, d1);
        cn_pair<double>(rng, STREAM_CHAN, (uint32_t)(6 * k1 + 3 + k2), 1.0, d2, d3);
        const cx<T> z0 = mk<T>((T)d0.x, (T)d0.y), z1 = mk<T>((T)d1.x, (T)d1.y), z2 = mk<T>((T)d2.x, (T)d2.y),
                    z3 = mk<T>((T)d3.x, (T)d3.y);
        double n2 = quant_abs2((double)z0.x, (double)z0.y);
        n2 += quant_abs2((double)z1.x, (double)z1.y);
        n2 += quant_abs2((double)z2.x, (double)z2.y);
        n2 += quant_abs2((double)z3.x, (double)z3.y);
        zero = !(n2 > 0.0);
        const double inv = 1.0 / sqrt(n2);
        const cx<T> z = kq == 0 ? z0 : kq == 1 ? z1 : kq == 2 ? z2 : z3;      // (selects: no lane-dependent register index)
        const T x = (T)((double)z.x * inv), y = (T)((double)z.y * inv);
        b[0] = x, b2[0] = y;          // inner index kq: Re of entry kq
        b[1] = y, b2[1] = -x;         // inner index 4 + kq: Im of entry kq
    } else {
        const int rowlen = p.K * p.nt;
        const cx<T>* base = bigH + (size_t)r * ((size_t)p.K * p.nr * rowlen) + (size_t)(k1 * p.nr) * rowlen + k2 * p.nt;
        double n2 = 0.0;
        for (int e = 0; e < p.dim; ++e) {
            const int i = e / p.nt, j = e - i * p.nt;
            const cx<T> v = base[i * rowlen + j];
            n2 += quant_abs2((double)v.x, (double)v.y);
        }
        zero = !(n2 > 0.0);
        const double inv = 1.0 / sqrt(n2);
#pragma unroll
        for (int jj = 0; jj < kQuantSteps; ++jj) {
            const int k = 4 * jj + kq;
            if (k < 2 * p.dim) {
                const bool re = k < p.dim;
                const int e = re ? k : k - p.dim, i = e / p.nt, j = e - i * p.nt;
                const cx<T> v = base[i * rowlen + j];
                const T x = (T)((double)v.x * inv), y = (T)((double)v.y * inv);
                b[jj] = re ? x : y;
                b2[jj] = re ? y : -x;
            }
        }
    }
}

// The search: index [n_links] (int32), bigHq (may be NULL, QUANT_INJECTED only) and dist (may be NULL) [n_links]
template <typename T, int METRIC, int SRC>
__device__ __forceinline__ void quant_search(const QuantParams& p, const cx<T>* __restrict__ bigH,
                                             const cx<T>* __restrict__ codebook, uint64_t seed, uint64_t first,
                                             int32_t* __restrict__ index, cx<T>* __restrict__ bigHq, double* __restrict__ dist,
                                             char* smem) {
    double* cw = reinterpret_cast<double*>(smem);
    T* Sc = reinterpret_cast<T*>(cw + p.CH);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c16 = lane & 15, kq = lane >> 4;
    const uint64_t n_strips = (p.n_links + 15) / 16, n_groups = (n_strips + 3) / 4;
    bool staged = false;
    for (uint64_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        const uint64_t link = (grp * 4 + wave) * 16 + c16;
        const bool live = link < p.n_links;
        T b[kQuantSteps], b2[kQuantSteps];
        bool zero;
        quant_column<T, SRC>(p, bigH, seed, first, link, live, kq, b, b2, zero);
        double best = INFINITY;
        int best_i = 0;
        for (int ch = 0; ch < p.n_chunks; ++ch) {
            const int w0 = ch * p.CH;
            if (!staged || p.n_chunks > 1) {
                if (staged) __syncthreads();          // every wavefront is done with the chunk that is replaced
                quant_stage<T, METRIC>(p, codebook, w0, Sc, cw, tid);
                staged = true;
            }
            const int n_tiles = (min(p.CH, p.C - w0) + 15) >> 4;
            for (int t = 0; t < n_tiles; ++t) {
                typename CbTile<T>::acc re = {0, 0, 0, 0}, im = {0, 0, 0, 0};
#pragma unroll
                for (int jj = 0; jj < kQuantSteps; ++jj)
                    if (4 * jj < p.KP) {
                        const T a = Sc[(4 * jj + kq) * p.ld + 16 * t + c16];
                        re = CbTile<T>::mma(a, b[jj], re);
                        if constexpr (METRIC == 1) im = CbTile<T>::mma(a, b2[jj], im);
                    }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int wl = 16 * t + CbTile<T>::row(lane, i);
                    const double s = cw[wl];
                    double d;
                    if constexpr (METRIC == 0)
                        d = fma(-2.0, (double)re[i], s);
                    else
                        d = fma(-quant_abs2((double)re[i], (double)im[i]), s, 1.0);
                    if (w0 + wl < p.C && d < best) best = d, best_i = w0 + wl;
                }
            }
        }
        for (int off = 16; off < 64; off <<= 1) {
            const double od = __shfl_xor(best, off, 64);
            const int oi = __shfl_xor(best_i, off, 64);
            if (od < best || (od == best && oi < best_i)) best = od, best_i = oi;
        }
        if (zero) best = NAN, best_i = 0;
        if (live) {
            if (kq == 0) {
                index[link] = best_i;
                if (dist) dist[link] = best;
            }
            if constexpr (SRC == QUANT_INJECTED) {
                if (bigHq) {
                    const int KK = p.K * p.K, rowlen = p.K * p.nt;
                    const uint64_t r = link / (uint64_t)KK;
                    const int l = (int)(link - r * (uint64_t)KK), k1 = l / p.K, k2 = l - k1 * p.K;
                    cx<T>* base = bigHq + (size_t)r * ((size_t)p.K * p.nr * rowlen) + (size_t)(k1 * p.nr) * rowlen + k2 * p.nt;
                    for (int e = kq; e < p.dim; e += 4) {
                        const int i = e / p.nt, j = e - i * p.nt;
                        base[i * rowlen + j] = codebook[(size_t)best_i * p.dim + e];
                    }
                }
            }
        }
    }
}

template <typename T, int METRIC, int SRC>
__global__ __launch_bounds__(256) void k_quantize(QuantParams p, const cx<T>* __restrict__ bigH, const cx<T>* __restrict__ codebook,
                                                  uint64_t seed, uint64_t first, int32_t* __restrict__ index,
                                                  cx<T>* __restrict__ bigHq, double* __restrict__ dist) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    quant_search<T, METRIC, SRC>(p, bigH, codebook, seed, first, index, bigHq, dist, smem);
}

// ---- host side -------------------------------------------------------------------------------------------------------------
int quant_check_cfg(int dtype, const mcle_quant_cfg* cfg) {
    MCLE_REQUIRE(dtype == MCLE_F32 || dtype == MCLE_F64, "dtype must be MCLE_F32 or MCLE_F64");
    MCLE_REQUIRE(cfg != nullptr, "null quantizer cfg");
    MCLE_REQUIRE(cfg->K >= 1 && cfg->K <= kQuantMaxK, "K must be in [1, %d] (got %d)", kQuantMaxK, cfg->K);
    MCLE_REQUIRE(cfg->nr >= 1 && cfg->nr <= kQuantMaxAnt, "nr must be in [1, %d] (got %d)", kQuantMaxAnt, cfg->nr);
    MCLE_REQUIRE(cfg->nt >= 1 && cfg->nt <= kQuantMaxAnt, "nt must be in [1, %d] (got %d)", kQuantMaxAnt, cfg->nt);
    MCLE_REQUIRE(cfg->n_codewords >= 1 && cfg->n_codewords <= kQuantMaxWords, "n_codewords must be in [1, %d] (got %d)",
                 kQuantMaxWords, cfg->n_codewords);
    MCLE_REQUIRE(cfg->metric == MCLE_QUANT_EUCLIDEAN || cfg->metric == MCLE_QUANT_CHORDAL,
                 "metric must be 0 (calc_dist) or 1 (calc_angle_dist) (got %d)", cfg->metric);
    return MCLE_OK;
}

template <typename T, int SRC>
static int launch_quant_t(mcle_ctx* ctx, const mcle_quant_cfg* cfg, const void* d_bigH, const void* d_codebook, uint64_t seed,
                          uint64_t first, int32_t* d_index, void* d_bigHq, double* d_dist, uint64_t batch) {
    const QuantParams p = quant_params(cfg->K, cfg->nr, cfg->nt, cfg->n_codewords, batch, sizeof(T));
    const size_t lds = quant_lds(p, sizeof(T));
    const uint64_t groups = ((p.n_links + 15) / 16 + 3) / 4;
    uint64_t per_cu = (size_t)160 * 1024 / lds;
    if (per_cu > 4) per_cu = 4;
    const unsigned grid = (unsigned)oversubscribed_grid(ctx, (uint64_t)(ctx->n_cu > 0 ? ctx->n_cu : 256) * per_cu, groups, 2);
    if (cfg->metric == MCLE_QUANT_EUCLIDEAN)
        hipLaunchKernelGGL((k_quantize<T, 0, SRC>), dim3(grid), dim3(256), lds, ctx->stream, p, (const cx<T>*)d_bigH,
                           (const cx<T>*)d_codebook, seed, first, d_index, (cx<T>*)d_bigHq, d_dist);
    else
        hipLaunchKernelGGL((k_quantize<T, 1, SRC>), dim3(grid), dim3(256), lds, ctx->stream, p, (const cx<T>*)d_bigH,
                           (const cx<T>*)d_codebook, seed, first, d_index, (cx<T>*)d_bigHq, d_dist);
    MCLE_LAUNCH_CHECK();
    return MCLE_OK;
}

int launch_quantize_drawn(mcle_ctx* ctx, int dtype, const mcle_quant_cfg* cfg, const void* d_codebook, uint64_t seed,
                          uint64_t first, uint64_t count, int32_t* d_index, double* d_dist) {
    return dtype == MCLE_F32
               ? launch_quant_t<float, QUANT_DRAWN>(ctx, cfg, nullptr, d_codebook, seed, first, d_index, nullptr, d_dist, count)
               : launch_quant_t<double, QUANT_DRAWN>(ctx, cfg, nullptr, d_codebook, seed, first, d_index, nullptr, d_dist, count);
}

}  // namespace mcle

using namespace mcle;

extern "C" {

int mcle_quantize_links(mcle_ctx* ctx, int dtype, const mcle_quant_cfg* cfg, const void* d_bigH, const void* d_codebook,
                        int32_t* d_index, void* d_bigHq, double* d_dist, size_t batch) {
    if (ctx) ctx->last_kernel[0] = 0;
    int rc;
    if ((rc = quant_check_cfg(dtype, cfg))) return rc;
    MCLE_REQUIRE((uint64_t)batch * (uint64_t)(cfg->K * cfg->K) <= 0x7fffffffull, "batch * K^2 must be at most 2^31-1");
    MCLE_REQUIRE(ctx != nullptr, "null context");
    if (batch == 0) return MCLE_OK;
    MCLE_REQUIRE(d_bigH != nullptr, "null d_bigH");
    MCLE_REQUIRE(d_codebook != nullptr, "null d_codebook");
    MCLE_REQUIRE(d_index != nullptr, "null d_index");
    if ((rc = ctx->bind())) return rc;
    rc = dtype == MCLE_F32
             ? launch_quant_t<float, QUANT_INJECTED>(ctx, cfg, d_bigH, d_codebook, 0, 0, d_index, d_bigHq, d_dist, batch)
             : launch_quant_t<double, QUANT_INJECTED>(ctx, cfg, d_bigH, d_codebook, 0, 0, d_index, d_bigHq, d_dist, batch);
    if (rc) return rc;
    ctx->set_kernel("quantize_links %s m%d", dtype == MCLE_F64 ? "f64" : "f32", cfg->metric);
    return MCLE_OK;
}

}  // extern "C"
