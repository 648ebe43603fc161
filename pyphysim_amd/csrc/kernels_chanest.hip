// kernels_chanest.hip -- pilot-based channel estimation from CAZAC reference signals (reference:
// reference_signals/channel_estimation.py:73-131 CazacBasedChannelEstimator, :135-251 the cover-code variant) and the fused
// estimation-error pipeline built on it.
//
// The reference computes FFT_{m Ne}( IFFT_{Ne}(conj(r) y)[0 : K + 1] ) (times Ne for a normalised sequence).  Only K + 1 delay
// taps survive the truncation, so both transforms are PRUNED direct DFTs over the one table w[j] = exp(-2 pi i j / (m Ne)):
//     h[t] = (1 / Ne) sum_n conj(r[n]) y[n] conj(w[(m n t) mod m Ne])      t = 0 .. K      (pass 1)
//     H[k] =          sum_t h[t]            w[(k t) mod m Ne]              k = 0 .. m Ne-1 (pass 2)
// Ne (K + 1)(1 + m) complex FMAs per row, any Ne.  One wavefront per row (a row = one realization and receive antenna), several
// rows per workgroup, grid-stride over rows; z = conj(r) y and the K + 1 taps live in the wavefront's own LDS, the table once
// per workgroup.  Twiddle indexes are stepped with a conditional subtract; the one product a lane needs at the start of its
// run is reduced with mod_small (no integer division anywhere).
#include "cazac_common.hpp"

namespace mcle {

struct CoverCode {
    double c[kCazacMaxCover];
};

// ref [ne]; rx [rows][n_cover][ne]; out [rows][N].  LDS: the table [N] when TWL, then per wavefront z [ne] and h [K + 1].
template <typename T, bool TWL>
__global__ __launch_bounds__(256) void k_cazac_estimate(const cx<T>* __restrict__ ref, const cx<T>* __restrict__ rx,
                                                        size_t rows, int n_cover, CoverCode cover, CazacShape s, T scale,
                                                        const cx<T>* __restrict__ tw, cx<T>* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cx<T>* base = reinterpret_cast<cx<T>*>(smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const cx<T>* w = tw;
    if constexpr (TWL) {
        for (int j = threadIdx.x; j < s.N; j += blockDim.x) base[j] = tw[j];
        w = base;
        base += s.N;
        __syncthreads();
    }
    cx<T>* z = base + (size_t)wave * (s.ne + s.n_tap);
    cx<T>* h = z + s.ne;
    const T inv_cover = (T)1 / (T)n_cover;
    for (size_t row = (size_t)blockIdx.x * waves + wave; row < rows; row += (size_t)gridDim.x * waves) {
        const cx<T>* y = rx + row * (size_t)n_cover * s.ne;
        for (int n = lane; n < s.ne; n += 64) {
            cx<T> v = y[n];
            if (n_cover > 1 || cover.c[0] != 1.0) {          // mean over the cover-code axis of cover[c] * y[c][n]
                v = cscale(v, (T)cover.c[0]);
#pragma unroll
                for (int c = 1; c < kCazacMaxCover; ++c)
                    if (c < n_cover) {
                        const cx<T> u = y[(size_t)c * s.ne + n];
                        v.x = fma((T)cover.c[c], u.x, v.x);
                        v.y = fma((T)cover.c[c], u.y, v.y);
                    }
                v = cscale(v, inv_cover);
            }
            z[n] = cmulc(v, ref[n]);
        }
        wave_lds_sync();
        cazac_taps<T>(z, h, s, w, scale, lane);
        wave_lds_sync();
        cx<T>* dst = out + row * (size_t)s.N;
        for (int k = lane; k < s.N; k += 64) dst[k] = cazac_bin<T>(h, s.n_tap, k, s.N, w);
        wave_lds_sync();
    }
}

template <typename T>
int launch_cazac(mcle_ctx* ctx, const void* d_ref, const void* d_rx, size_t rows, int n_cover, const CoverCode& cover,
                 const CazacShape& s, int normalized, const void* tw, void* d_out) {
    int waves, twl;
    size_t lds;
    cazac_lds_plan((size_t)s.N * sizeof(cx<T>), (size_t)(s.ne + s.n_tap) * sizeof(cx<T>), 0, &waves, &twl, &lds);
    MCLE_REQUIRE(waves > 0, "cazac estimate: %d + %d samples do not fit the device's LDS", s.ne, s.n_tap);
    const size_t groups = (rows + waves - 1) / waves;
    const size_t cap = (size_t)(ctx->n_cu > 0 ? ctx->n_cu : 256) * 8;
    const unsigned grid = (unsigned)(groups < cap ? groups : cap);
    const T scale = normalized ? (T)1 : (T)(1.0 / s.ne);
    auto go = [&](auto kernel) -> int {
        // (the default limit covers 64 KiB, static arrays included: the common sizes launch without this host round trip)
        if (lds > 63 * 1024) MCLE_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * waves), lds, ctx->stream, (const cx<T>*)d_ref, (const cx<T>*)d_rx,
                           rows, n_cover, cover, s, scale, (const cx<T>*)tw, (cx<T>*)d_out);
        MCLE_LAUNCH_CHECK();
        return MCLE_OK;
    };
    const int rc = twl ? go(k_cazac_estimate<T, true>) : go(k_cazac_estimate<T, false>);
    if (rc == MCLE_OK) ctx->set_kernel("cazac_estimate %s w%d%s", sizeof(T) == 8 ? "f64" : "f32", waves, twl ? "" : " gtw");
    return rc;
}

// ---- fused estimation-error pipeline ---------------------------------------------------------------------------------------
// One wavefront per realization.  Draws (mcle-philox-v1): tap i of link (user u, antenna a) = CN sample
// (u n_rx + a) n_taps + i of STREAM_CHAN scaled by sqrt(p_i); noise of (antenna a, comb position n) = CN sample
// 2 ceil(Ne / 2) a + n of STREAM_NOISE (a Philox block = positions 2 j and 2 j + 1 of one antenna) scaled by sqrt(noise_var).
struct ChanestParams {
    CazacShape s;
    int n_users, n_rx, n_taps, half;      // half = ceil(ne / 2)
    int normalized;
    double sigma;
    double amp[MCLE_MAX_TAPS];
    int delay[MCLE_MAX_TAPS];
};

// seq [n_users][ne]; err / pow [count][n_users].  LDS: delays and amplitudes, the table [N] when TWL, then per wavefront
// taps [n_users n_rx n_taps], y [ne], z [ne], h [K + 1].
template <typename T, bool TWL>
__global__ __launch_bounds__(256) void k_chanest(ChanestParams p, const cx<T>* __restrict__ seq, uint64_t seed, uint64_t first,
                                                 uint64_t count, const cx<T>* __restrict__ tw, double* __restrict__ err,
                                                 double* __restrict__ pow) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_delay[MCLE_MAX_TAPS];
    __shared__ T s_amp[MCLE_MAX_TAPS];
    cx<T>* base = reinterpret_cast<cx<T>*>(smem);
    const CazacShape& s = p.s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
#pragma unroll
    for (int i = 0; i < MCLE_MAX_TAPS; ++i)
        if ((int)threadIdx.x == i) {
            s_delay[i] = p.delay[i];
            s_amp[i] = (T)p.amp[i];
        }
    const cx<T>* w = tw;
    if constexpr (TWL) {
        for (int j = threadIdx.x; j < s.N; j += blockDim.x) base[j] = tw[j];
        w = base;
        base += s.N;
    }
    __syncthreads();
    const int n_links = p.n_users * p.n_rx, n_draw = n_links * p.n_taps;
    cx<T>* taps = base + (size_t)wave * (n_draw + 2 * s.ne + s.n_tap);
    cx<T>* y = taps + n_draw;
    cx<T>* z = y + s.ne;
    cx<T>* h = z + s.ne;
    const T scale = p.normalized ? (T)1 : (T)(1.0 / s.ne);
    for (uint64_t r = (uint64_t)blockIdx.x * waves + wave; r < count; r += (uint64_t)gridDim.x * waves) {
        const Rng rng(seed, first + r);
        for (int d = lane; d < n_draw; d += 64) {
            taps[d] = cn_sample<T>(rng, STREAM_CHAN, (uint64_t)d, s_amp[d % p.n_taps]);     // (<= 12 draws per lane)
        }
        wave_lds_sync();
        for (int a = 0; a < p.n_rx; ++a) {
            // the received comb of antenna a: Y[n] = sum_u r_u[n] sum_i h_uai w[(m n d_i) mod N] + noise; a lane takes the
            // positions 2 j and 2 j + 1 one Philox block serves
            for (int j = lane; j < p.half; j += 64) {
                cx<T> v[2];
                v[0] = v[1] = mk<T>(0, 0);
                if (p.sigma != 0.0) cn_pair<T>(rng, STREAM_NOISE, (uint32_t)(a * p.half + j), (T)p.sigma, v[0], v[1]);
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int n = 2 * j + e;
                    if (n >= s.ne) break;
                    const int mn = s.m * n;                                   // < N
                    for (int u = 0; u < p.n_users; ++u) {
                        const cx<T>* g = taps + (u * p.n_rx + a) * p.n_taps;
                        cx<T> H = mk<T>(0, 0);
                        for (int i = 0; i < p.n_taps; ++i)
                            H = cfma4(g[i], w[mod_small(mn * s_delay[i], s.N, s.inv_N)], H);   // mn d_i < N ne
                        v[e] = cfma4(H, seq[(size_t)u * s.ne + n], v[e]);
                    }
                    y[n] = v[e];
                }
            }
            wave_lds_sync();
            for (int u = 0; u < p.n_users; ++u) {
                for (int n = lane; n < s.ne; n += 64) z[n] = cmulc(y[n], seq[(size_t)u * s.ne + n]);
                wave_lds_sync();
                cazac_taps<T>(z, h, s, w, scale, lane);
                wave_lds_sync();
                const cx<T>* g = taps + (u * p.n_rx + a) * p.n_taps;
                double e2 = 0.0, p2 = 0.0;
                for (int k = lane; k < s.N; k += 64) {
                    const cx<T> est = cazac_bin<T>(h, s.n_tap, k, s.N, w);
                    cx<T> H = mk<T>(0, 0);
                    for (int i = 0; i < p.n_taps; ++i)
                        H = cfma4(g[i], w[mod_small(k * s_delay[i], s.N, s.inv_N)], H);        // k d_i < N ne
                    const cx<T> d = csub(est, H);
                    e2 += (double)(d.x * d.x + d.y * d.y);
                    p2 += (double)(H.x * H.x + H.y * H.y);
                }
                e2 = wave_sum_f64(e2);
                p2 = wave_sum_f64(p2);
                if (lane == 0) {     // antennas are added in index order by the one lane that owns the realization's outputs
                    double* pe = err + r * p.n_users + u;
                    double* pp = pow + r * p.n_users + u;
                    *pe = a == 0 ? e2 : *pe + e2;
                    *pp = a == 0 ? p2 : *pp + p2;
                }
                wave_lds_sync();
            }
        }
    }
}

template <typename T>
int run_chanest_impl(mcle_ctx* ctx, const mcle_chanest_cfg* cfg, uint64_t seed, uint64_t first, uint64_t count, double* d_err,
                     double* d_pow) {
    ChanestParams p;
    p.s = cazac_shape(cfg->ne, cfg->num_taps_to_keep, cfg->size_multiplier);
    p.n_users = cfg->n_users, p.n_rx = cfg->n_rx, p.n_taps = cfg->n_taps, p.half = (cfg->ne + 1) / 2;
    p.normalized = cfg->normalized != 0;
    p.sigma = std::sqrt(cfg->noise_var);
    chanest_tap_profile(cfg, p.amp, p.delay);
    int rc;
    void* tw = nullptr;
    if ((rc = ctx->get_twiddles(p.s.N, sizeof(T) == 8 ? MCLE_F64 : MCLE_F32, &tw))) return rc;
    const size_t n_draw = (size_t)cfg->n_users * cfg->n_rx * cfg->n_taps;
    int waves, twl;
    size_t lds;
    // (the static delay / amplitude arrays: 96 + 192 bytes, rounded up)
    cazac_lds_plan((size_t)p.s.N * sizeof(cx<T>), (n_draw + 2 * (size_t)p.s.ne + p.s.n_tap) * sizeof(cx<T>), 512, &waves,
                   &twl, &lds);
    MCLE_REQUIRE(waves > 0, "chanest: ne %d with %d taps kept does not fit the device's LDS", p.s.ne, p.s.n_tap);
    lds -= 512;
    const uint64_t groups = (count + waves - 1) / waves;
    const uint64_t resident = (uint64_t)(ctx->n_cu > 0 ? ctx->n_cu : 256) * 2;
    const unsigned grid = (unsigned)oversubscribed_grid(ctx, resident, groups, 2);
    auto go = [&](auto kernel) -> int {
        // (the default limit covers 64 KiB, static arrays included: the common sizes launch without this host round trip)
        if (lds > 63 * 1024) MCLE_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * waves), lds, ctx->stream, p, (const cx<T>*)cfg->d_ref_seq, seed, first,
                           count, (const cx<T>*)tw, d_err, d_pow);
        MCLE_LAUNCH_CHECK();
        return MCLE_OK;
    };
    rc = twl ? go(k_chanest<T, true>) : go(k_chanest<T, false>);
    if (rc == MCLE_OK) ctx->set_kernel("chanest %s w%d%s", sizeof(T) == 8 ? "f64" : "f32", waves, twl ? "" : " gtw");
    return rc;
}

}  // namespace mcle

using namespace mcle;

extern "C" {

int mcle_cazac_estimate(mcle_ctx* ctx, int dtype, const void* d_ref_seq, int ne, const void* d_rx, size_t rows, int n_cover,
                        const double* cover, int num_taps_to_keep, int size_multiplier, int normalized, void* d_out) {
    if (ctx) ctx->last_kernel[0] = 0;
    MCLE_REQUIRE(ctx != nullptr, "null context");
    MCLE_REQUIRE(dtype == MCLE_F32 || dtype == MCLE_F64, "dtype must be MCLE_F32 or MCLE_F64");
    int rc;
    if ((rc = cazac_check_sizes(ne, size_multiplier))) return rc;
    MCLE_REQUIRE(num_taps_to_keep >= 0 && num_taps_to_keep < ne, "num_taps_to_keep must be in [0, ne) (got %d, ne %d)",
                 num_taps_to_keep, ne);
    MCLE_REQUIRE(n_cover >= 1 && n_cover <= kCazacMaxCover, "the cover code has 1 .. %d elements (got %d)", kCazacMaxCover,
                 n_cover);
    MCLE_REQUIRE(n_cover == 1 || cover != nullptr, "null cover code");
    if (rows == 0) return MCLE_OK;
    MCLE_REQUIRE(d_ref_seq != nullptr && d_rx != nullptr && d_out != nullptr, "null array");
    if ((rc = ctx->bind())) return rc;
    void* tw = nullptr;
    if ((rc = ctx->get_twiddles(size_multiplier * ne, dtype, &tw))) return rc;
    CoverCode cc;
    for (int c = 0; c < kCazacMaxCover; ++c) cc.c[c] = (cover && c < n_cover) ? cover[c] : 1.0;
    const CazacShape s = cazac_shape(ne, num_taps_to_keep, size_multiplier);
    return dtype == MCLE_F32 ? launch_cazac<float>(ctx, d_ref_seq, d_rx, rows, n_cover, cc, s, normalized, tw, d_out)
                             : launch_cazac<double>(ctx, d_ref_seq, d_rx, rows, n_cover, cc, s, normalized, tw, d_out);
}

int mcle_run_chanest(mcle_ctx* ctx, int dtype, const mcle_chanest_cfg* cfg, uint64_t seed, uint64_t first, uint64_t count,
                     double* d_err, double* d_pow) {
    if (ctx) ctx->last_kernel[0] = 0;
    MCLE_REQUIRE(ctx != nullptr && cfg != nullptr, "null argument");
    MCLE_REQUIRE(dtype == MCLE_F32 || dtype == MCLE_F64, "dtype must be MCLE_F32 or MCLE_F64");
    int rc;
    if ((rc = chanest_check_cfg(cfg, count))) return rc;
    if (count == 0) return MCLE_OK;
    MCLE_REQUIRE(cfg->d_ref_seq != nullptr && d_err != nullptr && d_pow != nullptr, "null array");
    if ((rc = ctx->bind())) return rc;
    return dtype == MCLE_F32 ? run_chanest_impl<float>(ctx, cfg, seed, first, count, d_err, d_pow)
                             : run_chanest_impl<double>(ctx, cfg, seed, first, count, d_err, d_pow);
}

}  // extern "C"
