// kernels_chanest_ic.hip -- channel estimation with interference cancellation (reference: apps/simple_precoded_srs.py:127-205
// estimate_channels_remove_only_direct, :208-345 estimate_channels_remove_direct_and_perform_SIC): the staged cancellation
// operator and the fused estimation-error pipeline with a linear gain per user and three estimation rules.
//
//     mode 0   every user from the received comb Y
//     mode 1   the direct user d from Y;  R0[a][n] = Y[a][n] - H^_d[a][m n] r_d[n];  every other user from R0
//     mode 2   mode 1, then the others in descending order of the norm of their first estimates (an exact tie: the higher
//              index first); the strongest keeps its estimate, every later one is estimated again from the residual left by the
//              final estimates of all stronger ones
//
// No m Ne-bin spectrum is formed before the final error pass.  A subtraction needs the estimate at the comb bins only,
// H^[m n] = sum_t h[t] w[(m n t) mod N] (cazac_bin with k = m n: Ne (K + 1) FMAs), and the squared norm of an estimate over all
// N = m Ne bins is N sum_t |h[t]|^2 (Parseval: it is the N-point DFT of K + 1 <= N taps), so the order comes from the taps.
#include "cazac_common.hpp"

namespace mcle {

// ref [ne]; rx, out [rows][ne]; est [rows][m ne]: out[row][n] = rx[row][n] - est[row][m n] ref[n].  One wavefront per row;
// every element is read and written by the same lane, so out may be rx.
template <typename T>
__global__ __launch_bounds__(256) void k_cazac_cancel(const cx<T>* __restrict__ ref, const cx<T>* rx,
                                                      const cx<T>* __restrict__ est, size_t rows, int ne, int m, cx<T>* out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    for (size_t row = (size_t)blockIdx.x * waves + wave; row < rows; row += (size_t)gridDim.x * waves) {
        const cx<T>* y = rx + row * (size_t)ne;
        const cx<T>* e = est + row * (size_t)m * ne;
        cx<T>* dst = out + row * (size_t)ne;
        for (int n = lane; n < ne; n += 64) dst[n] = csub(y[n], cmul(e[m * n], ref[n]));
    }
}

template <typename T>
int launch_cazac_cancel(mcle_ctx* ctx, const void* d_ref, const void* d_rx, const void* d_est, size_t rows, int ne, int m,
                        void* d_out) {
    const size_t groups = (rows + 3) / 4;
    const size_t cap = (size_t)(ctx->n_cu > 0 ? ctx->n_cu : 256) * 8;
    const unsigned grid = (unsigned)(groups < cap ? groups : cap);
    hipLaunchKernelGGL(k_cazac_cancel<T>, dim3(grid), dim3(256), 0, ctx->stream, (const cx<T>*)d_ref, (const cx<T>*)d_rx,
                       (const cx<T>*)d_est, rows, ne, m, (cx<T>*)d_out);
    MCLE_LAUNCH_CHECK();
    ctx->set_kernel("cazac_cancel %s", sizeof(T) == 8 ? "f64" : "f32");
    return MCLE_OK;
}

// ---- fused estimation-error pipeline with cancellation ----------------------------------------------------------------------
// One wavefront per realization; the draws are those of k_chanest (mcle-philox-v1), the taps of user u times
// sqrt(link_gain[u]).
struct ChanestIcParams {
    CazacShape s;
    int n_users, n_rx, n_taps, half;      // half = ceil(ne / 2)
    int normalized, mode, direct;
    double sigma;
    double amp[MCLE_MAX_TAPS];
    int delay[MCLE_MAX_TAPS];
    double root_gain[kChanestMaxUsers];
};

// first estimate of user u from the comb (or residual) y [n_rx][ne]: K + 1 taps per antenna into he [n_rx][K + 1]
template <typename T>
__device__ __forceinline__ void ic_estimate(const cx<T>* y, cx<T>* z, cx<T>* he, const cx<T>* __restrict__ ref, int n_rx,
                                            const CazacShape& s, const cx<T>* w, T scale, int lane) {
    for (int a = 0; a < n_rx; ++a) {
        for (int n = lane; n < s.ne; n += 64) z[n] = cmulc(y[a * s.ne + n], ref[n]);
        wave_lds_sync();
        cazac_taps<T>(z, he + a * s.n_tap, s, w, scale, lane);
        wave_lds_sync();
    }
}

// y[a][n] -= H^[a][m n] ref[n] from the taps he [n_rx][K + 1]
template <typename T>
__device__ __forceinline__ void ic_cancel(cx<T>* y, const cx<T>* he, const cx<T>* __restrict__ ref, int n_rx,
                                          const CazacShape& s, const cx<T>* w, int lane) {
    for (int a = 0; a < n_rx; ++a)
        for (int n = lane; n < s.ne; n += 64) {
            const cx<T> H = cazac_bin<T>(he + a * s.n_tap, s.n_tap, s.m * n, s.N, w);          // m n < N
            y[a * s.ne + n] = csub(y[a * s.ne + n], cmul(H, ref[n]));
        }
    wave_lds_sync();
}

// the user whose lane holds place `st` of the order, the same in every lane (exactly one lane < n_users holds each place)
__device__ __forceinline__ int holder_of_place(int place, int st, int n_users, int lane) {
    return __ffsll((long long)__ballot(lane < n_users && place == st)) - 1;
}

// seq [n_users][ne]; err / pow [count][n_users]; order [count][n_users] or null.  LDS: delays, amplitudes and root gains, the
// table [N] when TWL, then per wavefront taps [n_users n_rx n_taps], y [n_rx][ne], z [ne], he [n_users][n_rx][K + 1].
template <typename T, bool TWL>
__global__ __launch_bounds__(256) void k_chanest_ic(ChanestIcParams p, const cx<T>* __restrict__ seq, uint64_t seed,
                                                    uint64_t first, uint64_t count, const cx<T>* __restrict__ tw,
                                                    double* __restrict__ err, double* __restrict__ pow,
                                                    int* __restrict__ order) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_delay[MCLE_MAX_TAPS];
    __shared__ T s_amp[MCLE_MAX_TAPS];
    __shared__ T s_gain[kChanestMaxUsers];
    cx<T>* base = reinterpret_cast<cx<T>*>(smem);
    const CazacShape& s = p.s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    // (indexed by the lane: read from the argument segment as memory, not held in scalar registers)
    if (threadIdx.x < MCLE_MAX_TAPS) {
        s_delay[threadIdx.x] = p.delay[threadIdx.x];
        s_amp[threadIdx.x] = (T)p.amp[threadIdx.x];
    }
    if (threadIdx.x < kChanestMaxUsers) s_gain[threadIdx.x] = (T)p.root_gain[threadIdx.x];
    const cx<T>* w = tw;
    if constexpr (TWL) {
        for (int j = threadIdx.x; j < s.N; j += blockDim.x) base[j] = tw[j];
        w = base;
        base += s.N;
    }
    __syncthreads();
    const int n_links = p.n_users * p.n_rx, n_draw = n_links * p.n_taps, per_user = p.n_rx * p.n_taps;
    const int he_user = p.n_rx * s.n_tap;
    cx<T>* taps = base + (size_t)wave * (n_draw + (p.n_rx + 1) * s.ne + p.n_users * he_user);
    cx<T>* y = taps + n_draw;
    cx<T>* z = y + p.n_rx * s.ne;
    cx<T>* he = z + s.ne;
    const T scale = p.normalized ? (T)1 : (T)(1.0 / s.ne);
    const int d0 = p.mode == 0 ? 0 : p.direct;          // who is estimated first
    const int n_steps = p.n_users + (p.mode == 2 && p.n_users > 2 ? p.n_users - 2 : 0);
    for (uint64_t r = (uint64_t)blockIdx.x * waves + wave; r < count; r += (uint64_t)gridDim.x * waves) {
        const Rng rng(seed, first + r);
        for (int d = lane; d < n_draw; d += 64)
            taps[d] = cscale(cn_sample<T>(rng, STREAM_CHAN, (uint64_t)d, s_amp[d % p.n_taps]), s_gain[d / per_user]);
        wave_lds_sync();
        // the received comb of every antenna: Y[a][n] = sum_u r_u[n] sum_i h_uai w[(m n d_i) mod N] + noise; a lane takes the
        // positions 2 j and 2 j + 1 one Philox block serves
        for (int a = 0; a < p.n_rx; ++a)
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
                    y[a * s.ne + n] = v[e];
                }
            }
        wave_lds_sync();
        // place of every user in the order of final estimates, held by lane u: the fixed order until mode 2 decides another
        int place = lane == d0 ? 0 : (lane < d0 ? lane + 1 : lane);
        // One loop over the estimation steps, so that the estimate and the subtraction are each inlined once.  Steps
        // 0 .. n_users - 1 are the first estimates: the direct user from Y, then the others in index order from Y (mode 0) or from
        // the residual R0; mode 2 adds n_users - 2 steps, the s-th strongest (s = 2, 3, ...) from the residual without the final
        // estimates of all stronger ones
        int prev = d0;
        for (int step = 0; step < n_steps; ++step) {
            int u;
            bool cancel;
            if (step < p.n_users) {
                u = step == 0 ? d0 : (step <= d0 ? step - 1 : step);
                cancel = step == 1 && p.mode != 0;
            } else {
                u = holder_of_place(place, step - p.n_users + 2, p.n_users, lane);
                cancel = true;
            }
            if (cancel) ic_cancel<T>(y, he + prev * he_user, seq + (size_t)prev * s.ne, p.n_rx, s, w, lane);
            ic_estimate<T>(y, z, he + u * he_user, seq + (size_t)u * s.ne, p.n_rx, s, w, scale, lane);
            if (step >= p.n_users) prev = u;
            if (step == p.n_users - 1 && p.mode == 2 && p.n_users > 1) {
                // the order by the norm of the first estimates: sum_a sum_t |h[t]|^2 (times N, which orders nothing), antennas
                // added in index order; the butterfly leaves the same double in every lane.  A norm that is NaN (a NaN in the
                // caller's sequences) counts as infinite: (norm, index) then orders any input totally, exactly one lane holds
                // each place and every entry of the order row is written
                double mine = 0.0;
                for (int v = 0; v < p.n_users; ++v) {
                    double nrm = 0.0;
                    for (int a = 0; a < p.n_rx; ++a) {
                        const cx<T>* h = he + v * he_user + a * s.n_tap;
                        double part = 0.0;
                        for (int t = lane; t < s.n_tap; t += 64) {
                            const double hx = (double)h[t].x, hy = (double)h[t].y;
                            part = fma(hx, hx, fma(hy, hy, part));
                        }
                        nrm += wave_sum_f64(part);
                    }
                    if (lane == v) mine = isnan(nrm) ? (double)INFINITY : nrm;
                }
                int stronger = 0;
                for (int v = 0; v < p.n_users; ++v) {
                    const double other = __shfl(mine, v, 64);
                    if (v != d0 && v != lane && (other > mine || (other == mine && v > lane))) ++stronger;
                }
                if (lane != d0) place = 1 + stronger;
                prev = holder_of_place(place, 1, p.n_users, lane);          // the strongest keeps its first estimate
            }
        }
        if (order != nullptr && lane < p.n_users) order[r * p.n_users + place] = lane;
        // final error pass: per user, antennas added in index order
        for (int u = 0; u < p.n_users; ++u) {
            double e_sum = 0.0, p_sum = 0.0;
            for (int a = 0; a < p.n_rx; ++a) {
                const cx<T>* g = taps + (u * p.n_rx + a) * p.n_taps;
                const cx<T>* h = he + u * he_user + a * s.n_tap;
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
                e_sum = a == 0 ? e2 : e_sum + e2;
                p_sum = a == 0 ? p2 : p_sum + p2;
            }
            if (lane == 0) {
                err[r * p.n_users + u] = e_sum;
                pow[r * p.n_users + u] = p_sum;
            }
        }
        wave_lds_sync();
    }
}

// complex elements of one wavefront's LDS: the drawn taps, the comb of every antenna, z and the kept taps of every link
inline size_t chanest_ic_per_wave(const mcle_chanest_cfg* cfg) {
    const size_t links = (size_t)cfg->n_users * cfg->n_rx;
    return links * cfg->n_taps + ((size_t)cfg->n_rx + 1) * cfg->ne + links * ((size_t)cfg->num_taps_to_keep + 1);
}

template <typename T>
int run_chanest_ic_impl(mcle_ctx* ctx, const mcle_chanest_ic_cfg* ic, uint64_t seed, uint64_t first, uint64_t count,
                        double* d_err, double* d_pow, int32_t* d_order) {
    const mcle_chanest_cfg* cfg = &ic->base;
    ChanestIcParams p;
    p.s = cazac_shape(cfg->ne, cfg->num_taps_to_keep, cfg->size_multiplier);
    p.n_users = cfg->n_users, p.n_rx = cfg->n_rx, p.n_taps = cfg->n_taps, p.half = (cfg->ne + 1) / 2;
    p.normalized = cfg->normalized != 0, p.mode = ic->mode, p.direct = ic->direct_user;
    p.sigma = std::sqrt(cfg->noise_var);
    chanest_tap_profile(cfg, p.amp, p.delay);
    for (int u = 0; u < kChanestMaxUsers; ++u) p.root_gain[u] = u < cfg->n_users ? std::sqrt(ic->link_gain[u]) : 0.0;
    int waves, twl;
    size_t lds;
    // (the static delay / amplitude / gain arrays: 96 + 192 + 64 bytes, rounded up)
    cazac_lds_plan((size_t)p.s.N * sizeof(cx<T>), chanest_ic_per_wave(cfg) * sizeof(cx<T>), 512, &waves, &twl, &lds);
    MCLE_REQUIRE(waves > 0, "chanest_ic: ne %d with %d taps kept, %d users and %d antennas does not fit the device's LDS",
                 p.s.ne, p.s.n_tap, p.n_users, p.n_rx);
    lds -= 512;
    int rc;
    if ((rc = ctx->bind())) return rc;
    void* tw = nullptr;
    if ((rc = ctx->get_twiddles(p.s.N, sizeof(T) == 8 ? MCLE_F64 : MCLE_F32, &tw))) return rc;
    const uint64_t groups = (count + waves - 1) / waves;
    const uint64_t resident = (uint64_t)(ctx->n_cu > 0 ? ctx->n_cu : 256) * 2;
    const unsigned grid = (unsigned)oversubscribed_grid(ctx, resident, groups, 2);
    auto go = [&](auto kernel) -> int {
        // (the default limit covers 64 KiB, static arrays included: the common sizes launch without this host round trip)
        if (lds > 63 * 1024) MCLE_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * waves), lds, ctx->stream, p, (const cx<T>*)cfg->d_ref_seq, seed, first,
                           count, (const cx<T>*)tw, d_err, d_pow, d_order);
        MCLE_LAUNCH_CHECK();
        return MCLE_OK;
    };
    rc = twl ? go(k_chanest_ic<T, true>) : go(k_chanest_ic<T, false>);
    if (rc == MCLE_OK) ctx->set_kernel("chanest_ic %s w%d%s", sizeof(T) == 8 ? "f64" : "f32", waves, twl ? "" : " gtw");
    return rc;
}

}  // namespace mcle

using namespace mcle;

extern "C" {

int mcle_cazac_cancel(mcle_ctx* ctx, int dtype, const void* d_ref_seq, int ne, const void* d_rx, const void* d_est, size_t rows,
                      int size_multiplier, void* d_out) {
    if (ctx) ctx->last_kernel[0] = 0;
    MCLE_REQUIRE(ctx != nullptr, "null context");
    MCLE_REQUIRE(dtype == MCLE_F32 || dtype == MCLE_F64, "dtype must be MCLE_F32 or MCLE_F64");
    int rc;
    if ((rc = cazac_check_sizes(ne, size_multiplier))) return rc;
    if (rows == 0) return MCLE_OK;
    MCLE_REQUIRE(d_ref_seq != nullptr && d_rx != nullptr && d_est != nullptr && d_out != nullptr, "null array");
    if ((rc = ctx->bind())) return rc;
    return dtype == MCLE_F32 ? launch_cazac_cancel<float>(ctx, d_ref_seq, d_rx, d_est, rows, ne, size_multiplier, d_out)
                             : launch_cazac_cancel<double>(ctx, d_ref_seq, d_rx, d_est, rows, ne, size_multiplier, d_out);
}

int mcle_run_chanest_ic(mcle_ctx* ctx, int dtype, const mcle_chanest_ic_cfg* cfg, uint64_t seed, uint64_t first,
                        uint64_t count, double* d_err, double* d_pow, int32_t* d_order) {
    if (ctx) ctx->last_kernel[0] = 0;
    MCLE_REQUIRE(ctx != nullptr && cfg != nullptr, "null argument");
    MCLE_REQUIRE(dtype == MCLE_F32 || dtype == MCLE_F64, "dtype must be MCLE_F32 or MCLE_F64");
    int rc;
    if ((rc = chanest_check_cfg(&cfg->base, count))) return rc;
    MCLE_REQUIRE(cfg->mode >= 0 && cfg->mode <= 2, "mode must be 0 (none), 1 (direct removed) or 2 (ordered SIC) (got %d)",
                 cfg->mode);
    MCLE_REQUIRE(cfg->direct_user >= 0 && cfg->direct_user < cfg->base.n_users, "direct_user must be in [0, n_users) (got %d)",
                 cfg->direct_user);
    for (int u = 0; u < cfg->base.n_users; ++u)
        MCLE_REQUIRE(cfg->link_gain[u] > 0.0 && std::isfinite(cfg->link_gain[u]),
                     "link gains must be positive and finite (user %d: %g)", u, cfg->link_gain[u]);
    if (count == 0) return MCLE_OK;
    MCLE_REQUIRE(cfg->base.d_ref_seq != nullptr && d_err != nullptr && d_pow != nullptr, "null array");
    return dtype == MCLE_F32 ? run_chanest_ic_impl<float>(ctx, cfg, seed, first, count, d_err, d_pow, d_order)
                             : run_chanest_ic_impl<double>(ctx, cfg, seed, first, count, d_err, d_pow, d_order);
}

}  // extern "C"
