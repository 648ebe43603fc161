// cazac_common.hpp -- what the channel-estimation translation units share (kernels_chanest.hip, kernels_chanest_ic.hip): the
// pruned direct DFTs of the CAZAC estimator over the one table w[j] = exp(-2 pi i j / (m Ne)), the lane plan of pass 1, the LDS
// plan and the argument rules of a mcle_chanest_cfg.
//     h[t] = (1 / Ne) sum_n conj(r[n]) y[n] conj(w[(m n t) mod m Ne])      t = 0 .. K      (pass 1, cazac_taps)
//     H[k] =          sum_t h[t]            w[(k t) mod m Ne]              k = 0 .. m Ne-1 (pass 2, cazac_bin)
// Twiddle indexes are stepped with a conditional subtract; the one product a lane needs at the start of its run is reduced
// with mod_small: no integer division in either DFT pass.  (The pipelines' tap draw does divide, once per drawn tap, to find
// the draw's tap and user.)
#pragma once
#include "philox.hpp"
#include "pipe_common.hpp"

namespace mcle {

constexpr int kCazacMaxN = 4096;     // table limit: size_multiplier * ne
constexpr int kCazacMaxCover = 8;
constexpr int kChanestMaxUsers = 8;
constexpr int kChanestMaxRx = 4;

// x mod n for 0 <= x <= 2^24 (exact in float) and 1 <= n <= 4096, inv = 1.0f / n: the float quotient is off by at most one
__host__ __device__ __forceinline__ int mod_small(int x, int n, float inv) {
    int r = x - (int)((float)x * inv) * n;
    if (r < 0) r += n;
    if (r >= n) r -= n;
    return r;
}

// acc + a * conj(b), four chained FMAs
template <typename C> __device__ __forceinline__ C cfmac4(C a, C b, C acc) {
    acc.x = fma(a.x, b.x, acc.x);
    acc.x = fma(a.y, b.y, acc.x);
    acc.y = fma(a.y, b.x, acc.y);
    acc.y = fma(-a.x, b.y, acc.y);
    return acc;
}

// How pass 1 spreads over the 64 lanes: TP = the power of two >= K + 1 (at most 64) lanes own a tap each, and the 64 / TP
// groups of them each walk `chunk` consecutive samples; the partial sums meet in log2(64 / TP) butterfly steps.  (With K = 15
// a lane-per-tap walk alone would leave 48 of the 64 lanes idle over the longer of the two passes.)
struct CazacShape {
    int ne, n_tap, m, N;     // N = m * ne
    int tp_shift, chunk;
    float inv_N;
};
inline CazacShape cazac_shape(int ne, int K, int m) {
    CazacShape s;
    s.ne = ne, s.n_tap = K + 1, s.m = m, s.N = m * ne;
    s.tp_shift = 0;
    while (s.tp_shift < 6 && (1 << s.tp_shift) < s.n_tap) ++s.tp_shift;
    const int parts = 64 >> s.tp_shift;
    s.chunk = (ne + parts - 1) / parts;
    s.inv_N = 1.0f / (float)s.N;
    return s;
}

// pass 1: z [ne] -> h [K + 1], both in the wavefront's LDS; `scale` = 1 / Ne (1 for a normalised sequence)
template <typename T>
__device__ __forceinline__ void cazac_taps(const cx<T>* z, cx<T>* h, const CazacShape& s, const cx<T>* w, T scale,
                                           int lane) {
    const int TP = 1 << s.tp_shift;
    const int tl = lane & (TP - 1), part = lane >> s.tp_shift;
    const int n0 = min(part * s.chunk, s.ne), n1 = min(n0 + s.chunk, s.ne);
    for (int tb = 0; tb < s.n_tap; tb += TP) {      // more than one trip only when K + 1 > 64 (then TP = 64, one part)
        const int t = tb + tl;
        cx<T> acc = mk<T>(0, 0);
        if (t < s.n_tap) {
            const int step = s.m * t;                               // < N
            int idx = mod_small(step * n0, s.N, s.inv_N);           // step * n0 < N * ne <= 2^24
#pragma unroll 4
            for (int n = n0; n < n1; ++n) {
                acc = cfmac4(z[n], w[idx], acc);
                idx += step;
                if (idx >= s.N) idx -= s.N;
            }
        }
        for (int off = TP; off < 64; off <<= 1) {
            acc.x += __shfl_xor(acc.x, off, 64);
            acc.y += __shfl_xor(acc.y, off, 64);
        }
        if (part == 0 && t < s.n_tap) h[t] = cscale(acc, scale);
    }
}

// pass 2, one bin: H[k] = sum_t h[t] w[(k t) mod N]
template <typename T>
__device__ __forceinline__ cx<T> cazac_bin(const cx<T>* h, int n_tap, int k, int N, const cx<T>* w) {
    cx<T> acc = mk<T>(0, 0);
    int idx = 0;
#pragma unroll 4
    for (int t = 0; t < n_tap; ++t) {
        acc = cfma4(h[t], w[idx], acc);
        idx += k;
        if (idx >= N) idx -= N;
    }
    return acc;
}

// Wavefronts per workgroup and whether the table goes to LDS, for `per_wave` + (table) bytes within the 160 KiB of a gfx950
// compute unit (mcle_ctx_create refuses every other device): the table stays in global memory (L2) only when nothing else fits
// beside it.
inline void cazac_lds_plan(size_t table_bytes, size_t per_wave, size_t fixed, int* waves, int* twl, size_t* lds) {
    const size_t budget = (size_t)160 * 1024;
    for (int t = 1; t >= 0; --t)
        for (int w = 4; w >= 1; w >>= 1) {
            const size_t need = fixed + (t ? table_bytes : 0) + (size_t)w * per_wave;
            if (need <= budget) {
                *waves = w, *twl = t, *lds = need;
                return;
            }
        }
    *waves = 0, *twl = 0, *lds = 0;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// The size rules every CAZAC entry point shares
inline int cazac_check_sizes(int ne, int size_multiplier) {
    MCLE_REQUIRE(ne >= 2, "the reference sequence needs at least 2 elements (got %d)", ne);
    MCLE_REQUIRE(size_multiplier >= 1, "size_multiplier must be positive (got %d)", size_multiplier);
    MCLE_REQUIRE((long long)size_multiplier * ne <= kCazacMaxN, "size_multiplier * ne must be <= %d (got %lld)", kCazacMaxN,
                 (long long)size_multiplier * ne);
    return MCLE_OK;
}

// The argument rules of a mcle_chanest_cfg and of the realization range (mcle_run_chanest, mcle_run_chanest_ic)
inline int chanest_check_cfg(const mcle_chanest_cfg* cfg, uint64_t count) {
    MCLE_REQUIRE(cfg->ne >= 2, "the reference sequence needs at least 2 elements (got %d)", cfg->ne);
    MCLE_REQUIRE(cfg->size_multiplier >= 1, "size_multiplier must be positive (got %d)", cfg->size_multiplier);
    MCLE_REQUIRE((long long)cfg->size_multiplier * cfg->ne <= kCazacMaxN, "size_multiplier * ne must be <= %d", kCazacMaxN);
    MCLE_REQUIRE(cfg->num_taps_to_keep >= 0 && cfg->num_taps_to_keep < cfg->ne, "num_taps_to_keep must be in [0, ne)");
    MCLE_REQUIRE(cfg->n_users >= 1 && cfg->n_users <= kChanestMaxUsers, "n_users must be in [1, %d]", kChanestMaxUsers);
    MCLE_REQUIRE(cfg->n_rx >= 1 && cfg->n_rx <= kChanestMaxRx, "n_rx must be in [1, %d]", kChanestMaxRx);
    MCLE_REQUIRE(cfg->n_taps >= 1 && cfg->n_taps <= MCLE_MAX_TAPS, "n_taps must be in [1, %d]", MCLE_MAX_TAPS);
    MCLE_REQUIRE(cfg->noise_var >= 0.0, "noise variance must be non-negative");
    double total = 0.0;
    for (int i = 0; i < cfg->n_taps; ++i) {
        MCLE_REQUIRE(cfg->tap_delay[i] >= 0 && cfg->tap_delay[i] < cfg->ne, "tap delays must be in [0, ne) (tap %d: %d)", i,
                     cfg->tap_delay[i]);
        MCLE_REQUIRE(cfg->tap_power[i] >= 0.0, "tap powers must be non-negative");
        total += cfg->tap_power[i];
    }
    MCLE_REQUIRE(total > 0.0, "the tap powers sum to zero");
    MCLE_REQUIRE(count <= 0x7fffffffull, "at most 2^31-1 realizations per call");
    return MCLE_OK;
}

// sqrt(p_i / sum p) per tap, zero beyond n_taps; delays alike
inline void chanest_tap_profile(const mcle_chanest_cfg* cfg, double* amp, int* delay) {
    double total = 0.0;
    for (int i = 0; i < cfg->n_taps; ++i) total += cfg->tap_power[i];
    for (int i = 0; i < MCLE_MAX_TAPS; ++i) {
        amp[i] = i < cfg->n_taps ? std::sqrt(cfg->tap_power[i] / total) : 0.0;
        delay[i] = i < cfg->n_taps ? cfg->tap_delay[i] : 0;
    }
}

}  // namespace mcle
