// pipeline_hex.hip -- hexagonal-cell system level: a cluster of 1 .. 19 hexagonal cells with a base station in every centre, the
// operator on injected points (mcle_hex_gains: distances, gains, SINR, best cell) and the fused Monte Carlo over user drops
// (mcle_run_hex_drops: random placement, gains, SINR, capacity, the per-realization path-loss records mcle_run_comp reads).
// Reference: apps/comp_BD/simulate_comp.py ('Random' user positioning, :159-220), cell/cell.py Cluster / Cell.add_random_user,
// channels/pathloss.py PathLossGeneral with handle_small_distances_bool set.  The geometry tables (cell centres, wrapped copies,
// external radius) come from the host (pyphysim_amd/cell.py) in the parameter block.
//
// Arithmetic.  Positions, offsets and squared distances are f64 in both instantiations; from log2 of the squared distance on
// everything is T.  A loss is kept in the log2 domain, loss2 = loss_dB log2(10) / 10, so that a gain is ONE exp2(-loss2):
//     GENERAL   10 n log10(d s) + C  =  (n / 2) log2(d^2) + k  =  n log2(d) + k                         [times log2(10) / 10]
// clamped at 0 dB from below (d = 0: log2(0) = -inf -> 0 dB, gain 1).  The interferer stands at external_radius - |p - centre|
// (clamped at 0 from below: a point on or beyond the external circle is ON the interferer).
//
// Placement.  Attempt t of user q of drop r takes the uniforms 2 (q A + t) and 2 (q A + t) + 1 of STREAM_DROP (A = 128): one
// Philox block per two attempts.  The candidate is centre + (2 (u - 1/2)) r per axis, formed WITHOUT contraction (the host
// statement forms it in separate roundings and positions are compared bit for bit: hex_rounded); it is taken when strictly
// inside the cell (|y| < h and sqrt(3) |x| + |y| < 2 h on the offset) and not closer than min_dist_ratio r to the centre.
//
// Drops: one drop per wavefront, user q = cell U + slot on lane q % 64 (UPL = 1, 2 or 4 users per lane).  A user's figures
// depend on its own position alone, the per-drop sums are a lane-ordered slot sum followed by a fixed DPP tree (wave_lanes.hpp)
// and the histogram is exact integers: NO OUTPUT DEPENDS ON THE GRID, ON MCLE_OPT_GRID_OVERSUB OR ON HOW [first, first + count)
// IS SPLIT, bit for bit.  The histogram lives in LDS per workgroup and is flushed once with 64-bit atomics that skip zeros
// (totals.hpp).
#include <cfloat>
#include <cmath>

#include "philox.hpp"
#include "pipe_common.hpp"
#include "wave_lanes.hpp"

namespace mcle {

constexpr int kHexMaxCells = 19, kHexMaxPos = MCLE_HEX_MAX_POS, kHexMaxUsers = 256, kHexMaxBins = 256, kHexMaxExt = 8;
constexpr int kHexWaves = 4;             // wavefronts (drops in flight) per workgroup
constexpr int kHexAttempts = 128;        // A of the placement ledger
constexpr double kHexDbPerLog2 = 3.0102999566398119521;      // 10 log10(x) = kHexDbPerLog2 log2(x)
constexpr double kHexSqrt3 = 1.7320508075688772;             // sqrt(3.0) rounded to f64

struct HexParams {
    int K, U, KU, E, bins, n_pos;
    int start[kHexMaxCells + 1];                             // cell c owns positions [start[c], start[c + 1]): centre, then copies
    double px[kHexMaxPos], py[kHexMaxPos];
    double ccx, ccy, ext_radius;                             // cluster centre, external radius
    double r, h, two_h, min2;                                // cell radius, height, 2 h, (min_dist_ratio r)^2
    double a2, k2;                                           // log2-domain constants: loss2 = a2 log2(d^2) + k2 = 2 a2 log2(d) + k2
    double tx, noise, pe, hist_lo, hist_step;
};

template <typename T> struct HexConsts {
    T a2, a1, k2, tx, noise, pe;
    __device__ explicit HexConsts(const HexParams& p)
        : a2((T)p.a2), a1((T)(2.0 * p.a2)), k2((T)p.k2), tx((T)p.tx), noise((T)p.noise), pe((T)p.pe) {}
};

// v_log_f32 / v_exp_f32 in f32 (one unit in the last place each), the device libm in f64
__device__ __forceinline__ float hex_log2(float x) { return __builtin_amdgcn_logf(x); }
__device__ __forceinline__ double hex_log2(double x) { return log2(x); }
__device__ __forceinline__ float hex_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ double hex_exp2(double x) { return exp2(x); }

// gain of a base station at squared distance d2, of the interferer at distance de; a negative loss is 0 dB
template <typename T, int MODEL> __device__ __forceinline__ T hex_gain_d2(const HexConsts<T>& k, double d2) {
    if constexpr (MODEL == MCLE_HEX_PL_NONE) return (T)1;
    const T loss = fma(k.a2, hex_log2((T)d2), k.k2);
    return hex_exp2(-(loss < (T)0 ? (T)0 : loss));
}
template <typename T, int MODEL> __device__ __forceinline__ T hex_gain_d(const HexConsts<T>& k, double de) {
    if constexpr (MODEL == MCLE_HEX_PL_NONE) return (T)1;
    const T loss = fma(k.a1, hex_log2((T)de), k.k2);
    return hex_exp2(-(loss < (T)0 ? (T)0 : loss));
}

struct HexLds {
    double px[kHexMaxPos], py[kHexMaxPos];
    int start[kHexMaxCells + 1];
};

__device__ __forceinline__ void hex_build_table(const HexParams& p, HexLds& s) {
    const int tid = threadIdx.x;
    if (tid < kHexMaxPos) {
        s.px[tid] = tid < p.n_pos ? p.px[tid] : 0.0;
        s.py[tid] = tid < p.n_pos ? p.py[tid] : 0.0;
    }
    if (tid <= kHexMaxCells) s.start[tid] = tid <= p.K ? p.start[tid] : p.n_pos;
    __syncthreads();
}

// squared distance (f64) from (x, y) to cell c: its centre, or with WRAP the nearest of its positions (wave-uniform LDS reads)
template <bool WRAP> __device__ __forceinline__ double hex_cell_d2(const HexLds& s, int c, double x, double y) {
    if constexpr (!WRAP) {
        const double dx = x - s.px[c], dy = y - s.py[c];
        return fma(dx, dx, dy * dy);
    } else {
        double best = INFINITY;
        for (int i = s.start[c]; i < s.start[c + 1]; ++i) {
            const double dx = x - s.px[i], dy = y - s.py[i];
            best = fmin(best, fma(dx, dx, dy * dy));
        }
        return best;
    }
}

// distance of (x, y) to the interferer: external_radius - |p - cluster centre|, not below 0
__device__ __forceinline__ double hex_ext_dist(const HexParams& p, double x, double y) {
    return fmax(p.ext_radius - hypot(x - p.ccx, y - p.ccy), 0.0);
}

__device__ __forceinline__ double hex_db(double sinr) { return kHexDbPerLog2 * log2(sinr); }

// ---- the operator on injected points: one point per thread ------------------------------------------------------------------
template <typename T, int MODEL, bool WRAP>
__global__ __launch_bounds__(256) void k_hex_gains(HexParams p, const double* __restrict__ points, uint64_t n_points,
                                                   double* __restrict__ dist, double* __restrict__ gain,
                                                   double* __restrict__ sinr_dB, int32_t* __restrict__ assoc) {
    __shared__ HexLds s;
    hex_build_table(p, s);
    const HexConsts<T> k(p);
    const int K = p.K;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_points; i += (uint64_t)gridDim.x * 256) {
        const double x = points[2 * i], y = points[2 * i + 1];
        // the best cell so far with its gain, every other gain summed: when a better cell appears the old best's gain moves
        // into the sum (the interference is never formed as total minus desired)
        T gbest = 0, sum = 0;
        int best = 0;
        for (int c = 0; c < K; ++c) {
            const double d2 = hex_cell_d2<WRAP>(s, c, x, y);
            const T g = hex_gain_d2<T, MODEL>(k, d2);
            if (dist) dist[i * (uint64_t)K + c] = sqrt(d2);
            if (gain) gain[i * (uint64_t)(K + 1) + c] = (double)g;
            if (c == 0 || g > gbest) {
                sum += gbest;
                gbest = g;
                best = c;
            } else {
                sum += g;
            }
        }
        const T ge = hex_gain_d<T, MODEL>(k, hex_ext_dist(p, x, y));
        if (gain) gain[i * (uint64_t)(K + 1) + K] = (double)ge;
        if (sinr_dB) sinr_dB[i] = hex_db((double)((k.tx * gbest) / fma(k.tx, sum, fma(k.pe, ge, k.noise))));
        if (assoc) assoc[i] = best;
    }
}

// ---- the drops: one drop per wavefront -------------------------------------------------------------------------------------
struct HexDropOut {
    int32_t* flags;
    double* records;
    double* pos_out;
    double* sinr_dB;
    double* capacity;
    unsigned long long* hist;
    double* sum_capacity;
    double* min_sinr_dB;
};

struct HexDropTail {
    HexDropOut out;
    double hist_lo, hist_step;
    int bins;
};

// A product the backend may not fuse into the addition that follows: the library is built with -ffp-contract=fast, which
// lets the code generator contract across statements whatever a pragma says; an empty asm statement that "modifies" the value
// ends the pattern.
__device__ __forceinline__ double hex_rounded(double v) {
    asm volatile("" : "+v"(v));
    return v;
}

// one placement attempt from two Philox words; every product and sum is rounded on its own
__device__ __forceinline__ bool hex_attempt(const HexParams& p, double cx, double cy, uint32_t wx, uint32_t wy, double& x,
                                            double& y) {
    const double ux = (double)wx * 0x1p-32, uy = (double)wy * 0x1p-32;
    x = cx + hex_rounded((2.0 * (ux - 0.5)) * p.r);
    y = cy + hex_rounded((2.0 * (uy - 0.5)) * p.r);
    const double dx = x - cx, dy = y - cy;
    const double ax = fabs(dx), ay = fabs(dy);
    const double reach = hex_rounded(kHexSqrt3 * ax);
    const double d2 = hex_rounded(dx * dx) + hex_rounded(dy * dy);
    return ay < p.h && reach + ay < p.two_h && !(d2 < p.min2);
}

template <typename T, int MODEL, int UPL, bool WRAP>
__global__ __launch_bounds__(64 * kHexWaves) void k_hex_drops(HexParams p, uint64_t seed, uint64_t first, uint64_t count,
                                                              const double* __restrict__ positions, HexDropOut out) {
    __shared__ HexLds s;
    __shared__ unsigned long long s_hist[kHexMaxBins + 2];
    __shared__ HexDropTail s_tail;       // (the output pointers wait in LDS, not in SGPRs over the whole drop loop: pipeline_indoor.hip)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int i = tid; i < kHexMaxBins + 2; i += 64 * kHexWaves) s_hist[i] = 0ull;
    if (tid == 0) {
        s_tail.out = out;
        s_tail.hist_lo = p.hist_lo, s_tail.hist_step = p.hist_step, s_tail.bins = p.bins;
    }
    const HexDropTail& tl = s_tail;
    hex_build_table(p, s);                                   // (ends with a barrier)
    const HexConsts<T> k(p);
    const int K = p.K, U = p.U, KU = p.KU, cols = p.K + p.E;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);

    for (uint64_t d = (uint64_t)blockIdx.x * kHexWaves + wave; d < count; d += (uint64_t)gridDim.x * kHexWaves) {
        const Rng rng(seed, first + d);
        double x[UPL], y[UPL];
        int cell[UPL];
        bool bad = false;
#pragma unroll
        for (int j = 0; j < UPL; ++j) {
            const int q = lane + 64 * j;
            x[j] = 0.0, y[j] = 0.0, cell[j] = 0;
            if (q < KU) {
                cell[j] = q / U;
                if (positions) {
                    x[j] = positions[(d * (uint64_t)KU + q) * 2];
                    y[j] = positions[(d * (uint64_t)KU + q) * 2 + 1];
                } else {
                    const int ci = s.start[cell[j]];
                    const double cx = s.px[ci], cy = s.py[ci];
                    const uint32_t blk0 = (uint32_t)q * (kHexAttempts / 2);
                    bool found = false;
                    for (int tb = 0; tb < kHexAttempts / 2 && !found; ++tb) {
                        const Words4 b = rng.block(STREAM_DROP, blk0 + (uint32_t)tb);
                        found = hex_attempt(p, cx, cy, b.w[0], b.w[1], x[j], y[j]);
                        if (!found) found = hex_attempt(p, cx, cy, b.w[2], b.w[3], x[j], y[j]);
                    }
                    bad = bad || !found;
                }
            }
        }
        const bool fail = __ballot(bad) != 0ull;             // some user ran out of attempts: the whole drop is flagged
        T own[UPL], sum[UPL];
#pragma unroll
        for (int j = 0; j < UPL; ++j) own[j] = 0, sum[j] = 0;
        for (int c = 0; c < K; ++c) {
#pragma unroll
            for (int j = 0; j < UPL; ++j) {
                const int q = lane + 64 * j;
                if (q >= KU) continue;                       // (a lane without a user is masked; a slot without any is skipped)
                const T g = hex_gain_d2<T, MODEL>(k, hex_cell_d2<WRAP>(s, c, x[j], y[j]));
                if (c == cell[j])
                    own[j] = g;
                else
                    sum[j] += g;                             // the other cells, in cell order
                if (tl.out.records) tl.out.records[(d * (uint64_t)KU + q) * cols + c] = fail ? nan : (double)g;
            }
        }
        double cap_sum = 0.0, db_min = INFINITY;
#pragma unroll
        for (int j = 0; j < UPL; ++j) {
            const int q = lane + 64 * j;
            if (q < KU) {
                const T ge = hex_gain_d<T, MODEL>(k, hex_ext_dist(p, x[j], y[j]));
                const double sinr = (double)((k.tx * own[j]) / fma(k.tx, sum[j], fma(k.pe, ge, k.noise)));
                const double db = hex_db(sinr), cap = log2(1.0 + sinr);
                cap_sum += cap;
                db_min = fmin(db_min, db);
                const uint64_t o = d * (uint64_t)KU + q;
                if (tl.out.records)
                    for (int e = 0; e < p.E; ++e) tl.out.records[o * cols + K + e] = fail ? nan : (double)ge;
                if (tl.out.pos_out) {
                    tl.out.pos_out[2 * o] = fail ? nan : x[j];
                    tl.out.pos_out[2 * o + 1] = fail ? nan : y[j];
                }
                if (tl.out.sinr_dB) tl.out.sinr_dB[o] = fail ? nan : db;
                if (tl.out.capacity) tl.out.capacity[o] = fail ? nan : cap;
                if (tl.out.hist && !fail) {
                    int slot = 0;
                    if (!(db < tl.hist_lo)) {
                        const double t = floor((db - tl.hist_lo) / tl.hist_step);
                        slot = (tl.bins == 0 || !(t < (double)tl.bins)) ? tl.bins + 1 : 1 + (int)t;
                    }
                    atomicAdd(&s_hist[slot], 1ull);
                }
            }
        }
        cap_sum = wave_total_f64(cap_sum);
        db_min = wave_min_f64(db_min);
        if (lane == 0) {
            if (tl.out.flags) tl.out.flags[d] = fail ? 1 : 0;
            if (tl.out.sum_capacity) tl.out.sum_capacity[d] = fail ? nan : cap_sum;
            if (tl.out.min_sinr_dB) tl.out.min_sinr_dB[d] = fail ? nan : db_min;
        }
    }
    __syncthreads();
    // (a zero is not added: totals.hpp)
    if (tl.out.hist)
        for (int i = tid; i < tl.bins + 2; i += 64 * kHexWaves)
            if (s_hist[i]) atomicAdd(&tl.out.hist[i], s_hist[i]);
}

// ---- host side -------------------------------------------------------------------------------------------------------------
// The argument rules both entry points share (before the context and the pointers) and the kernel's parameter block
static int hex_check(int dtype, const mcle_hex_cfg* cfg, bool drops, HexParams& p) {
    MCLE_REQUIRE(dtype == MCLE_F32 || dtype == MCLE_F64, "dtype must be MCLE_F32 or MCLE_F64");
    MCLE_REQUIRE(cfg != nullptr, "null hex cfg");
    MCLE_REQUIRE(cfg->num_cells >= 1 && cfg->num_cells <= kHexMaxCells, "num_cells must be in [1, %d] (got %d)", kHexMaxCells,
                 cfg->num_cells);
    const int K = cfg->num_cells;
    MCLE_REQUIRE(cfg->model == MCLE_HEX_PL_NONE || cfg->model == MCLE_HEX_PL_GENERAL, "model must be 0 (none) or 1 (general) (got %d)",
                 cfg->model);
    MCLE_REQUIRE(cfg->wrap_around == 0 || cfg->wrap_around == 1, "wrap_around must be 0 or 1 (got %d)", cfg->wrap_around);
    MCLE_REQUIRE(!cfg->wrap_around || K == 19, "wrap_around needs num_cells = 19 (got %d)", K);
    MCLE_REQUIRE(cfg->n_ext >= 0 && cfg->n_ext <= kHexMaxExt, "n_ext must be in [0, %d] (got %d)", kHexMaxExt, cfg->n_ext);
    if (drops) {
        MCLE_REQUIRE(cfg->users_per_cell >= 1 && (long long)K * cfg->users_per_cell <= kHexMaxUsers,
                     "users_per_cell must be at least 1 with num_cells * users_per_cell <= %d (got %d x %d)", kHexMaxUsers, K,
                     cfg->users_per_cell);
        MCLE_REQUIRE(std::isfinite(cfg->min_dist_ratio) && cfg->min_dist_ratio >= 0.0 && cfg->min_dist_ratio <= 0.7,
                     "min_dist_ratio must be in [0, 0.7] (got %g)", cfg->min_dist_ratio);
        MCLE_REQUIRE(cfg->hist_bins >= 0 && cfg->hist_bins <= kHexMaxBins, "hist_bins must be in [0, %d] (got %d)", kHexMaxBins,
                     cfg->hist_bins);
        if (cfg->hist_bins > 0)
            MCLE_REQUIRE(std::isfinite(cfg->hist_lo_dB) && std::isfinite(cfg->hist_step_dB) && cfg->hist_step_dB > 0.0,
                         "hist_lo_dB must be finite and hist_step_dB positive");
        else
            MCLE_REQUIRE(std::isfinite(cfg->hist_lo_dB), "hist_lo_dB must be finite");
    }
    MCLE_REQUIRE(std::isfinite(cfg->cell_radius) && cfg->cell_radius > 0.0, "cell_radius must be positive");
    if (cfg->model == MCLE_HEX_PL_GENERAL) {
        MCLE_REQUIRE(std::isfinite(cfg->pl_n) && cfg->pl_n > 0.0, "pl_n must be positive");
        MCLE_REQUIRE(std::isfinite(cfg->pl_C), "pl_C must be finite");
        MCLE_REQUIRE(std::isfinite(cfg->dist_scale) && cfg->dist_scale > 0.0, "dist_scale must be positive");
    }
    MCLE_REQUIRE(std::isfinite(cfg->tx_power) && cfg->tx_power > 0.0, "tx_power must be positive");
    MCLE_REQUIRE(std::isfinite(cfg->noise_power) && cfg->noise_power > 0.0, "noise_power must be positive");
    MCLE_REQUIRE(std::isfinite(cfg->ext_power) && cfg->ext_power >= 0.0, "ext_power must be non-negative");
    if (dtype == MCLE_F32) {
        // all three are rounded to f32: a power that is no normal f32 number would make the SINR of a lone cell inf or NaN
        MCLE_REQUIRE(cfg->tx_power >= (double)FLT_MIN && cfg->tx_power <= (double)FLT_MAX,
                     "tx_power must be a normal f32 number (1.18e-38 .. 3.4e38) in f32 arithmetic (got %g)", cfg->tx_power);
        MCLE_REQUIRE(cfg->noise_power >= (double)FLT_MIN && cfg->noise_power <= (double)FLT_MAX,
                     "noise_power must be a normal f32 number (1.18e-38 .. 3.4e38) in f32 arithmetic (got %g)", cfg->noise_power);
        MCLE_REQUIRE(cfg->ext_power == 0.0 || (cfg->ext_power >= (double)FLT_MIN && cfg->ext_power <= (double)FLT_MAX),
                     "ext_power must be 0 or a normal f32 number (1.18e-38 .. 3.4e38) in f32 arithmetic (got %g)", cfg->ext_power);
    }
    // the geometry tables of the host
    MCLE_REQUIRE(cfg->n_pos >= K && cfg->n_pos <= kHexMaxPos, "n_pos must be in [num_cells, %d] (got %d)", kHexMaxPos, cfg->n_pos);
    MCLE_REQUIRE(cfg->pos_start[0] == 0 && cfg->pos_start[K] == cfg->n_pos, "pos_start must run from 0 to n_pos");
    for (int c = 0; c < K; ++c) {
        const int len = cfg->pos_start[c + 1] - cfg->pos_start[c];
        MCLE_REQUIRE(len >= 1 && (cfg->wrap_around ? len <= 4 : len == 1),
                     "pos_start: cell %d must own %s (got %d)", c + 1, cfg->wrap_around ? "1 to 4 positions" : "one position", len);
    }
    for (int i = 0; i < cfg->n_pos; ++i)
        MCLE_REQUIRE(std::isfinite(cfg->pos_x[i]) && std::isfinite(cfg->pos_y[i]), "pos_x / pos_y must be finite (entry %d)", i);
    MCLE_REQUIRE(std::isfinite(cfg->external_radius) && cfg->external_radius > 0.0, "external_radius must be positive");
    MCLE_REQUIRE(std::isfinite(cfg->centre_x) && std::isfinite(cfg->centre_y), "centre_x / centre_y must be finite");

    std::memset(&p, 0, sizeof(p));
    p.K = K, p.U = drops ? cfg->users_per_cell : 0, p.KU = K * p.U, p.E = cfg->n_ext, p.n_pos = cfg->n_pos;
    p.bins = drops ? cfg->hist_bins : 0;
    for (int c = 0; c <= K; ++c) p.start[c] = cfg->pos_start[c];
    for (int i = 0; i < cfg->n_pos; ++i) p.px[i] = cfg->pos_x[i], p.py[i] = cfg->pos_y[i];
    p.ccx = cfg->centre_x, p.ccy = cfg->centre_y, p.ext_radius = cfg->external_radius;
    p.r = cfg->cell_radius;
    p.h = std::sqrt(3.0) * cfg->cell_radius / 2.0;
    p.two_h = 2.0 * p.h;
    const double m = drops ? cfg->min_dist_ratio * cfg->cell_radius : 0.0;
    p.min2 = m * m;
    if (cfg->model == MCLE_HEX_PL_GENERAL) {
        const double c2 = std::log2(10.0) / 10.0;
        p.a2 = cfg->pl_n / 2.0;
        p.k2 = (10.0 * cfg->pl_n * std::log10(cfg->dist_scale) + cfg->pl_C) * c2;
    }
    p.tx = cfg->tx_power, p.noise = cfg->noise_power, p.pe = cfg->ext_power;
    p.hist_lo = cfg->hist_lo_dB, p.hist_step = p.bins > 0 ? cfg->hist_step_dB : 1.0;
    return MCLE_OK;
}

template <typename T, int MODEL>
static int launch_hex_gains(mcle_ctx* ctx, const HexParams& p, bool wrap, const double* d_points, size_t n, double* d_dist,
                            double* d_gain, double* d_sinr_dB, int32_t* d_assoc) {
    const unsigned grid = (unsigned)grid_for(ctx, n, 256, 8);
    if (wrap)
        hipLaunchKernelGGL((k_hex_gains<T, MODEL, true>), dim3(grid), dim3(256), 0, ctx->stream, p, d_points, (uint64_t)n, d_dist,
                           d_gain, d_sinr_dB, d_assoc);
    else
        hipLaunchKernelGGL((k_hex_gains<T, MODEL, false>), dim3(grid), dim3(256), 0, ctx->stream, p, d_points, (uint64_t)n, d_dist,
                           d_gain, d_sinr_dB, d_assoc);
    MCLE_LAUNCH_CHECK();
    return MCLE_OK;
}

template <typename T, int MODEL, bool WRAP>
static int launch_hex_drops(mcle_ctx* ctx, const HexParams& p, uint64_t seed, uint64_t first, uint64_t count,
                            const double* d_positions, const HexDropOut& out, int& upl) {
    const uint64_t groups = (count + kHexWaves - 1) / kHexWaves;
    const unsigned grid = (unsigned)oversubscribed_grid(ctx, (uint64_t)(ctx->n_cu > 0 ? ctx->n_cu : 256) * 8, groups, 2);
    upl = p.KU <= 64 ? 1 : p.KU <= 128 ? 2 : 4;
#define MCLE_HEX_GO(UPL_)                                                                                                      \
    hipLaunchKernelGGL((k_hex_drops<T, MODEL, UPL_, WRAP>), dim3(grid), dim3(64 * kHexWaves), 0, ctx->stream, p, seed, first,  \
                       count, d_positions, out)
    if (upl == 1)
        MCLE_HEX_GO(1);
    else if (upl == 2)
        MCLE_HEX_GO(2);
    else
        MCLE_HEX_GO(4);
#undef MCLE_HEX_GO
    MCLE_LAUNCH_CHECK();
    return MCLE_OK;
}

}  // namespace mcle

using namespace mcle;

extern "C" {

int mcle_hex_gains(mcle_ctx* ctx, int dtype, const mcle_hex_cfg* cfg, const double* d_points, size_t n, double* d_dist,
                   double* d_gain, double* d_sinr_dB, int32_t* d_assoc) {
    if (ctx) ctx->last_kernel[0] = 0;
    HexParams p;
    int rc;
    if ((rc = hex_check(dtype, cfg, false, p))) return rc;
    MCLE_REQUIRE((uint64_t)n <= 0x7fffffffull, "n must be at most 2^31-1");
    MCLE_REQUIRE(ctx != nullptr, "null context");
    if (n == 0) return MCLE_OK;
    MCLE_REQUIRE(d_points != nullptr, "null d_points");
    if ((rc = ctx->bind())) return rc;
    const bool wrap = cfg->wrap_around != 0;
#define MCLE_HEX_OP(T_, M_) rc = launch_hex_gains<T_, M_>(ctx, p, wrap, d_points, n, d_dist, d_gain, d_sinr_dB, d_assoc)
    switch (cfg->model * 2 + (dtype == MCLE_F64)) {
        case 0: MCLE_HEX_OP(float, MCLE_HEX_PL_NONE); break;
        case 1: MCLE_HEX_OP(double, MCLE_HEX_PL_NONE); break;
        case 2: MCLE_HEX_OP(float, MCLE_HEX_PL_GENERAL); break;
        default: MCLE_HEX_OP(double, MCLE_HEX_PL_GENERAL); break;
    }
#undef MCLE_HEX_OP
    if (rc) return rc;
    ctx->set_kernel("hex_gains %s m%d w%d", dtype == MCLE_F64 ? "f64" : "f32", cfg->model, cfg->wrap_around);
    return MCLE_OK;
}

int mcle_run_hex_drops(mcle_ctx* ctx, int dtype, const mcle_hex_cfg* cfg, uint64_t seed, uint64_t first, uint64_t count,
                       const double* d_positions, int32_t* d_flags, double* d_records, double* d_pos_out, double* d_sinr_dB,
                       double* d_capacity, uint64_t* d_hist, double* d_sum_capacity, double* d_min_sinr_dB) {
    if (ctx) ctx->last_kernel[0] = 0;
    HexParams p;
    int rc;
    if ((rc = hex_check(dtype, cfg, true, p))) return rc;
    MCLE_REQUIRE(count <= 0x7fffffffull, "count must be at most 2^31-1 drops per call");
    MCLE_REQUIRE(ctx != nullptr, "null context");
    if (count == 0) return MCLE_OK;
    if ((rc = ctx->bind())) return rc;
    HexDropOut out;
    out.flags = d_flags, out.records = d_records, out.pos_out = d_pos_out, out.sinr_dB = d_sinr_dB, out.capacity = d_capacity;
    out.hist = (unsigned long long*)d_hist, out.sum_capacity = d_sum_capacity, out.min_sinr_dB = d_min_sinr_dB;
    int upl = 0;
#define MCLE_HEX_RUN(T_, M_)                                                                                         \
    rc = cfg->wrap_around ? launch_hex_drops<T_, M_, true>(ctx, p, seed, first, count, d_positions, out, upl)        \
                          : launch_hex_drops<T_, M_, false>(ctx, p, seed, first, count, d_positions, out, upl)
    switch (cfg->model * 2 + (dtype == MCLE_F64)) {
        case 0: MCLE_HEX_RUN(float, MCLE_HEX_PL_NONE); break;
        case 1: MCLE_HEX_RUN(double, MCLE_HEX_PL_NONE); break;
        case 2: MCLE_HEX_RUN(float, MCLE_HEX_PL_GENERAL); break;
        default: MCLE_HEX_RUN(double, MCLE_HEX_PL_GENERAL); break;
    }
#undef MCLE_HEX_RUN
    if (rc) return rc;
    ctx->set_kernel("hex_drops %s m%d u%d w%d", dtype == MCLE_F64 ? "f64" : "f32", cfg->model, upl, cfg->wrap_around);
    return MCLE_OK;
}

}  // extern "C"
