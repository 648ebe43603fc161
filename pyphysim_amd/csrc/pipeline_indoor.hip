// pipeline_indoor.hip -- indoor system level: one floor of n x n square rooms with access points (APs) in the room centres, the
// SINR heat-map operator (mcle_indoor_sinr) and the fused Monte Carlo over user drops (mcle_run_indoor_drops).  Reference:
// apps/metis_scenarios/simulate_metis_scenario.py (heat map, closest AP, every AP on) and simulate_metis_scenario2.py (random
// users, best channel, only the chosen APs on); channels/pathloss.py PathLossGeneral / PathLoss3GPP1 / PathLossFreeSpace /
// PathLossMetisPS7 with handle_small_distances_bool set.
//
// Arithmetic.  Positions, the room of a point (nearest centre, per axis, lowest index on a tie) and the wall count
// |row - row_ap| + |col - col_ap| are f64 / integer in both instantiations; dx, dy are taken in f64 and rounded once to T, and
// everything from d^2 on is T.  Every loss is kept in the log2 domain, loss2 = loss_dB log2(10) / 10, so that a gain is ONE
// exp2(-loss2):
//     GENERAL   10 n log10(d s) + C      =  (n / 2) log2(d^2) + k                                       [times log2(10) / 10]
//     METIS PS7 A log10(d) + B + F + X   =  (A / 20) log2(d^2) + k_los   or   (A' / 20) log2(d^2) + k_nlos + kx walls
// -- one log2 of d^2 per pair, no square root.  The path loss is clamped at 0 dB from below (d = 0: log2(0) = -inf -> 0) and the
// wall loss walls * wall_loss_dB is added to it for every model.
//
// Drops: one drop per wavefront, user u on lane u % 64 (slot u / 64, UPL = 1, 2 or 4 slots per lane).  The AP table (x, y, row,
// column) is built once per workgroup in LDS and read wave-uniformly (every lane the same address: a broadcast).
//   active == 0: ONE pass over the APs.  A lane keeps (key, index, gain) of its best AP so far and the sum of all OTHER gains:
//                when a better AP appears the old best's gain moves into the sum (the interference is never formed as total minus
//                desired, which would lose it to cancellation next to an AP).
//   active == 1: pass 1 takes the best AP from the losses alone (no exponential), LDS atomics build the drop's 256-bit mask of
//                chosen APs and the users per AP; pass 2 walks the set bits of the mask wave-uniformly, one log2 and one exp2 per
//                (user, transmitting AP).
// A user's figures depend on its own position and on the drop's mask and loads alone, the per-drop sums are a lane-ordered slot
// sum followed by a fixed DPP tree (wave_lanes.hpp), and both histograms are exact integers: NO OUTPUT DEPENDS ON THE GRID, ON
// MCLE_OPT_GRID_OVERSUB OR ON HOW [first, first + count) IS SPLIT, bit for bit.  The histograms live in LDS per workgroup and are
// flushed once with 64-bit atomics that skip zeros (totals.hpp).
#include <cfloat>
#include <cmath>

#include "philox.hpp"
#include "pipe_common.hpp"
#include "wave_lanes.hpp"

namespace mcle {

constexpr int kIndoorMaxSide = 16, kIndoorMaxAps = 256, kIndoorMaxUsers = 256, kIndoorMaxBins = 256;
constexpr int kIndoorWaves = 4;          // wavefronts (drops in flight) per workgroup
// 10 log10(x) = kIndoorDbPerLog2 log2(x): the per-user epilogue then needs one logarithm's constants, not two (they live in SGPRs)
constexpr double kIndoorDbPerLog2 = 3.0102999566398119521;

struct IndoorParams {
    int n, dec, A, U, assoc, bins;
    double cx[kIndoorMaxSide], cy[kIndoorMaxSide];      // centre x of column c, centre y of row r (row 0 is the top one)
    double nL;                                          // n * side_length: the floor the users are dropped on
    double a_los, k_los, a_nlos, k_nlos, kx, wall2;     // log2-domain constants (see the head of the file)
    double tx, noise, hist_lo, hist_step;
};

template <typename T> struct IndoorConsts {
    T a_los, k_los, a_nlos, k_nlos, kx, wall2, tx, noise;
    __device__ explicit IndoorConsts(const IndoorParams& p)
        : a_los((T)p.a_los), k_los((T)p.k_los), a_nlos((T)p.a_nlos), k_nlos((T)p.k_nlos), kx((T)p.kx), wall2((T)p.wall2),
          tx((T)p.tx), noise((T)p.noise) {}
};

// v_log_f32 / v_exp_f32 in complex64's arithmetic (one unit in the last place each), the device libm in f64
__device__ __forceinline__ float indoor_log2(float x) { return __builtin_amdgcn_logf(x); }
__device__ __forceinline__ double indoor_log2(double x) { return log2(x); }
__device__ __forceinline__ float indoor_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ double indoor_exp2(double x) { return exp2(x); }

// total loss of one (point, AP) pair in the log2 domain from d^2 and the wall count
template <typename T, int MODEL>
__device__ __forceinline__ T indoor_loss2(const IndoorConsts<T>& k, T d2, int walls) {
    const T w = (T)walls;
    T pl = 0;
    if constexpr (MODEL == MCLE_INDOOR_PL_GENERAL) {
        pl = fma(k.a_los, indoor_log2(d2), k.k_los);
    } else if constexpr (MODEL == MCLE_INDOOR_PL_METIS_PS7) {
        const T l = indoor_log2(d2);
        pl = walls == 0 ? fma(k.a_los, l, k.k_los) : fma(k.a_nlos, l, fma(k.kx, w, k.k_nlos));
    }
    return fma(w, k.wall2, fmax(pl, (T)0));
}

struct IndoorLds {
    double apx[kIndoorMaxAps], apy[kIndoorMaxAps];
    double cx[kIndoorMaxSide], cy[kIndoorMaxSide];
    int aprc[kIndoorMaxAps];                             // row | column << 8
};

__device__ __forceinline__ bool indoor_is_ap(int r, int c, int dec) {
    return dec == 1 ? true : dec == 2 ? ((r + c) & 1) != 0 : dec == 4 ? ((r & 1) && (c & 1)) : (r % 3 == 1 && c % 3 == 1);
}

// The AP table, APs in row-major order of their rooms (room_positions[mask]); first wavefront of the workgroup, then a barrier
__device__ __forceinline__ void indoor_build_table(const IndoorParams& p, IndoorLds& s) {
    const int tid = threadIdx.x;
    if (tid < kIndoorMaxSide) {
        s.cx[tid] = tid < p.n ? p.cx[tid] : 0.0;
        s.cy[tid] = tid < p.n ? p.cy[tid] : 0.0;
    }
    __syncthreads();
    if (tid < 64) {
        int base = 0;
        for (int ch = 0; ch < (p.n * p.n + 63) / 64; ++ch) {
            const int t = ch * 64 + tid, r = t / p.n, c = t - r * p.n;
            const bool ap = t < p.n * p.n && indoor_is_ap(r, c, p.dec);
            const unsigned long long m = __ballot(ap);
            if (ap) {
                const int a = base + __popcll(m & ((1ull << tid) - 1ull));
                s.apx[a] = s.cx[c];
                s.apy[a] = s.cy[r];
                s.aprc[a] = r | (c << 8);
            }
            base += __popcll(m);
        }
    }
    __syncthreads();
}

// room of a point: nearest centre per axis, the lowest index on a tie (numpy.argmin over the rooms in row-major order)
__device__ __forceinline__ int indoor_room(const IndoorParams& p, const IndoorLds& s, double x, double y) {
    int row = 0, col = 0;
    double bx = fabs(x - s.cx[0]), by = fabs(y - s.cy[0]);
    for (int i = 1; i < p.n; ++i) {
        const double ex = fabs(x - s.cx[i]), ey = fabs(y - s.cy[i]);
        if (ex < bx) bx = ex, col = i;
        if (ey < by) by = ey, row = i;
    }
    return row | (col << 8);
}

template <typename T> struct IndoorUser {
    double x, y;
    int rc;          // room: row | column << 8
    T key, gbest, sum;
    int best;
};

template <typename T> __device__ __forceinline__ void indoor_user_reset(IndoorUser<T>& u) {
    u.key = (T)INFINITY;
    u.gbest = 0;
    u.sum = 0;
    u.best = 0;
}

// d^2 (T) and the wall count of (user, AP a)
template <typename T>
__device__ __forceinline__ T indoor_pair(const IndoorUser<T>& u, double ax, double ay, int arc, int& walls) {
    const T dx = (T)(u.x - ax), dy = (T)(u.y - ay);
    walls = abs((u.rc & 255) - (arc & 255)) + abs((u.rc >> 8) - (arc >> 8));
    return fma(dx, dx, dy * dy);
}

// one AP of the single pass: best so far with its gain, every other gain summed
template <typename T, int MODEL>
__device__ __forceinline__ void indoor_step_all(const IndoorConsts<T>& k, int assoc, IndoorUser<T>& u, int a, double ax, double ay,
                                                int arc) {
    int walls;
    const T d2 = indoor_pair(u, ax, ay, arc, walls);
    const T loss = indoor_loss2<T, MODEL>(k, d2, walls);
    const T g = indoor_exp2(-loss);
    const T key = assoc ? loss : d2;
    if (key < u.key) {
        u.sum += u.gbest;
        u.gbest = g;
        u.key = key;
        u.best = a;
    } else {
        u.sum += g;
    }
}

// SINR of a user from its best gain and the sum of the others: tx g* / (tx sum + noise), in T
template <typename T> __device__ __forceinline__ T indoor_sinr(const IndoorConsts<T>& k, const IndoorUser<T>& u) {
    return (k.tx * u.gbest) / fma(k.tx, u.sum, k.noise);
}

// ---- the heat-map operator: one point per thread ---------------------------------------------------------------------------
template <typename T, int MODEL>
__global__ __launch_bounds__(256) void k_indoor_sinr(IndoorParams p, const double* __restrict__ points, uint64_t n_points,
                                                     double* __restrict__ sinr_dB, int32_t* __restrict__ assoc_out) {
    __shared__ IndoorLds s;
    indoor_build_table(p, s);
    const IndoorConsts<T> k(p);
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_points; i += (uint64_t)gridDim.x * 256) {
        IndoorUser<T> u;
        u.x = points[2 * i];
        u.y = points[2 * i + 1];
        u.rc = indoor_room(p, s, u.x, u.y);
        indoor_user_reset(u);
        for (int a = 0; a < p.A; ++a) indoor_step_all<T, MODEL>(k, p.assoc, u, a, s.apx[a], s.apy[a], s.aprc[a]);
        if (sinr_dB) sinr_dB[i] = kIndoorDbPerLog2 * log2((double)indoor_sinr(k, u));
        if (assoc_out) assoc_out[i] = u.best;
    }
}

// ---- the drops: one drop per wavefront ---------------------------------------------------------------------------------------
struct IndoorDropOut {
    unsigned long long* hist;
    unsigned long long* load_hist;
    double* sum_capacity;
    double* sum_sinr_dB;
    double* min_sinr_dB;
    int32_t* active_aps;
    double* sinr_dB;
    double* capacity;
    int32_t* assoc;
};

struct IndoorDropTail {
    IndoorDropOut out;
    double hist_lo, hist_step, nL;
    int bins;
};

template <typename T, int MODEL, int ACTIVE, int UPL>
__global__ __launch_bounds__(64 * kIndoorWaves) void k_indoor_drops(IndoorParams p, uint64_t seed, uint64_t first, uint64_t count,
                                                                    const double* __restrict__ positions, IndoorDropOut out) {
    __shared__ IndoorLds s;
    __shared__ unsigned long long s_hist[kIndoorMaxBins + 2], s_load[kIndoorMaxUsers + 1];
    __shared__ unsigned s_cnt[kIndoorWaves][kIndoorMaxAps], s_mask[kIndoorWaves][kIndoorMaxAps / 32];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int i = tid; i < kIndoorMaxBins + 2; i += 64 * kIndoorWaves) s_hist[i] = 0ull;
    for (int i = tid; i < kIndoorMaxUsers + 1; i += 64 * kIndoorWaves) s_load[i] = 0ull;
    // the output pointers and the epilogue's scalars wait in LDS: as kernel arguments they stay in SGPRs over the whole drop
    // loop, next to the constants of the two passes, and the allocator parks dozens of them in VGPR lanes
    __shared__ IndoorDropTail s_tail;
    if (tid == 0) {
        s_tail.out = out;
        s_tail.hist_lo = p.hist_lo, s_tail.hist_step = p.hist_step, s_tail.nL = p.nL, s_tail.bins = p.bins;
    }
    const IndoorDropTail& tl = s_tail;
    indoor_build_table(p, s);                                // (ends with a barrier)
    const IndoorConsts<T> k(p);
    unsigned* cnt = s_cnt[wave];
    unsigned* mask = s_mask[wave];
    const int A = p.A, U = p.U;

    for (uint64_t d = (uint64_t)blockIdx.x * kIndoorWaves + wave; d < count; d += (uint64_t)gridDim.x * kIndoorWaves) {
        for (int i = lane; i < kIndoorMaxAps; i += 64) cnt[i] = 0u;
        if (lane < kIndoorMaxAps / 32) mask[lane] = 0u;
        IndoorUser<T> u[UPL];
        const Rng rng(seed, first + d);
#pragma unroll
        for (int j = 0; j < UPL; ++j) {
            const int uu = lane + 64 * j;
            u[j].x = 0.0, u[j].y = 0.0;
            if (uu < U) {
                if (positions) {
                    u[j].x = positions[(d * (uint64_t)U + uu) * 2];
                    u[j].y = positions[(d * (uint64_t)U + uu) * 2 + 1];
                } else {
                    // uniforms 2 u and 2 u + 1 of STREAM_CHAN: one Philox block per two users
                    const Words4 b = rng.block(STREAM_CHAN, (uint32_t)(uu >> 1));
                    const bool hi = (uu & 1) != 0;
                    u[j].x = tl.nL * ((double)(hi ? b.w[2] : b.w[0]) * 0x1p-32 - 0.5);
                    u[j].y = tl.nL * ((double)(hi ? b.w[3] : b.w[1]) * 0x1p-32 - 0.5);
                }
            }
            u[j].rc = indoor_room(p, s, u[j].x, u[j].y);
            indoor_user_reset(u[j]);
        }
        wave_lds_sync();                                     // the zeroed counts before the atomics below
        if constexpr (ACTIVE == 0) {
            for (int a = 0; a < A; ++a) {
                const double ax = s.apx[a], ay = s.apy[a];
                const int arc = s.aprc[a];
#pragma unroll
                for (int j = 0; j < UPL; ++j) indoor_step_all<T, MODEL>(k, p.assoc, u[j], a, ax, ay, arc);
            }
#pragma unroll
            for (int j = 0; j < UPL; ++j)
                if (lane + 64 * j < U) atomicAdd(&cnt[u[j].best], 1u);
        } else {
            // pass 1: the best AP from the losses alone
            for (int a = 0; a < A; ++a) {
                const double ax = s.apx[a], ay = s.apy[a];
                const int arc = s.aprc[a];
#pragma unroll
                for (int j = 0; j < UPL; ++j) {
                    int walls;
                    const T d2 = indoor_pair(u[j], ax, ay, arc, walls);
                    const T key = p.assoc ? indoor_loss2<T, MODEL>(k, d2, walls) : d2;
                    if (key < u[j].key) u[j].key = key, u[j].best = a;
                }
            }
#pragma unroll
            for (int j = 0; j < UPL; ++j)
                if (lane + 64 * j < U) {
                    atomicAdd(&cnt[u[j].best], 1u);
                    atomicOr(&mask[u[j].best >> 5], 1u << (u[j].best & 31));
                }
            wave_lds_sync();
            // pass 2: the transmitting APs only, taken wave-uniformly from the mask
            for (int wd = 0; wd < (A + 31) / 32; ++wd) {
                unsigned m = (unsigned)__builtin_amdgcn_readfirstlane((int)mask[wd]);
                while (m) {
                    const int a = 32 * wd + __ffs(m) - 1;
                    m &= m - 1u;
                    const double ax = s.apx[a], ay = s.apy[a];
                    const int arc = s.aprc[a];
#pragma unroll
                    for (int j = 0; j < UPL; ++j) {
                        int walls;
                        const T d2 = indoor_pair(u[j], ax, ay, arc, walls);
                        const T g = indoor_exp2(-indoor_loss2<T, MODEL>(k, d2, walls));
                        if (a == u[j].best)
                            u[j].gbest = g;
                        else
                            u[j].sum += g;
                    }
                }
            }
        }
        wave_lds_sync();                                     // every user's count is in
        // per user: SINR in dB, capacity shared among the users of its AP (f64 from the T SINR), the histogram slot
        double cap_sum = 0.0, db_sum = 0.0, db_min = INFINITY;
#pragma unroll
        for (int j = 0; j < UPL; ++j) {
            const int uu = lane + 64 * j;
            if (uu < U) {
                const double sinr = (double)indoor_sinr(k, u[j]);
                const double db = kIndoorDbPerLog2 * log2(sinr);
                const double cap = log2(1.0 + sinr) / (double)cnt[u[j].best];
                cap_sum += cap;
                db_sum += db;
                db_min = fmin(db_min, db);
                const uint64_t o = d * (uint64_t)U + uu;
                if (tl.out.sinr_dB) tl.out.sinr_dB[o] = db;
                if (tl.out.capacity) tl.out.capacity[o] = cap;
                if (tl.out.assoc) tl.out.assoc[o] = u[j].best;
                if (tl.out.hist) {
                    int slot = 0;
                    if (!(db < tl.hist_lo)) {
                        const double t = floor((db - tl.hist_lo) / tl.hist_step);
                        slot = (tl.bins == 0 || !(t < (double)tl.bins)) ? tl.bins + 1 : 1 + (int)t;
                    }
                    atomicAdd(&s_hist[slot], 1ull);
                }
            }
        }
        if (tl.out.load_hist)
            for (int a = lane; a < A; a += 64) atomicAdd(&s_load[cnt[a]], 1ull);
        int n_active = A;
        if constexpr (ACTIVE == 1) {
            n_active = 0;
            for (int wd = 0; wd < kIndoorMaxAps / 32; ++wd) n_active += __popc(mask[wd]);
        }
        cap_sum = wave_total_f64(cap_sum);
        db_sum = wave_total_f64(db_sum);
        db_min = wave_min_f64(db_min);
        if (lane == 0) {
            if (tl.out.sum_capacity) tl.out.sum_capacity[d] = cap_sum;
            if (tl.out.sum_sinr_dB) tl.out.sum_sinr_dB[d] = db_sum;
            if (tl.out.min_sinr_dB) tl.out.min_sinr_dB[d] = db_min;
            if (tl.out.active_aps) tl.out.active_aps[d] = n_active;
        }
        wave_lds_sync();                                     // cnt / mask are read before the next drop zeroes them
    }
    __syncthreads();
    // (a zero is not added: totals.hpp)
    if (tl.out.hist)
        for (int i = tid; i < tl.bins + 2; i += 64 * kIndoorWaves)
            if (s_hist[i]) atomicAdd(&tl.out.hist[i], s_hist[i]);
    if (tl.out.load_hist)
        for (int i = tid; i < U + 1; i += 64 * kIndoorWaves)
            if (s_load[i]) atomicAdd(&tl.out.load_hist[i], s_load[i]);
}

// ---- host side -------------------------------------------------------------------------------------------------------------
static int indoor_count_aps(int n, int dec) {
    int A = 0;
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c)
            A += dec == 1 ? 1 : dec == 2 ? ((r + c) & 1) : dec == 4 ? ((r & 1) && (c & 1)) : (r % 3 == 1 && c % 3 == 1);
    return A;
}

// The argument rules both entry points share (before the context and the pointers) and the kernel's parameter block
static int indoor_check(int dtype, const mcle_indoor_cfg* cfg, bool drops, IndoorParams& p) {
    MCLE_REQUIRE(dtype == MCLE_F32 || dtype == MCLE_F64, "dtype must be MCLE_F32 or MCLE_F64");
    MCLE_REQUIRE(cfg != nullptr, "null indoor cfg");
    MCLE_REQUIRE(cfg->rooms_per_side >= 1 && cfg->rooms_per_side <= kIndoorMaxSide, "rooms_per_side must be in [1, %d] (got %d)",
                 kIndoorMaxSide, cfg->rooms_per_side);
    MCLE_REQUIRE(cfg->ap_decimation == 1 || cfg->ap_decimation == 2 || cfg->ap_decimation == 4 || cfg->ap_decimation == 9,
                 "ap_decimation must be 1, 2, 4 or 9 (got %d)", cfg->ap_decimation);
    const int n = cfg->rooms_per_side, A = indoor_count_aps(n, cfg->ap_decimation);
    MCLE_REQUIRE(A >= 1, "ap_decimation %d leaves %d rooms per side without an access point", cfg->ap_decimation, n);
    MCLE_REQUIRE(cfg->model >= MCLE_INDOOR_PL_NONE && cfg->model <= MCLE_INDOOR_PL_METIS_PS7,
                 "model must be 0 (none), 1 (general) or 2 (METIS PS7) (got %d)", cfg->model);
    MCLE_REQUIRE(cfg->assoc == 0 || cfg->assoc == 1, "assoc must be 0 (closest) or 1 (best channel) (got %d)", cfg->assoc);
    if (drops) {
        MCLE_REQUIRE(cfg->active == 0 || cfg->active == 1, "active must be 0 (every AP) or 1 (chosen APs) (got %d)", cfg->active);
        MCLE_REQUIRE(cfg->n_users >= 1 && cfg->n_users <= kIndoorMaxUsers, "n_users must be in [1, %d] (got %d)",
                     kIndoorMaxUsers, cfg->n_users);
        MCLE_REQUIRE(cfg->hist_bins >= 0 && cfg->hist_bins <= kIndoorMaxBins, "hist_bins must be in [0, %d] (got %d)",
                     kIndoorMaxBins, cfg->hist_bins);
        if (cfg->hist_bins > 0)
            MCLE_REQUIRE(std::isfinite(cfg->hist_lo_dB) && std::isfinite(cfg->hist_step_dB) && cfg->hist_step_dB > 0.0,
                         "hist_lo_dB must be finite and hist_step_dB positive");
        else
            MCLE_REQUIRE(std::isfinite(cfg->hist_lo_dB), "hist_lo_dB must be finite");
    } else {
        MCLE_REQUIRE(cfg->active == 0, "active must be 0 for the heat-map operator (got %d)", cfg->active);
    }
    MCLE_REQUIRE(std::isfinite(cfg->side_length) && cfg->side_length > 0.0, "side_length must be positive");
    MCLE_REQUIRE(std::isfinite(cfg->wall_loss_dB) && cfg->wall_loss_dB >= 0.0, "wall_loss_dB must be non-negative");
    if (cfg->model == MCLE_INDOOR_PL_GENERAL) {
        MCLE_REQUIRE(std::isfinite(cfg->pl_n) && cfg->pl_n > 0.0, "pl_n must be positive");
        MCLE_REQUIRE(std::isfinite(cfg->pl_C), "pl_C must be finite");
        MCLE_REQUIRE(std::isfinite(cfg->dist_scale) && cfg->dist_scale > 0.0, "dist_scale must be positive");
    }
    if (cfg->model == MCLE_INDOOR_PL_METIS_PS7)
        MCLE_REQUIRE(std::isfinite(cfg->fc_MHz) && cfg->fc_MHz > 0.0, "fc_MHz must be positive");
    MCLE_REQUIRE(std::isfinite(cfg->tx_power) && cfg->tx_power > 0.0, "tx_power must be positive");
    MCLE_REQUIRE(std::isfinite(cfg->noise_power) && cfg->noise_power > 0.0, "noise_power must be positive");
    if (dtype == MCLE_F32) {
        // both are rounded to f32: a power that is no normal f32 number would make the SINR of a lone AP inf or NaN
        MCLE_REQUIRE(cfg->tx_power >= (double)FLT_MIN && cfg->tx_power <= (double)FLT_MAX,
                     "tx_power must be a normal f32 number (1.18e-38 .. 3.4e38) in f32 arithmetic (got %g)", cfg->tx_power);
        MCLE_REQUIRE(cfg->noise_power >= (double)FLT_MIN && cfg->noise_power <= (double)FLT_MAX,
                     "noise_power must be a normal f32 number (1.18e-38 .. 3.4e38) in f32 arithmetic (got %g)", cfg->noise_power);
    }

    std::memset(&p, 0, sizeof(p));
    p.n = n, p.dec = cfg->ap_decimation, p.A = A, p.U = drops ? cfg->n_users : 0, p.assoc = cfg->assoc;
    p.bins = drops ? cfg->hist_bins : 0;
    // room centres as calc_room_positions_square forms them, the floor division of the shift included (volatile: no contraction)
    const double L = cfg->side_length;
    const double shift = std::floor(L * (double)(n - 1) / 2.0);
    for (int i = 0; i < n; ++i) {
        volatile double tx = L * ((double)i - 0.5), ty = L * ((double)(n - 1 - i) - 0.5);
        volatile double sx = tx - shift, sy = ty - shift;
        p.cx[i] = sx + L / 2.0;
        p.cy[i] = sy + L / 2.0;
    }
    p.nL = (double)n * L;
    // walls: the reference's round(|Re| + |Im|) of (room - 1.0001 ap) / side_length must be the Manhattan distance of the room
    // indices.  Shown per axis: each part within a quarter of its index distance, so the sum rounds to the Manhattan distance.
    for (int i = 0; i < n; ++i)
        for (int ia = 0; ia < n; ++ia) {
            const double re = std::fabs((p.cx[i] - 1.0001 * p.cx[ia]) / L), im = std::fabs((p.cy[i] - 1.0001 * p.cy[ia]) / L);
            const double want = (double)std::abs(i - ia);
            MCLE_REQUIRE(std::fabs(re - want) < 0.25 && std::fabs(im - want) < 0.25,
                         "rooms_per_side %d with side_length %g: the reference's wall count is not the Manhattan distance of the "
                         "room indices", n, L);
        }
    const double c2 = std::log2(10.0) / 10.0;
    if (cfg->model == MCLE_INDOOR_PL_GENERAL) {
        p.a_los = p.a_nlos = cfg->pl_n / 2.0;
        p.k_los = p.k_nlos = (10.0 * cfg->pl_n * std::log10(cfg->dist_scale) + cfg->pl_C) * c2;
    } else if (cfg->model == MCLE_INDOOR_PL_METIS_PS7) {
        const double F = 20.0 * std::log10(cfg->fc_MHz / 1e3 / 5.0);
        p.a_los = 18.7 / 20.0, p.k_los = (46.8 + F) * c2;
        p.a_nlos = 36.8 / 20.0, p.k_nlos = (43.8 + F - 5.0) * c2, p.kx = 5.0 * c2;
    }
    p.wall2 = cfg->wall_loss_dB * c2;
    p.tx = cfg->tx_power, p.noise = cfg->noise_power;
    p.hist_lo = cfg->hist_lo_dB, p.hist_step = p.bins > 0 ? cfg->hist_step_dB : 1.0;
    return MCLE_OK;
}

template <typename T, int MODEL>
static int launch_indoor_sinr(mcle_ctx* ctx, const IndoorParams& p, const double* d_points, size_t n, double* d_sinr_dB,
                              int32_t* d_assoc) {
    const unsigned grid = (unsigned)grid_for(ctx, n, 256, 8);
    hipLaunchKernelGGL((k_indoor_sinr<T, MODEL>), dim3(grid), dim3(256), 0, ctx->stream, p, d_points, (uint64_t)n, d_sinr_dB,
                       d_assoc);
    MCLE_LAUNCH_CHECK();
    return MCLE_OK;
}

template <typename T, int MODEL, int ACTIVE>
static int launch_indoor_drops(mcle_ctx* ctx, const IndoorParams& p, uint64_t seed, uint64_t first, uint64_t count,
                               const double* d_positions, const IndoorDropOut& out, int& upl) {
    const uint64_t groups = (count + kIndoorWaves - 1) / kIndoorWaves;
    const unsigned grid = (unsigned)oversubscribed_grid(ctx, (uint64_t)(ctx->n_cu > 0 ? ctx->n_cu : 256) * 8, groups, 2);
    upl = p.U <= 64 ? 1 : p.U <= 128 ? 2 : 4;
#define MCLE_INDOOR_GO(UPL_)                                                                                                    \
    hipLaunchKernelGGL((k_indoor_drops<T, MODEL, ACTIVE, UPL_>), dim3(grid), dim3(64 * kIndoorWaves), 0, ctx->stream, p, seed,  \
                       first, count, d_positions, out)
    if (upl == 1)
        MCLE_INDOOR_GO(1);
    else if (upl == 2)
        MCLE_INDOOR_GO(2);
    else
        MCLE_INDOOR_GO(4);
#undef MCLE_INDOOR_GO
    MCLE_LAUNCH_CHECK();
    return MCLE_OK;
}

}  // namespace mcle

using namespace mcle;

extern "C" {

int mcle_indoor_sinr(mcle_ctx* ctx, int dtype, const mcle_indoor_cfg* cfg, const double* d_points, size_t n, double* d_sinr_dB,
                     int32_t* d_assoc) {
    if (ctx) ctx->last_kernel[0] = 0;
    IndoorParams p;
    int rc;
    if ((rc = indoor_check(dtype, cfg, false, p))) return rc;
    MCLE_REQUIRE((uint64_t)n <= 0x7fffffffull, "n must be at most 2^31-1");
    MCLE_REQUIRE(ctx != nullptr, "null context");
    if (n == 0) return MCLE_OK;
    MCLE_REQUIRE(d_points != nullptr, "null d_points");
    if ((rc = ctx->bind())) return rc;
#define MCLE_INDOOR_OP(T_, M_) rc = launch_indoor_sinr<T_, M_>(ctx, p, d_points, n, d_sinr_dB, d_assoc)
    switch (cfg->model * 2 + (dtype == MCLE_F64)) {
        case 0: MCLE_INDOOR_OP(float, MCLE_INDOOR_PL_NONE); break;
        case 1: MCLE_INDOOR_OP(double, MCLE_INDOOR_PL_NONE); break;
        case 2: MCLE_INDOOR_OP(float, MCLE_INDOOR_PL_GENERAL); break;
        case 3: MCLE_INDOOR_OP(double, MCLE_INDOOR_PL_GENERAL); break;
        case 4: MCLE_INDOOR_OP(float, MCLE_INDOOR_PL_METIS_PS7); break;
        default: MCLE_INDOOR_OP(double, MCLE_INDOOR_PL_METIS_PS7); break;
    }
#undef MCLE_INDOOR_OP
    if (rc) return rc;
    ctx->set_kernel("indoor_sinr %s m%d a%d", dtype == MCLE_F64 ? "f64" : "f32", cfg->model, cfg->assoc);
    return MCLE_OK;
}

int mcle_run_indoor_drops(mcle_ctx* ctx, int dtype, const mcle_indoor_cfg* cfg, uint64_t seed, uint64_t first, uint64_t count,
                          const double* d_positions, uint64_t* d_hist, uint64_t* d_load_hist, double* d_sum_capacity,
                          double* d_sum_sinr_dB, double* d_min_sinr_dB, int32_t* d_active_aps, double* d_sinr_dB,
                          double* d_capacity, int32_t* d_assoc) {
    if (ctx) ctx->last_kernel[0] = 0;
    IndoorParams p;
    int rc;
    if ((rc = indoor_check(dtype, cfg, true, p))) return rc;
    MCLE_REQUIRE(count <= 0x7fffffffull, "count must be at most 2^31-1 drops per call");
    MCLE_REQUIRE(ctx != nullptr, "null context");
    if (count == 0) return MCLE_OK;
    if ((rc = ctx->bind())) return rc;
    IndoorDropOut out;
    out.hist = (unsigned long long*)d_hist, out.load_hist = (unsigned long long*)d_load_hist;
    out.sum_capacity = d_sum_capacity, out.sum_sinr_dB = d_sum_sinr_dB, out.min_sinr_dB = d_min_sinr_dB;
    out.active_aps = d_active_aps, out.sinr_dB = d_sinr_dB, out.capacity = d_capacity, out.assoc = d_assoc;
    int upl = 0;
#define MCLE_INDOOR_RUN(T_, M_)                                                                                     \
    rc = cfg->active ? launch_indoor_drops<T_, M_, 1>(ctx, p, seed, first, count, d_positions, out, upl)            \
                     : launch_indoor_drops<T_, M_, 0>(ctx, p, seed, first, count, d_positions, out, upl)
    switch (cfg->model * 2 + (dtype == MCLE_F64)) {
        case 0: MCLE_INDOOR_RUN(float, MCLE_INDOOR_PL_NONE); break;
        case 1: MCLE_INDOOR_RUN(double, MCLE_INDOOR_PL_NONE); break;
        case 2: MCLE_INDOOR_RUN(float, MCLE_INDOOR_PL_GENERAL); break;
        case 3: MCLE_INDOOR_RUN(double, MCLE_INDOOR_PL_GENERAL); break;
        case 4: MCLE_INDOOR_RUN(float, MCLE_INDOOR_PL_METIS_PS7); break;
        default: MCLE_INDOOR_RUN(double, MCLE_INDOOR_PL_METIS_PS7); break;
    }
#undef MCLE_INDOOR_RUN
    if (rc) return rc;
    ctx->set_kernel("indoor_drops %s m%d a%d t%d u%d", dtype == MCLE_F64 ? "f64" : "f32", cfg->model, cfg->assoc, cfg->active, upl);
    return MCLE_OK;
}

}  // extern "C"
