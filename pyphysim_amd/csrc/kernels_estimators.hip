// kernels_estimators.hip -- the LS and MMSE block-pilot channel estimators (reference: channel_estimation/estimators.py:12-61
// compute_ls_estimation, :100-174 compute_mmse_estimation; Fodor et al. 2014) and the fused estimation-error pipeline built on
// them (the Monte-Carlo loop of the reference's tests/channel_estimation_package_test.py:246-325).
//
// Model: Y = h s + N, Y [nr][P], s [nt][P], h [nr][nt] with covariance C across the receive antennas.
//     LS:    h^ = Y s^H (s s^H)^-1                      a row of Y (one realization, one antenna) at a time
//     MMSE:  h^ = A (Y s^H) P / |s|^2,  A = (noise_power I + P C)^-1 C,  nt = 1
// A is one nr x nr matrix shared by every realization (computed once per call, in f64, on the host): applying it to a batch of
// matched-filter outputs is a complex GEMM whose N dimension is the realization index.  It runs on v_mfma_f64_16x16x4_f64 /
// v_mfma_f32_16x16x4_f32 as four real products per 16 x 16 x 4 step over a tile of 16 realizations per wavefront:
//     Re D += Re A Re Z - Im A Im Z,   Im D += Re A Im Z + Im A Re Z.
// The antenna tail is zero-padded to a multiple of 16, the realization tail masked.  The matrix is read from global memory
// (transposed, so that the 16 lanes of a k share 16 consecutive elements): every workgroup reads the same nr x nr values, which
// stay in L2 -- at nr = 128 in complex128 they are 256 KiB and would not fit the LDS.  The channel colouring h = alpha L w of the
// pipeline is the same product with L in A's place.
//
// A column of the product depends on that column of Z alone and every per-realization sum is taken in an order fixed by the
// shape, so no output depends on where in a tile, a grid or a split of the batch its realization falls.
#include <cmath>
#include <complex>
#include <mutex>

#include "cazac_common.hpp"

namespace mcle {

constexpr int kEstMaxNr = 128;
constexpr int kEstMaxNt = 8;
constexpr int kEstMaxPilots = 1024;
constexpr int kPilotMseMaxPilots = 256;
constexpr int kLsTile = 32;                      // realizations per workgroup trip of k_ls_estimate
constexpr size_t kEstLdsBudget = (size_t)160 * 1024;

typedef float est_f32x4 __attribute__((ext_vector_type(4)));
typedef double est_f64x4 __attribute__((ext_vector_type(4)));

// the 16 x 16 x 4 matrix-core step in either arithmetic: lane l supplies A[l & 15][l >> 4] and B[l >> 4][l & 15]; result i of
// lane l is D[row(l, i)][l & 15] -- the two arithmetics number the rows differently
template <typename T> struct Tile16;
template <> struct Tile16<float> {
    using acc = est_f32x4;
    static __device__ __forceinline__ acc mma(float a, float b, acc c) {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ int row(int lane, int i) { return (lane >> 4) * 4 + i; }
};
template <> struct Tile16<double> {
    using acc = est_f64x4;
    static __device__ __forceinline__ acc mma(double a, double b, acc c) {
        return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ int row(int lane, int i) { return (lane >> 4) + 4 * i; }
};

// D[16 m + row][col] = sum_k M[16 m + row][k] B[k][col], k < nrp.  Mt: the matrix TRANSPOSED in global memory, Mt[k][row],
// [nrp][nrp], zero beyond nr; B: planes bre, bim [nrp][16] in the wavefront's LDS.
template <typename T>
__device__ __forceinline__ void tile_apply(const cx<T>* __restrict__ Mt, const T* bre, const T* bim, int nrp, int m, int lane,
                                           typename Tile16<T>::acc& dr, typename Tile16<T>::acc& di) {
    const int col = lane & 15, kq = lane >> 4;
    dr = (typename Tile16<T>::acc){0, 0, 0, 0};
    di = dr;
    // sixteen k at a time (nrp is a multiple of 16): the four matrix reads of a trip are in flight together -- one read per
    // step left the product waiting for L2 once per four k
    for (int k0 = 0; k0 < nrp; k0 += 16) {
        cx<T> a[4];
        T br[4], bi[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + 4 * j + kq;
            a[j] = Mt[(size_t)k * nrp + 16 * m + col];
            br[j] = bre[k * 16 + col];
            bi[j] = bim[k * 16 + col];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            dr = Tile16<T>::mma(a[j].x, br[j], dr);
            dr = Tile16<T>::mma(-a[j].y, bi[j], dr);
            di = Tile16<T>::mma(a[j].x, bi[j], di);
            di = Tile16<T>::mma(a[j].y, br[j], di);
        }
    }
}

// (s s^H)[t][u] = sum_p s[t][p] conj(s[u][p]), accumulated in f64 whatever the arithmetic of s
template <typename T> __device__ __forceinline__ double2 gram_entry(const cx<T>* s, int P, int t, int u) {
    double2 acc = make_double2(0.0, 0.0);
    const cx<T>* st = s + (size_t)t * P;
    const cx<T>* su = s + (size_t)u * P;
    for (int p = 0; p < P; ++p) {
        const double2 a = make_double2((double)st[p].x, (double)st[p].y);
        const double2 b = make_double2((double)su[p].x, (double)su[p].y);
        acc = cfmac4(a, b, acc);
    }
    return acc;
}

// g [nt][nt] in LDS, owned by the calling lane: inverted in place by Gauss-Jordan without pivoting -- the Gram matrix is
// Hermitian positive definite when the pilots have full row rank.  A singular one leaves inf / nan behind, never a fault.
__device__ __forceinline__ void invert_in_place(double2* g, int nt) {
    for (int k = 0; k < nt; ++k) {
        const double2 piv = g[k * nt + k];
        const double d = piv.x * piv.x + piv.y * piv.y;
        const double2 inv = make_double2(piv.x / d, -piv.y / d);
        g[k * nt + k] = make_double2(1.0, 0.0);
        for (int j = 0; j < nt; ++j) g[k * nt + j] = cmul(g[k * nt + j], inv);
        for (int i = 0; i < nt; ++i) {
            if (i == k) continue;
            const double2 f = g[i * nt + k];
            g[i * nt + k] = make_double2(0.0, 0.0);
            for (int j = 0; j < nt; ++j) g[i * nt + j] = cfma4(make_double2(-f.x, -f.y), g[k * nt + j], g[i * nt + j]);
        }
    }
}

template <typename T> __device__ __forceinline__ cx<T> from_f64(double2 v) { return mk<T>((T)v.x, (T)v.y); }

// h^[u] = sum_t z[t] ginv[t][u] for the nt entries of one row; NTP = nt rounded up to a power of two
template <typename T, int NTP>
__device__ __forceinline__ void ls_row(const cx<T> (&z)[NTP], const double2* ginv, int nt, cx<T> (&est)[NTP]) {
#pragma unroll
    for (int u = 0; u < NTP; ++u) {
        cx<T> acc = mk<T>(0, 0);
#pragma unroll
        for (int t = 0; t < NTP; ++t)
            if (t < nt && u < nt) acc = cfma4(z[t], from_f64<T>(ginv[t * nt + u]), acc);
        est[u] = acc;
    }
}

// ---- LS operator -----------------------------------------------------------------------------------------------------------
// Y [batch][nr][P]; s [nt][P] or [batch][nt][P]; out [batch][nr][nt].  A workgroup takes kLsTile realizations per trip: their
// inverse Gram matrices go to LDS (one lane each; shared pilots: once per workgroup), then a lane per row of Y.
template <typename T, int NTP>
__global__ __launch_bounds__(256) void k_ls_estimate(const cx<T>* __restrict__ Y, const cx<T>* __restrict__ s, int nr, int nt,
                                                     int P, int per_real, size_t batch, cx<T>* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double2* g_all = reinterpret_cast<double2*>(smem);
    const int gsz = nt * nt;
    if (!per_real) {
        if ((int)threadIdx.x < gsz) g_all[threadIdx.x] = gram_entry<T>(s, P, (int)threadIdx.x / nt, (int)threadIdx.x % nt);
        __syncthreads();
        if (threadIdx.x == 0) invert_in_place(g_all, nt);
        __syncthreads();
    }
    const size_t tiles = (batch + kLsTile - 1) / kLsTile;
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const size_t b0 = tile * kLsTile;
        const int nb = (int)(batch - b0 < (size_t)kLsTile ? batch - b0 : (size_t)kLsTile);
        if (per_real) {
            __syncthreads();                         // the previous trip's readers
            if ((int)threadIdx.x < nb) {
                double2* g = g_all + (size_t)threadIdx.x * gsz;
                const cx<T>* sb = s + (b0 + threadIdx.x) * (size_t)nt * P;
                for (int e = 0; e < gsz; ++e) g[e] = gram_entry<T>(sb, P, e / nt, e % nt);
                invert_in_place(g, nt);
            }
            __syncthreads();
        }
        for (int rho = threadIdx.x; rho < nb * nr; rho += blockDim.x) {
            const int bl = rho / nr;
            const size_t row = b0 * nr + rho;
            const cx<T>* y = Y + row * (size_t)P;
            const cx<T>* sb = per_real ? s + (b0 + bl) * (size_t)nt * P : s;
            const double2* g = per_real ? g_all + (size_t)bl * gsz : g_all;
            cx<T> z[NTP], est[NTP];
#pragma unroll
            for (int t = 0; t < NTP; ++t) z[t] = mk<T>(0, 0);
            for (int p = 0; p < P; ++p) {
                const cx<T> v = y[p];
#pragma unroll
                for (int t = 0; t < NTP; ++t)
                    if (t < nt) z[t] = cfmac4(v, sb[(size_t)t * P + p], z[t]);
            }
            ls_row<T, NTP>(z, g, nt, est);
#pragma unroll
            for (int u = 0; u < NTP; ++u)
                if (u < nt) out[row * nt + u] = est[u];
        }
    }
}

// ---- MMSE operator ---------------------------------------------------------------------------------------------------------
// Y [batch][nr][P]; s [P] or [batch][P]; At: A transposed and padded, [nrp][nrp]; out [batch][nr].  One wavefront per workgroup
// and per tile of 16 realizations: lane (q, b) forms z[a][b] = (Y[b][a] . conj(s)) P / |s|^2 for a = q, q + 4, ... into the
// planes of the wavefront's LDS, then A is applied 16 rows at a time.
template <typename T>
__global__ __launch_bounds__(64) void k_mmse_estimate(const cx<T>* __restrict__ Y, const cx<T>* __restrict__ s, int nr, int nrp,
                                                      int P, int per_real, size_t batch, const cx<T>* __restrict__ At,
                                                      cx<T>* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* zre = reinterpret_cast<T*>(smem);
    T* zim = zre + nrp * 16;
    const int lane = threadIdx.x, bl = lane & 15, q = lane >> 4;
    const size_t tiles = (batch + 15) / 16;
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const size_t b = tile * 16 + bl;
        const bool valid = b < batch;
        const cx<T>* sb = (per_real && valid) ? s + b * (size_t)P : s;
        T scale = 0;
        if (valid) {
            double n2 = 0.0;
            for (int p = 0; p < P; ++p) n2 += (double)sb[p].x * (double)sb[p].x + (double)sb[p].y * (double)sb[p].y;
            scale = (T)((double)P / n2);
        }
        for (int a = q; a < nrp; a += 4) {
            cx<T> z = mk<T>(0, 0);
            if (valid && a < nr) {
                const cx<T>* y = Y + (b * nr + a) * (size_t)P;
#pragma unroll 4
                for (int p = 0; p < P; ++p) z = cfmac4(y[p], sb[p], z);
                z = cscale(z, scale);
            }
            zre[a * 16 + bl] = z.x;
            zim[a * 16 + bl] = z.y;
        }
        wave_lds_sync();
        for (int m = 0; m < (nrp >> 4); ++m) {
            typename Tile16<T>::acc dr, di;
            tile_apply<T>(At, zre, zim, nrp, m, lane, dr, di);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = 16 * m + Tile16<T>::row(lane, i);
                if (valid && row < nr) out[b * nr + row] = mk<T>(dr[i], di[i]);
            }
        }
        wave_lds_sync();
    }
}

// ---- fused estimation-error pipeline ---------------------------------------------------------------------------------------
// One wavefront per workgroup and per tile of NB = 16 / NTP realizations (NTP = nt rounded up to a power of two): column
// c = NTP b + t of the 16-column planes is transmit antenna t of the tile's realization b.  Draws (mcle-philox-v1, DESIGN
// section 4): pilot phase of (t, p) = uniform t P + p of STREAM_PHASE; w[a][t] = CN sample t nr + a of STREAM_CHAN; noise of
// (antenna a, pilot p) = CN sample 2 ceil(P / 2) a + p of STREAM_NOISE (a Philox block = pilots 2 j and 2 j + 1 of one antenna).
// Lane (q, b) owns the rows a = q, q + 64 / NB, ... of realization b: y = h[a] s[:, p] + n is formed and matched-filtered in
// registers (Y never exists in memory), its LS estimate taken as k_ls_estimate does, its squared error added in that order; the
// 64 / NB partial sums of a realization meet in a fixed tree.  With a covariance (nt = 1) the scaled matched filter goes to the
// planes the draw w has left, A is applied as k_mmse_estimate does, and the error is summed against h in the product's own lanes.
struct PilotMseParams {
    int nr, nrp, nt, P, half;                    // half = ceil(P / 2)
    int random_pilots, has_L, has_mmse;
    double amp, sigma, alpha;                    // sqrt(pilot_power), sqrt(noise_power)
};

template <int NTP> constexpr int pilot_mse_nb() { return 16 / NTP; }

// LDS of one wavefront: the inverse Gram matrices, the planes w / z and h, the pilots
inline size_t pilot_mse_lds(const PilotMseParams& p, int ntp, size_t real_bytes) {
    const size_t nb = 16 / ntp, ng = p.random_pilots ? nb : 1;
    return ng * p.nt * p.nt * sizeof(double2) + 2 * (2 * (size_t)p.nrp * 16 * real_bytes) +
           ng * (size_t)p.nt * p.P * 2 * real_bytes;
}

template <typename T, int NTP>
__global__ __launch_bounds__(64) void k_pilot_mse(PilotMseParams p, const cx<T>* __restrict__ pilots,
                                                  const cx<T>* __restrict__ Lt, const cx<T>* __restrict__ At, uint64_t seed,
                                                  uint64_t first, uint64_t count, double* __restrict__ err_ls,
                                                  double* __restrict__ err_mmse, double* __restrict__ pow) {
    constexpr int NB = 16 / NTP, Q = 64 / NB;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int nt = p.nt, nr = p.nr, nrp = p.nrp, P = p.P, gsz = nt * nt, per = nt * P;
    const int ng = p.random_pilots ? NB : 1;
    double2* G = reinterpret_cast<double2*>(smem);
    T* wre = reinterpret_cast<T*>(G + ng * gsz);
    T* wim = wre + nrp * 16;
    T* hre = wim + nrp * 16;
    T* him = hre + nrp * 16;
    cx<T>* S = reinterpret_cast<cx<T>*>(him + nrp * 16);
    const int lane = threadIdx.x, bl = lane % NB, q = lane / NB;
    if (!p.random_pilots) {
        for (int i = lane; i < per; i += 64) S[i] = pilots[i];
        wave_lds_sync();
        if (lane < gsz) G[lane] = gram_entry<T>(S, P, lane / nt, lane % nt);
        wave_lds_sync();
        if (lane == 0) invert_in_place(G, nt);
        wave_lds_sync();
    }
    const uint64_t tiles = (count + NB - 1) / NB;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t r0 = tile * NB, r = r0 + bl;
        const bool valid = r < count;
        const Rng rng(seed, first + r);
        if (p.random_pilots) {
            for (int i = lane; i < NB * per; i += 64) {
                const int b2 = i / per, pos = i - b2 * per;
                cx<T> v = mk<T>(0, 0);
                if (r0 + b2 < count) {
                    const double u = uniform_at(Rng(seed, first + r0 + b2), STREAM_PHASE, (uint64_t)pos);
                    double sn, cs;
                    sincospi(2.0 * u, &sn, &cs);
                    v = mk<T>((T)(p.amp * cs), (T)(p.amp * sn));
                }
                S[i] = v;
            }
            wave_lds_sync();
            if (q == 0 && valid) {
                double2* g = G + bl * gsz;
                for (int e = 0; e < gsz; ++e) g[e] = gram_entry<T>(S + bl * per, P, e / nt, e % nt);
                invert_in_place(g, nt);
            }
            wave_lds_sync();
        }
        // ---- w, and h = alpha L w
        {
            T* dre = p.has_L ? wre : hre;
            T* dim = p.has_L ? wim : him;
            const T alpha = p.has_L ? (T)1 : (T)p.alpha;          // (alpha is folded into Lt)
            for (int i = lane; i < nrp * 16; i += 64) {
                const int a = i >> 4, c = i & 15, b2 = c / NTP, t = c % NTP;
                cx<T> w = mk<T>(0, 0);
                if (a < nr && t < nt && r0 + b2 < count)
                    w = cn_sample<T>(Rng(seed, first + r0 + b2), STREAM_CHAN, (uint64_t)(t * nr + a), (T)1);
                dre[i] = alpha * w.x;
                dim[i] = alpha * w.y;
            }
            wave_lds_sync();
            if (p.has_L) {
                for (int m = 0; m < (nrp >> 4); ++m) {
                    typename Tile16<T>::acc dr, di;
                    tile_apply<T>(Lt, wre, wim, nrp, m, lane, dr, di);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int row = 16 * m + Tile16<T>::row(lane, i);
                        hre[row * 16 + (lane & 15)] = dr[i];
                        him[row * 16 + (lane & 15)] = di[i];
                    }
                }
                wave_lds_sync();
            }
        }
        // ---- the rows of this lane's realization
        const cx<T>* sb = S + (p.random_pilots ? bl * per : 0);
        const double2* g = G + (p.random_pilots ? bl * gsz : 0);
        double e_ls = 0.0, pw = 0.0;
        const int a_end = (NTP == 1 && p.has_mmse) ? nrp : nr;
        for (int a = q; a < a_end; a += Q) {
            cx<T> zs = mk<T>(0, 0);
            if (valid && a < nr) {
                cx<T> h[NTP], z[NTP], est[NTP];
#pragma unroll
                for (int t = 0; t < NTP; ++t) {
                    z[t] = mk<T>(0, 0);
                    h[t] = mk<T>(hre[a * 16 + bl * NTP + t], him[a * 16 + bl * NTP + t]);     // (zero for t >= nt)
                }
                for (int j = 0; j < p.half; ++j) {
                    cx<T> n[2];
                    n[0] = n[1] = mk<T>(0, 0);
                    if (p.sigma != 0.0) cn_pair<T>(rng, STREAM_NOISE, (uint32_t)(a * p.half + j), (T)p.sigma, n[0], n[1]);
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const int pp = 2 * j + e;
                        if (pp >= P) break;
                        cx<T> y = n[e];
#pragma unroll
                        for (int t = 0; t < NTP; ++t)
                            if (t < nt) y = cfma4(h[t], sb[t * P + pp], y);
#pragma unroll
                        for (int t = 0; t < NTP; ++t)
                            if (t < nt) z[t] = cfmac4(y, sb[t * P + pp], z[t]);
                    }
                }
                ls_row<T, NTP>(z, g, nt, est);
#pragma unroll
                for (int t = 0; t < NTP; ++t)
                    if (t < nt) {
                        const cx<T> d = csub(est[t], h[t]);
                        e_ls += (double)(d.x * d.x + d.y * d.y);
                        pw += (double)(h[t].x * h[t].x + h[t].y * h[t].y);
                    }
                if constexpr (NTP == 1) zs = cscale(z[0], (T)((double)P * g[0].x));      // g[0] = 1 / |s|^2
            }
            if constexpr (NTP == 1)
                if (p.has_mmse) {
                    wre[a * 16 + bl] = zs.x;
                    wim[a * 16 + bl] = zs.y;
                }
        }
#pragma unroll
        for (int off = NB; off < 64; off <<= 1) {
            e_ls += __shfl_xor(e_ls, off, 64);
            pw += __shfl_xor(pw, off, 64);
        }
        if (q == 0 && valid) {
            err_ls[r] = e_ls;
            pow[r] = pw;
        }
        if constexpr (NTP == 1)
            if (p.has_mmse) {
                wave_lds_sync();
                double e_mm = 0.0;
                for (int m = 0; m < (nrp >> 4); ++m) {
                    typename Tile16<T>::acc dr, di;
                    tile_apply<T>(At, wre, wim, nrp, m, lane, dr, di);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int row = 16 * m + Tile16<T>::row(lane, i);          // (rows >= nr: 0 - 0)
                        const T dx = dr[i] - hre[row * 16 + (lane & 15)], dy = di[i] - him[row * 16 + (lane & 15)];
                        e_mm += (double)(dx * dx + dy * dy);
                    }
                }
                e_mm += __shfl_xor(e_mm, 16, 64);
                e_mm += __shfl_xor(e_mm, 32, 64);
                if (q == 0 && valid) err_mmse[r] = e_mm;
            }
        wave_lds_sync();
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
typedef std::complex<double> zc;

inline int round_up16(int n) { return (n + 15) & ~15; }
inline int pow2_at_least(int n) {
    int v = 1;
    while (v < n) v <<= 1;
    return v;
}

// A = (noise_power I + P C)^-1 C by Gaussian elimination with partial pivoting, complex128; false: singular
static bool mmse_matrix(const double* cov, int nr, int P, double noise_power, std::vector<zc>& A) {
    std::vector<zc> M((size_t)nr * nr);
    A.assign((size_t)nr * nr, zc(0.0, 0.0));
    for (int i = 0; i < nr; ++i)
        for (int k = 0; k < nr; ++k) {
            const zc c(cov[2 * ((size_t)i * nr + k)], cov[2 * ((size_t)i * nr + k) + 1]);
            A[(size_t)i * nr + k] = c;
            M[(size_t)i * nr + k] = (double)P * c + (i == k ? zc(noise_power, 0.0) : zc(0.0, 0.0));
        }
    for (int k = 0; k < nr; ++k) {
        int piv = k;
        double best = std::abs(M[(size_t)k * nr + k]);
        for (int i = k + 1; i < nr; ++i)
            if (std::abs(M[(size_t)i * nr + k]) > best) best = std::abs(M[(size_t)i * nr + k]), piv = i;
        if (!(best > 0.0) || !std::isfinite(best)) return false;
        if (piv != k)
            for (int j = 0; j < nr; ++j) {
                std::swap(M[(size_t)k * nr + j], M[(size_t)piv * nr + j]);
                std::swap(A[(size_t)k * nr + j], A[(size_t)piv * nr + j]);
            }
        const zc inv = 1.0 / M[(size_t)k * nr + k];
        for (int i = k + 1; i < nr; ++i) {
            const zc f = M[(size_t)i * nr + k] * inv;
            if (f == zc(0.0, 0.0)) continue;
            for (int j = k; j < nr; ++j) M[(size_t)i * nr + j] -= f * M[(size_t)k * nr + j];
            for (int j = 0; j < nr; ++j) A[(size_t)i * nr + j] -= f * A[(size_t)k * nr + j];
        }
    }
    for (int k = nr - 1; k >= 0; --k) {
        const zc inv = 1.0 / M[(size_t)k * nr + k];
        for (int j = 0; j < nr; ++j) {
            zc v = A[(size_t)k * nr + j];
            for (int i = k + 1; i < nr; ++i) v -= M[(size_t)k * nr + i] * A[(size_t)i * nr + j];
            A[(size_t)k * nr + j] = v * inv;
        }
    }
    return true;
}

// The same with the last result kept: a simulator calls with one (cov, n_pilots, noise_power) batch after batch, and at
// nr = 128 the elimination (milliseconds on the host) would outweigh the kernel.  A is a pure function of its inputs, so one
// process-wide entry behind a mutex serves every context.
static bool mmse_matrix_cached(const double* cov, int nr, int P, double noise_power, std::vector<zc>& A) {
    static std::mutex mu;
    static std::vector<double> key_cov;
    static std::vector<zc> last;
    static int key_nr = 0, key_P = 0;
    static double key_noise = 0.0;
    const size_t n = 2 * (size_t)nr * nr;
    std::lock_guard<std::mutex> lock(mu);
    if (key_nr == nr && key_P == P && key_noise == noise_power && key_cov.size() == n &&
        std::memcmp(key_cov.data(), cov, n * sizeof(double)) == 0) {
        A = last;
        return true;
    }
    if (!mmse_matrix(cov, nr, P, noise_power, A)) return false;
    key_cov.assign(cov, cov + n);
    key_nr = nr, key_P = P, key_noise = noise_power;
    last = A;
    return true;
}

// scale * M [nr][nr] -> host image of the device layout: transposed, zero-padded to [nrp][nrp], complex of T
template <typename T> static void pack_transposed(const zc* M, int nr, int nrp, double scale, cx<T>* dst) {
    for (size_t i = 0; i < (size_t)nrp * nrp; ++i) dst[i] = mk<T>(0, 0);
    for (int i = 0; i < nr; ++i)
        for (int k = 0; k < nr; ++k) {
            const zc v = scale * M[(size_t)i * nr + k];
            dst[(size_t)k * nrp + i] = mk<T>((T)v.real(), (T)v.imag());
        }
}

static bool all_finite(const double* v, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

inline unsigned est_grid(const mcle_ctx* ctx, uint64_t tiles, size_t lds, int per_cu_max) {
    uint64_t per_cu = lds > 0 ? kEstLdsBudget / lds : (uint64_t)per_cu_max;
    if (per_cu > (uint64_t)per_cu_max) per_cu = per_cu_max;
    if (per_cu < 1) per_cu = 1;
    const uint64_t resident = (uint64_t)(ctx->n_cu > 0 ? ctx->n_cu : 256) * per_cu;
    return (unsigned)oversubscribed_grid(ctx, resident, tiles, 2);
}

template <typename T, int NTP>
int launch_ls(mcle_ctx* ctx, const void* d_Y, const void* d_s, int nr, int nt, int P, int per_real, size_t batch, void* d_out) {
    const size_t lds = (size_t)(per_real ? kLsTile : 1) * nt * nt * sizeof(double2);
    const size_t tiles = (batch + kLsTile - 1) / kLsTile;
    const size_t cap = (size_t)(ctx->n_cu > 0 ? ctx->n_cu : 256) * 8;
    const unsigned grid = (unsigned)(tiles < cap ? tiles : cap);
    hipLaunchKernelGGL((k_ls_estimate<T, NTP>), dim3(grid), dim3(256), lds, ctx->stream, (const cx<T>*)d_Y, (const cx<T>*)d_s, nr,
                       nt, P, per_real, batch, (cx<T>*)d_out);
    MCLE_LAUNCH_CHECK();
    ctx->set_kernel("ls_estimate %s nt%d", sizeof(T) == 8 ? "f64" : "f32", NTP);
    return MCLE_OK;
}

template <typename T>
int dispatch_ls(mcle_ctx* ctx, const void* d_Y, const void* d_s, int nr, int nt, int P, int per_real, size_t batch, void* d_out) {
    switch (pow2_at_least(nt)) {
        case 1: return launch_ls<T, 1>(ctx, d_Y, d_s, nr, nt, P, per_real, batch, d_out);
        case 2: return launch_ls<T, 2>(ctx, d_Y, d_s, nr, nt, P, per_real, batch, d_out);
        case 4: return launch_ls<T, 4>(ctx, d_Y, d_s, nr, nt, P, per_real, batch, d_out);
        default: return launch_ls<T, 8>(ctx, d_Y, d_s, nr, nt, P, per_real, batch, d_out);
    }
}

template <typename T>
int launch_mmse(mcle_ctx* ctx, const void* d_Y, const void* d_s, int nr, int P, int per_real, size_t batch,
                const std::vector<zc>& A, void* d_out) {
    const int nrp = round_up16(nr);
    const size_t bytes = (size_t)nrp * nrp * sizeof(cx<T>);
    std::vector<cx<T>> host((size_t)nrp * nrp);
    pack_transposed<T>(A.data(), nr, nrp, 1.0, host.data());
    void* d_At = nullptr;
    int rc;
    if ((rc = ctx->scratch(bytes, &d_At))) return rc;
    MCLE_HIP(hipMemcpyAsync(d_At, host.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
    MCLE_HIP(hipStreamSynchronize(ctx->stream));  // `host` goes out of scope
    const size_t lds = 2 * (size_t)nrp * 16 * sizeof(T);
    const unsigned grid = est_grid(ctx, (batch + 15) / 16, lds, 16);
    hipLaunchKernelGGL(k_mmse_estimate<T>, dim3(grid), dim3(64), lds, ctx->stream, (const cx<T>*)d_Y, (const cx<T>*)d_s, nr, nrp,
                       P, per_real, batch, (const cx<T>*)d_At, (cx<T>*)d_out);
    MCLE_LAUNCH_CHECK();
    ctx->set_kernel("mmse_estimate %s ga", sizeof(T) == 8 ? "f64" : "f32");
    return MCLE_OK;
}

template <typename T, int NTP>
int launch_pilot_mse(mcle_ctx* ctx, const PilotMseParams& p, const mcle_pilot_mse_cfg* cfg, const void* d_Lt, const void* d_At,
                     uint64_t seed, uint64_t first, uint64_t count, double* d_err_ls, double* d_err_mmse, double* d_pow) {
    constexpr int NB = 16 / NTP;
    const size_t lds = pilot_mse_lds(p, NTP, sizeof(T));
    MCLE_REQUIRE(lds <= kEstLdsBudget, "pilot_mse: nr %d, nt %d, n_pilots %d (%zu bytes of LDS per wavefront) does not fit the device's LDS",
                 p.nr, p.nt, p.P, lds);
    auto kernel = k_pilot_mse<T, NTP>;
    // (the default limit covers 64 KiB: the common sizes launch without this host round trip)
    if (lds > 63 * 1024) MCLE_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const unsigned grid = est_grid(ctx, (count + NB - 1) / NB, lds, 8);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), lds, ctx->stream, p, (const cx<T>*)cfg->d_pilots, (const cx<T>*)d_Lt,
                       (const cx<T>*)d_At, seed, first, count, d_err_ls, d_err_mmse, d_pow);
    MCLE_LAUNCH_CHECK();
    ctx->set_kernel("pilot_mse %s b%d %s%s", sizeof(T) == 8 ? "f64" : "f32", NB, p.has_mmse ? "ls+mmse" : "ls",
                    p.has_L ? " gl" : "");
    return MCLE_OK;
}

template <typename T>
int run_pilot_mse_impl(mcle_ctx* ctx, const mcle_pilot_mse_cfg* cfg, const std::vector<zc>& A, uint64_t seed, uint64_t first,
                       uint64_t count, double* d_err_ls, double* d_err_mmse, double* d_pow) {
    PilotMseParams p;
    p.nr = cfg->nr, p.nrp = round_up16(cfg->nr), p.nt = cfg->nt, p.P = cfg->n_pilots, p.half = (cfg->n_pilots + 1) / 2;
    p.random_pilots = cfg->random_pilots != 0, p.has_L = cfg->chan_factor != nullptr, p.has_mmse = cfg->cov != nullptr;
    p.amp = std::sqrt(cfg->pilot_power), p.sigma = std::sqrt(cfg->noise_power), p.alpha = cfg->alpha;
    // the two matrices travel in one block: alpha L, then A
    const size_t n_mat = (size_t)p.nrp * p.nrp;
    const int mats = (p.has_L ? 1 : 0) + (p.has_mmse ? 1 : 0);
    cx<T>*d_Lt = nullptr, *d_At = nullptr;
    int rc;
    if (mats) {
        std::vector<cx<T>> host(n_mat * mats);
        void* d_blk = nullptr;
        if ((rc = ctx->scratch(host.size() * sizeof(cx<T>), &d_blk))) return rc;
        size_t at = 0;
        if (p.has_L) {
            pack_transposed<T>(reinterpret_cast<const zc*>(cfg->chan_factor), p.nr, p.nrp, cfg->alpha, host.data());
            d_Lt = (cx<T>*)d_blk;
            at = n_mat;
        }
        if (p.has_mmse) {
            pack_transposed<T>(A.data(), p.nr, p.nrp, 1.0, host.data() + at);
            d_At = (cx<T>*)d_blk + at;
        }
        MCLE_HIP(hipMemcpyAsync(d_blk, host.data(), host.size() * sizeof(cx<T>), hipMemcpyHostToDevice, ctx->stream));
        MCLE_HIP(hipStreamSynchronize(ctx->stream));  // `host` goes out of scope
    }
    switch (pow2_at_least(p.nt)) {
        case 1: return launch_pilot_mse<T, 1>(ctx, p, cfg, d_Lt, d_At, seed, first, count, d_err_ls, d_err_mmse, d_pow);
        case 2: return launch_pilot_mse<T, 2>(ctx, p, cfg, d_Lt, d_At, seed, first, count, d_err_ls, d_err_mmse, d_pow);
        case 4: return launch_pilot_mse<T, 4>(ctx, p, cfg, d_Lt, d_At, seed, first, count, d_err_ls, d_err_mmse, d_pow);
        default: return launch_pilot_mse<T, 8>(ctx, p, cfg, d_Lt, d_At, seed, first, count, d_err_ls, d_err_mmse, d_pow);
    }
}

// the rules the two operators share
inline int est_check_common(const mcle_ctx* ctx, int dtype, int nr, int n_pilots, int s_per_realization) {
    MCLE_REQUIRE(ctx != nullptr, "null context");
    MCLE_REQUIRE(dtype == MCLE_F32 || dtype == MCLE_F64, "dtype must be MCLE_F32 or MCLE_F64");
    MCLE_REQUIRE(nr >= 1 && nr <= kEstMaxNr, "nr must be in [1, %d] (got %d)", kEstMaxNr, nr);
    MCLE_REQUIRE(n_pilots >= 1 && n_pilots <= kEstMaxPilots, "n_pilots must be in [1, %d] (got %d)", kEstMaxPilots, n_pilots);
    MCLE_REQUIRE(s_per_realization == 0 || s_per_realization == 1, "s_per_realization must be 0 or 1 (got %d)",
                 s_per_realization);
    return MCLE_OK;
}

}  // namespace mcle

using namespace mcle;

extern "C" {

int mcle_ls_estimate(mcle_ctx* ctx, int dtype, const void* d_Y, const void* d_s, int nr, int nt, int n_pilots,
                     int s_per_realization, size_t batch, void* d_out) {
    if (ctx) ctx->last_kernel[0] = 0;
    int rc;
    if ((rc = est_check_common(ctx, dtype, nr, n_pilots, s_per_realization))) return rc;
    MCLE_REQUIRE(nt >= 1 && nt <= kEstMaxNt, "nt must be in [1, %d] (got %d)", kEstMaxNt, nt);
    MCLE_REQUIRE(nt <= n_pilots, "n_pilots must be at least nt (got %d pilots, nt %d)", n_pilots, nt);
    MCLE_REQUIRE(batch <= 0x7fffffffull, "batch must be at most 2^31-1");
    if (batch == 0) return MCLE_OK;
    MCLE_REQUIRE(d_Y != nullptr && d_s != nullptr && d_out != nullptr, "null array");
    if ((rc = ctx->bind())) return rc;
    return dtype == MCLE_F32 ? dispatch_ls<float>(ctx, d_Y, d_s, nr, nt, n_pilots, s_per_realization, batch, d_out)
                             : dispatch_ls<double>(ctx, d_Y, d_s, nr, nt, n_pilots, s_per_realization, batch, d_out);
}

int mcle_mmse_estimate(mcle_ctx* ctx, int dtype, const void* d_Y, const void* d_s, int nr, int n_pilots, int s_per_realization,
                       size_t batch, double noise_power, const double* cov, void* d_out) {
    if (ctx) ctx->last_kernel[0] = 0;
    int rc;
    if ((rc = est_check_common(ctx, dtype, nr, n_pilots, s_per_realization))) return rc;
    MCLE_REQUIRE(std::isfinite(noise_power) && noise_power >= 0.0, "noise_power must be finite and non-negative");
    MCLE_REQUIRE(cov != nullptr, "null cov");
    MCLE_REQUIRE(all_finite(cov, 2 * (size_t)nr * nr), "cov holds a value that is not finite");
    MCLE_REQUIRE(batch <= 0x7fffffffull, "batch must be at most 2^31-1");
    if (batch == 0) return MCLE_OK;
    MCLE_REQUIRE(d_Y != nullptr && d_s != nullptr && d_out != nullptr, "null array");
    std::vector<zc> A;
    MCLE_REQUIRE(mmse_matrix_cached(cov, nr, n_pilots, noise_power, A), "noise_power * I + n_pilots * cov is singular");
    if ((rc = ctx->bind())) return rc;
    return dtype == MCLE_F32 ? launch_mmse<float>(ctx, d_Y, d_s, nr, n_pilots, s_per_realization, batch, A, d_out)
                             : launch_mmse<double>(ctx, d_Y, d_s, nr, n_pilots, s_per_realization, batch, A, d_out);
}

int mcle_run_pilot_mse(mcle_ctx* ctx, int dtype, const mcle_pilot_mse_cfg* cfg, uint64_t seed, uint64_t first, uint64_t count,
                       double* d_err_ls, double* d_err_mmse, double* d_pow) {
    if (ctx) ctx->last_kernel[0] = 0;
    MCLE_REQUIRE(ctx != nullptr && cfg != nullptr, "null argument");
    MCLE_REQUIRE(dtype == MCLE_F32 || dtype == MCLE_F64, "dtype must be MCLE_F32 or MCLE_F64");
    MCLE_REQUIRE(cfg->nr >= 1 && cfg->nr <= kEstMaxNr, "nr must be in [1, %d] (got %d)", kEstMaxNr, cfg->nr);
    MCLE_REQUIRE(cfg->nt >= 1 && cfg->nt <= kEstMaxNt, "nt must be in [1, %d] (got %d)", kEstMaxNt, cfg->nt);
    MCLE_REQUIRE(cfg->n_pilots >= cfg->nt, "n_pilots must be at least nt (got %d pilots, nt %d)", cfg->n_pilots, cfg->nt);
    MCLE_REQUIRE(cfg->n_pilots <= kPilotMseMaxPilots, "n_pilots must be at most %d (got %d)", kPilotMseMaxPilots, cfg->n_pilots);
    MCLE_REQUIRE(cfg->random_pilots == 0 || cfg->random_pilots == 1, "random_pilots must be 0 or 1 (got %d)", cfg->random_pilots);
    MCLE_REQUIRE(std::isfinite(cfg->noise_power) && cfg->noise_power >= 0.0, "noise_power must be finite and non-negative");
    MCLE_REQUIRE(std::isfinite(cfg->alpha), "alpha must be finite");
    MCLE_REQUIRE(!cfg->random_pilots || (std::isfinite(cfg->pilot_power) && cfg->pilot_power > 0.0),
                 "pilot_power must be finite and positive");
    MCLE_REQUIRE(cfg->random_pilots || cfg->d_pilots != nullptr, "null d_pilots with random_pilots = 0");
    MCLE_REQUIRE(cfg->cov == nullptr || cfg->nt == 1, "the MMSE estimator (cov) needs nt = 1 (got %d)", cfg->nt);
    const size_t n2 = 2 * (size_t)cfg->nr * cfg->nr;
    MCLE_REQUIRE(cfg->chan_factor == nullptr || all_finite(cfg->chan_factor, n2), "chan_factor holds a value that is not finite");
    MCLE_REQUIRE(cfg->cov == nullptr || all_finite(cfg->cov, n2), "cov holds a value that is not finite");
    MCLE_REQUIRE(count <= 0x7fffffffull, "at most 2^31-1 realizations per call");
    if (count == 0) return MCLE_OK;
    MCLE_REQUIRE(d_err_ls != nullptr && d_pow != nullptr, "null array");
    MCLE_REQUIRE(cfg->cov == nullptr || d_err_mmse != nullptr, "null d_err_mmse with cov");
    std::vector<zc> A;
    if (cfg->cov)
        MCLE_REQUIRE(mmse_matrix_cached(cfg->cov, cfg->nr, cfg->n_pilots, cfg->noise_power, A), "noise_power * I + n_pilots * cov is singular");
    int rc;
    if ((rc = ctx->bind())) return rc;
    return dtype == MCLE_F32 ? run_pilot_mse_impl<float>(ctx, cfg, A, seed, first, count, d_err_ls, d_err_mmse, d_pow)
                             : run_pilot_mse_impl<double>(ctx, cfg, A, seed, first, count, d_err_ls, d_err_mmse, d_pow);
}

}  // extern "C"
