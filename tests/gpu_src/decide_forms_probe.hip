// Test-only probe of the decision forms the fused pipelines decide with, on points the TEST chooses (tests/test_gpu_decide_forms.py
// compiles this file with hipcc at test time and loads it next to libmcle.so; decide_probe.hip covers walk_decide<double, DEC, 4> alone):
//   probe_multi  demod_multi_cert<T, K> around demod_grid4_multi<K> / demod_mindist_multi<K> on the float4 table {re, im, |c|^2/2}
//                (the complex64 decision of the pipelines), around demod_grid_multi<K> / demod_mindist_multi<K> on double2 (the
//                complex128 lockstep search), and the single-symbol demod_grid4 as the K = 1 anchor -- one label per point;
//   probe_walk   walk_decide<T, DEC, N> for T = float / double, every DEC, N = 2 / 4 / 6 -- the error counts of each group.
// One thread = one group of K (N) CONSECUTIVE points: the grouping is the caller's.  Not part of the product: nothing under
// pyphysim_amd/ refers to it.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"
#include "modem.hpp"
#include "pipe_common.hpp"
#include "walk_f64.hpp"

using namespace mcle;

enum : int { FORM_GRID4_MULTI = 0, FORM_MINDIST4_MULTI = 1, FORM_GRID_MULTI = 2, FORM_MINDIST_MULTI = 3, FORM_GRID4 = 4 };
constexpr int kProbeBlock = 256, kProbeTable = 256, kProbeCells = kMaxGridCells;

// the points of group g; a slot past the end repeats the group's first point (finite, inside the set) and its label is not written
template <typename T, int K>
__device__ __forceinline__ void probe_group(const cx<T>* __restrict__ pts, int n_points, int g, cx<T> (&r)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) r[k] = pts[K * g + k < n_points ? K * g + k : K * g];
}

// complex64: the float4 table is filled in LDS with the two expressions the pipelines use -- half_form 0: from the float table,
// 0.5f * (c.x * c.x + c.y * c.y); 1: from the double table, (float)(0.5 * (c.x * c.x + c.y * c.y))
template <int FORM, int K>
__global__ __launch_bounds__(kProbeBlock) void k_probe_multi_f32(ModemParams<float> mp, const double2* __restrict__ g_table_f64, int half_form,
                                                                 const float2* __restrict__ pts, int n_points, int* __restrict__ labels) {
    __shared__ float4 s_tab4[kProbeTable];
    __shared__ unsigned long long s_grid[kProbeCells];
    for (int m = threadIdx.x; m < mp.M; m += blockDim.x) {
        if (half_form == 0) {
            const float2 c = mp.g_table[m];
            s_tab4[m] = make_float4(c.x, c.y, 0.5f * (c.x * c.x + c.y * c.y), 0.f);
        } else {
            const double2 c = g_table_f64[m];
            s_tab4[m] = make_float4((float)c.x, (float)c.y, (float)(0.5 * (c.x * c.x + c.y * c.y)), 0.f);
        }
    }
    load_grid(mp, s_grid);
    __syncthreads();
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if ((long long)K * g >= n_points) return;
    float2 r[K];
    int dec[K];
    probe_group<float, K>(pts, n_points, g, r);
    if constexpr (FORM == FORM_GRID4_MULTI) {
        demod_multi_cert(mp, r, dec, [&](int (&d_)[K]) { demod_grid4_multi<K>(s_tab4, s_grid, mp.grid, mp.M, r, d_); });
    } else if constexpr (FORM == FORM_MINDIST4_MULTI) {
        demod_multi_cert(mp, r, dec, [&](int (&d_)[K]) { demod_mindist_multi<K>(s_tab4, mp.M, r, d_); });
    } else {
        static_assert(K == 1, "demod_grid4 decides one symbol");
        demod_multi_cert(mp, r, dec, [&](int (&d_)[K]) { d_[0] = demod_grid4(s_tab4, s_grid, mp.grid, mp.M, r[0]); });
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (K * g + k < n_points) labels[K * g + k] = dec[k];
}

template <int FORM, int K>
__global__ __launch_bounds__(kProbeBlock) void k_probe_multi_f64(ModemParams<double> mp, const double2* __restrict__ pts, int n_points,
                                                                 int* __restrict__ labels) {
    __shared__ double2 s_table[kProbeTable];
    __shared__ unsigned long long s_grid[kProbeCells];
    load_table(mp, s_table);
    load_grid(mp, s_grid);
    __syncthreads();
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if ((long long)K * g >= n_points) return;
    double2 r[K];
    int dec[K];
    probe_group<double, K>(pts, n_points, g, r);
    if constexpr (FORM == FORM_GRID_MULTI) {
        demod_multi_cert(mp, r, dec, [&](int (&d_)[K]) { demod_grid_multi<K>(s_table, s_grid, mp.grid, mp.M, r, d_); });
    } else {
        demod_multi_cert(mp, r, dec, [&](int (&d_)[K]) { demod_mindist_multi<K>(s_table, mp.M, r, d_); });
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (K * g + k < n_points) labels[K * g + k] = dec[k];
}

// one thread = one group of N estimates: its symbol / bit error counts against the N labels in tx
template <typename T, int DEC, int N>
__global__ __launch_bounds__(kProbeBlock) void k_probe_walk(ModemParams<T> mp, const cx<T>* __restrict__ pts, const int* __restrict__ tx,
                                                            int n_groups, unsigned* __restrict__ se_out, unsigned* __restrict__ be_out) {
    __shared__ cx<T> s_table[kProbeTable];
    __shared__ unsigned long long s_grid[kProbeCells];
    load_table(mp, s_table);
    load_grid(mp, s_grid);
    __syncthreads();
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    cx<T> e[N];
    int t[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        e[i] = pts[(size_t)N * g + i];
        t[i] = tx[(size_t)N * g + i];
    }
    unsigned se = 0, be = 0;
    walk_decide<T, DEC, N>(mp, s_table, s_grid, e, t, se, be);
    se_out[g] = se;
    be_out[g] = be;
}

namespace {

// device buffers of one call: freed on every way out
struct ProbeBuffers {
    void* p[4] = {nullptr, nullptr, nullptr, nullptr};
    ~ProbeBuffers() {
        for (void* q : p)
            if (q) (void)hipFree(q);
    }
};
#define PROBE_HIP(call) \
    if ((err = (call)) != hipSuccess) return -1000 - (int)err

template <int FORM, int K>
void launch_multi_f32(const ModemParams<float>& mp, const double2* t64, int half_form, const float2* pts, int n, int* lab) {
    const int groups = (n + K - 1) / K;
    hipLaunchKernelGGL((k_probe_multi_f32<FORM, K>), dim3((unsigned)((groups + kProbeBlock - 1) / kProbeBlock)), dim3(kProbeBlock), 0, 0, mp, t64,
                       half_form, pts, n, lab);
}
template <int FORM, int K> void launch_multi_f64(const ModemParams<double>& mp, const double2* pts, int n, int* lab) {
    const int groups = (n + K - 1) / K;
    hipLaunchKernelGGL((k_probe_multi_f64<FORM, K>), dim3((unsigned)((groups + kProbeBlock - 1) / kProbeBlock)), dim3(kProbeBlock), 0, 0, mp, pts, n,
                       lab);
}
template <int FORM> void launch_multi_f32_k(int K, const ModemParams<float>& mp, const double2* t64, int hf, const float2* pts, int n, int* lab) {
    switch (K) {
        case 1: launch_multi_f32<FORM, 1>(mp, t64, hf, pts, n, lab); break;
        case 2: launch_multi_f32<FORM, 2>(mp, t64, hf, pts, n, lab); break;
        case 3: launch_multi_f32<FORM, 3>(mp, t64, hf, pts, n, lab); break;
        default: launch_multi_f32<FORM, 4>(mp, t64, hf, pts, n, lab); break;
    }
}
template <int FORM> void launch_multi_f64_k(int K, const ModemParams<double>& mp, const double2* pts, int n, int* lab) {
    switch (K) {
        case 1: launch_multi_f64<FORM, 1>(mp, pts, n, lab); break;
        case 2: launch_multi_f64<FORM, 2>(mp, pts, n, lab); break;
        case 3: launch_multi_f64<FORM, 3>(mp, pts, n, lab); break;
        default: launch_multi_f64<FORM, 4>(mp, pts, n, lab); break;
    }
}

template <typename T, int DEC>
void launch_walk_n(int N, const ModemParams<T>& mp, const cx<T>* pts, const int* tx, int n_groups, unsigned* se, unsigned* be) {
    const dim3 grid((unsigned)((n_groups + kProbeBlock - 1) / kProbeBlock)), block(kProbeBlock);
    switch (N) {
        case 2: hipLaunchKernelGGL((k_probe_walk<T, DEC, 2>), grid, block, 0, 0, mp, pts, tx, n_groups, se, be); break;
        case 4: hipLaunchKernelGGL((k_probe_walk<T, DEC, 4>), grid, block, 0, 0, mp, pts, tx, n_groups, se, be); break;
        default: hipLaunchKernelGGL((k_probe_walk<T, DEC, 6>), grid, block, 0, 0, mp, pts, tx, n_groups, se, be); break;
    }
}

template <typename T>
int walk_host(mcle_ctx* ctx, int method, int N, const void* pts_host, const int* tx_host, int n_groups, unsigned* se_host, unsigned* be_host) {
    ModemParams<T> mp = pipe_modem<T>(ctx, method);
    const int dec = walk_dec_kind(ctx, mp);
    ProbeBuffers b;
    const size_t n = (size_t)N * n_groups;
    hipError_t err;
    PROBE_HIP(hipMalloc(&b.p[0], n * sizeof(cx<T>)));
    PROBE_HIP(hipMalloc(&b.p[1], n * sizeof(int)));
    PROBE_HIP(hipMalloc(&b.p[2], n_groups * sizeof(unsigned)));
    PROBE_HIP(hipMalloc(&b.p[3], n_groups * sizeof(unsigned)));
    PROBE_HIP(hipMemcpy(b.p[0], pts_host, n * sizeof(cx<T>), hipMemcpyHostToDevice));
    PROBE_HIP(hipMemcpy(b.p[1], tx_host, n * sizeof(int), hipMemcpyHostToDevice));
    const cx<T>* d_pts = static_cast<const cx<T>*>(b.p[0]);
    const int* d_tx = static_cast<const int*>(b.p[1]);
    unsigned *d_se = static_cast<unsigned*>(b.p[2]), *d_be = static_cast<unsigned*>(b.p[3]);
    switch (dec) {
        case WDEC_GENERIC: launch_walk_n<T, WDEC_GENERIC>(N, mp, d_pts, d_tx, n_groups, d_se, d_be); break;
        case WDEC_SLICER: launch_walk_n<T, WDEC_SLICER>(N, mp, d_pts, d_tx, n_groups, d_se, d_be); break;
        case WDEC_QAM_CERT: launch_walk_n<T, WDEC_QAM_CERT>(N, mp, d_pts, d_tx, n_groups, d_se, d_be); break;
        case WDEC_QUAD_CERT: launch_walk_n<T, WDEC_QUAD_CERT>(N, mp, d_pts, d_tx, n_groups, d_se, d_be); break;
        default: launch_walk_n<T, WDEC_AXIS4_CERT>(N, mp, d_pts, d_tx, n_groups, d_se, d_be); break;
    }
    PROBE_HIP(hipGetLastError());
    PROBE_HIP(hipDeviceSynchronize());
    PROBE_HIP(hipMemcpy(se_host, d_se, n_groups * sizeof(unsigned), hipMemcpyDeviceToHost));
    PROBE_HIP(hipMemcpy(be_host, d_be, n_groups * sizeof(unsigned), hipMemcpyDeviceToHost));
    return dec;
}

}  // namespace

// host: one int32 label per point.  dtype MCLE_F32 with FORM_GRID4_MULTI / FORM_MINDIST4_MULTI / FORM_GRID4 (K = 1), MCLE_F64 with
// FORM_GRID_MULTI / FORM_MINDIST_MULTI; pts: interleaved (re, im) of that dtype.  Returns 0, -1 for arguments outside that, -2 where the
// context binds no candidate grid (or a table beyond the probe's LDS arrays), -1000 - the HIP error.  The context's options decide
// whether certificates are on (demod_nocert), as in the pipelines: ModemParams come from pipe_modem.
extern "C" int probe_multi(mcle_ctx* ctx, int dtype, int form, int K, int half_form, const void* pts_host, int n_points, int* labels_host) {
    if (ctx == nullptr || pts_host == nullptr || labels_host == nullptr || n_points <= 0 || K < 1 || K > 4) return -1;
    if (half_form != 0 && half_form != 1) return -1;
    const bool f32 = dtype == MCLE_F32;
    if (f32 ? !(form == FORM_GRID4_MULTI || form == FORM_MINDIST4_MULTI || (form == FORM_GRID4 && K == 1))
            : !(dtype == MCLE_F64 && (form == FORM_GRID_MULTI || form == FORM_MINDIST_MULTI)))
        return -1;
    if (ctx->M < 2 || ctx->M > kProbeTable) return -2;
    ProbeBuffers b;
    hipError_t err;
    const size_t point_bytes = f32 ? sizeof(float2) : sizeof(double2);
    PROBE_HIP(hipMalloc(&b.p[0], (size_t)n_points * point_bytes));
    PROBE_HIP(hipMalloc(&b.p[1], (size_t)n_points * sizeof(int)));
    PROBE_HIP(hipMemcpy(b.p[0], pts_host, (size_t)n_points * point_bytes, hipMemcpyHostToDevice));
    int* d_lab = static_cast<int*>(b.p[1]);
    if (f32) {
        const ModemParams<float> mp = pipe_modem<float>(ctx, MCLE_DEMOD_MINDIST);
        if (mp.grid.G <= 0 || mp.grid.G * mp.grid.G > kProbeCells) return -2;
        const float2* d_pts = static_cast<const float2*>(b.p[0]);
        const double2* t64 = ctx->d_table_f64;
        if (form == FORM_GRID4_MULTI) launch_multi_f32_k<FORM_GRID4_MULTI>(K, mp, t64, half_form, d_pts, n_points, d_lab);
        else if (form == FORM_MINDIST4_MULTI) launch_multi_f32_k<FORM_MINDIST4_MULTI>(K, mp, t64, half_form, d_pts, n_points, d_lab);
        else launch_multi_f32<FORM_GRID4, 1>(mp, t64, half_form, d_pts, n_points, d_lab);
    } else {
        const ModemParams<double> mp = pipe_modem<double>(ctx, MCLE_DEMOD_MINDIST);
        if (mp.grid.G <= 0 || mp.grid.G * mp.grid.G > kProbeCells) return -2;
        const double2* d_pts = static_cast<const double2*>(b.p[0]);
        if (form == FORM_GRID_MULTI) launch_multi_f64_k<FORM_GRID_MULTI>(K, mp, d_pts, n_points, d_lab);
        else launch_multi_f64_k<FORM_MINDIST_MULTI>(K, mp, d_pts, n_points, d_lab);
    }
    PROBE_HIP(hipGetLastError());
    PROBE_HIP(hipDeviceSynchronize());
    PROBE_HIP(hipMemcpy(labels_host, d_lab, (size_t)n_points * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

// host: the error counts of n_groups groups of N consecutive points against the labels in tx; returns the decision form the
// library would compile for this context, method and arithmetic (WDEC_*), -1 for bad arguments, -2 for a table beyond the probe's
// LDS arrays, -1000 - the HIP error
extern "C" int probe_walk(mcle_ctx* ctx, int dtype, int method, int N, const void* pts_host, const int* tx_host, int n_groups,
                          unsigned* se_host, unsigned* be_host) {
    if (ctx == nullptr || pts_host == nullptr || tx_host == nullptr || se_host == nullptr || be_host == nullptr || n_groups <= 0) return -1;
    if (!(N == 2 || N == 4 || N == 6) || !(dtype == MCLE_F32 || dtype == MCLE_F64)) return -1;
    if (!(method == MCLE_DEMOD_MINDIST || (method == MCLE_DEMOD_QAM_SLICER && ctx->kind == MCLE_CONST_QAM))) return -1;
    if (ctx->M < 2 || ctx->M > kProbeTable || ctx->grid_G * ctx->grid_G > kProbeCells) return -2;
    if (dtype == MCLE_F32) return walk_host<float>(ctx, method, N, pts_host, tx_host, n_groups, se_host, be_host);
    return walk_host<double>(ctx, method, N, pts_host, tx_host, n_groups, se_host, be_host);
}
