// Test-only probe of the complex128 noise sample on the DEVICE: cn_from_words_lds_pairs (one phase, the witness) and
// cn_finish(cn_fetch_lds_pairs(...)) (two phases, the form the headline kernel's pipelined draw uses) on word pairs the TEST
// chooses, both from ONE LDS copy of the tables, compared as 64-bit patterns in the kernel, component by component.  The library is
// built with contraction on: that the split form compiles to the same fusions (ang - theta_k into the product in front of it) has
// to be shown on the device, not assumed from the host build (tests/test_gpu_bm_phase.py compiles this file with hipcc at test
// time, with the library's flags).  Each form takes its words through an empty asm statement, so the compiler cannot see that the
// two take the same input and merge them into one evaluation.  Not part of the product: nothing under pyphysim_amd/ refers to it.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "philox.hpp"

using namespace mcle;

__device__ __forceinline__ uint32_t hidden(uint32_t w) {
    asm volatile("" : "+v"(w));
    return w;
}

// diffs[0] / diffs[1]: pairs whose real / imaginary parts differ; first_bad: the smallest index with a difference (n if none);
// out[2 i], out[2 i + 1] = the two-phase sample, i < n_out
__global__ void __launch_bounds__(256) k_bm_phase_probe(const uint32_t* __restrict__ x0s, const uint32_t* __restrict__ x1s, size_t n, double sigma,
                                                        double* __restrict__ out, size_t n_out, unsigned long long* __restrict__ diffs,
                                                        unsigned long long* __restrict__ first_bad) {
    __shared__ __attribute__((aligned(16))) double s_bm[(kBmLdsDoubles + 1) & ~1];
    bm_tables_to_lds_pairs(s_bm, (int)threadIdx.x, (int)blockDim.x);
    __syncthreads();
    unsigned long long bad[2] = {0, 0};
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t x0 = x0s[i], x1 = x1s[i];
        const double2 a = cn_from_words_lds_pairs(hidden(x0), hidden(x1), sigma, s_bm);
        const BmFetched t = cn_fetch_lds_pairs(hidden(x0), hidden(x1), s_bm);
        const double2 b = cn_finish(t, sigma);
        const bool dx = __builtin_bit_cast(uint64_t, a.x) != __builtin_bit_cast(uint64_t, b.x);
        const bool dy = __builtin_bit_cast(uint64_t, a.y) != __builtin_bit_cast(uint64_t, b.y);
        bad[0] += dx;
        bad[1] += dy;
        if (dx || dy) atomicMin(first_bad, (unsigned long long)i);
        if (i < n_out) {
            out[2 * i] = b.x;
            out[2 * i + 1] = b.y;
        }
    }
#pragma unroll
    for (int f = 0; f < 2; ++f)
        if (bad[f]) atomicAdd(diffs + f, bad[f]);
}

// host: 0, or -1000 - the HIP error.  diffs_host[2], *first_bad_host = n when the forms agree everywhere
extern "C" int probe_bm_phase(const uint32_t* x0_host, const uint32_t* x1_host, size_t n, double sigma, double* out_host, size_t n_out,
                              unsigned long long* diffs_host, unsigned long long* first_bad_host) {
    if (n == 0 || n_out > n) return -1;
    uint32_t* d_words = nullptr;                        // x0[n], x1[n]
    double* d_out = nullptr;
    unsigned long long* d_res = nullptr;               // diffs[2], first_bad
    unsigned long long init[3] = {0, 0, (unsigned long long)n};
    hipError_t err;
#define PROBE_HIP(call) \
    if ((err = (call)) != hipSuccess) return -1000 - (int)err
    PROBE_HIP(hipMalloc(&d_words, 2 * n * sizeof(uint32_t)));
    PROBE_HIP(hipMalloc(&d_out, (n_out ? 2 * n_out : 1) * sizeof(double)));
    PROBE_HIP(hipMalloc(&d_res, sizeof init));
    PROBE_HIP(hipMemcpy(d_words, x0_host, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    PROBE_HIP(hipMemcpy(d_words + n, x1_host, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    PROBE_HIP(hipMemcpy(d_res, init, sizeof init, hipMemcpyHostToDevice));
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_bm_phase_probe, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, 0, d_words, d_words + n, n, sigma, d_out,
                       n_out, d_res, d_res + 2);
    PROBE_HIP(hipGetLastError());
    PROBE_HIP(hipDeviceSynchronize());
    PROBE_HIP(hipMemcpy(init, d_res, sizeof init, hipMemcpyDeviceToHost));
    if (n_out) PROBE_HIP(hipMemcpy(out_host, d_out, 2 * n_out * sizeof(double), hipMemcpyDeviceToHost));
    (void)hipFree(d_words);
    (void)hipFree(d_out);
    (void)hipFree(d_res);
#undef PROBE_HIP
    for (int f = 0; f < 2; ++f) diffs_host[f] = init[f];
    *first_bad_host = init[2];
    return 0;
}
