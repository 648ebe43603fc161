// Test-only probe of csrc/bm_f64.hpp on the DEVICE: bm_neg_log (the form tests/test_bm_f64_cpu.py pins) and bm_neg_log_q (the form
// the complex128 pipelines draw with) on words the TEST chooses, compared as 64-bit patterns in the kernel.  The library is built
// with contraction on, so the device's expressions are not the host's: that the two forms agree word for word has to be shown
// here as well as on the host (tests/test_gpu_bm_logq.py compiles this file with hipcc at test time, with the library's flags).
// Not part of the product: nothing under pyphysim_amd/ refers to it.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "bm_f64.hpp"

using namespace mcle;

// diffs[0]: new form, global table        vs  old form, global table
// diffs[1]: new form, LDS copy (pairs: one 16-byte read, bm_tables_to_lds_pairs)      vs  old
// diffs[2]: new form, LDS copy (two 8-byte reads, bm_tables_to_lds)                   vs  old
// first_bad: the smallest index with any difference (n if none); out[i] = the new form's value, i < n_out
__global__ void __launch_bounds__(256) k_bm_probe(const uint32_t* __restrict__ words, size_t n, double* __restrict__ out, size_t n_out,
                                                  unsigned long long* __restrict__ diffs, unsigned long long* __restrict__ first_bad) {
    __shared__ __attribute__((aligned(16))) double s_pairs[kBmLdsDoubles];
    __shared__ __attribute__((aligned(16))) double s_plain[kBmLdsDoubles];
    bm_tables_to_lds_pairs(s_pairs, (int)threadIdx.x, (int)blockDim.x);
    bm_tables_to_lds(s_plain, (int)threadIdx.x, (int)blockDim.x);
    __syncthreads();
    unsigned long long bad[3] = {0, 0, 0};
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t x0 = words[i];
        const uint64_t w = __builtin_bit_cast(uint64_t, bm_neg_log(x0));
        const double q = bm_neg_log_q(x0);
        const uint64_t v[3] = {__builtin_bit_cast(uint64_t, q), __builtin_bit_cast(uint64_t, bm_neg_log_q<true>(x0, s_pairs)),
                               __builtin_bit_cast(uint64_t, bm_neg_log_q(x0, s_plain))};
        bool any = false;
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            bad[f] += v[f] != w;
            any = any || v[f] != w;
        }
        if (any) atomicMin(first_bad, (unsigned long long)i);
        if (i < n_out) out[i] = q;
    }
#pragma unroll
    for (int f = 0; f < 3; ++f)
        if (bad[f]) atomicAdd(diffs + f, bad[f]);
}

// host: 0, or -1000 - the HIP error.  diffs_host[3], *first_bad_host = n when the forms agree everywhere
extern "C" int probe_bm_logq(const uint32_t* words_host, size_t n, double* out_host, size_t n_out, unsigned long long* diffs_host,
                             unsigned long long* first_bad_host) {
    if (n == 0 || n_out > n) return -1;
    uint32_t* d_words = nullptr;
    double* d_out = nullptr;
    unsigned long long* d_res = nullptr;               // diffs[3], first_bad
    unsigned long long init[4] = {0, 0, 0, (unsigned long long)n};
    hipError_t err;
#define PROBE_HIP(call) \
    if ((err = (call)) != hipSuccess) return -1000 - (int)err
    PROBE_HIP(hipMalloc(&d_words, n * sizeof(uint32_t)));
    PROBE_HIP(hipMalloc(&d_out, (n_out ? n_out : 1) * sizeof(double)));
    PROBE_HIP(hipMalloc(&d_res, sizeof init));
    PROBE_HIP(hipMemcpy(d_words, words_host, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    PROBE_HIP(hipMemcpy(d_res, init, sizeof init, hipMemcpyHostToDevice));
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_bm_probe, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, 0, d_words, n, d_out, n_out, d_res, d_res + 3);
    PROBE_HIP(hipGetLastError());
    PROBE_HIP(hipDeviceSynchronize());
    PROBE_HIP(hipMemcpy(init, d_res, sizeof init, hipMemcpyDeviceToHost));
    if (n_out) PROBE_HIP(hipMemcpy(out_host, d_out, n_out * sizeof(double), hipMemcpyDeviceToHost));
    (void)hipFree(d_words);
    (void)hipFree(d_out);
    (void)hipFree(d_res);
#undef PROBE_HIP
    for (int f = 0; f < 3; ++f) diffs_host[f] = init[f];
    *first_bad_host = init[3];
    return 0;
}
