// Test-only probe of the two wavefront reductions of a 32-bit count: csrc/common.hpp::wave_sum_u32 (six ds_bpermute_b32 round trips,
// the sum in every lane) against csrc/walk_f64.hpp::walk_wave_total (six v_add_u32 with DPP modifiers, the sum read from lane 63 as
// a scalar) -- tests/test_gpu_wave_total.py compiles this file with hipcc at test time and loads it next to libmcle.so.  The
// headline complex128 kernel takes its per-realization error totals by the second since round 22; the sums are 32-bit unsigned and
// must be the same WORDS, wrap-around included.  Not part of the product: nothing under pyphysim_amd/ refers to it.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"
#include "modem.hpp"
#include "pipe_common.hpp"
#include "walk_f64.hpp"

using namespace mcle;

// one wavefront = one vector of 64 words: both reductions of it, and whether they differ in any lane's view
__global__ void k_wave_total_probe(const uint32_t* __restrict__ in, int n_vec, uint32_t* __restrict__ sum_out,
                                   uint32_t* __restrict__ dpp_out, unsigned* __restrict__ n_diff) {
    const int lane = threadIdx.x & 63;
    const int vec = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);         // (wave-uniform: the block is a multiple of 64)
    if (vec >= n_vec) return;
    const uint32_t x = in[(size_t)vec * 64 + lane];
    const uint32_t a = wave_sum_u32(x);                                           // every lane holds the sum
    const uint32_t b = walk_wave_total(x);                                        // a scalar
    if (a != b) atomicAdd(n_diff, 1u);                                            // (any lane whose sum is not the scalar)
    if (lane == 0) {
        sum_out[vec] = a;
        dpp_out[vec] = b;
    }
}

// host: 0, or -1000 - the HIP error
extern "C" int probe_wave_total(const uint32_t* in_host, int n_vec, uint32_t* sum_host, uint32_t* dpp_host, unsigned* n_diff_host) {
    uint32_t *d_in = nullptr, *d_sum = nullptr, *d_dpp = nullptr;
    unsigned* d_diff = nullptr;
    const size_t n = (size_t)64 * n_vec;
    hipError_t err;
#define PROBE_HIP(call) \
    if ((err = (call)) != hipSuccess) return -1000 - (int)err
    PROBE_HIP(hipMalloc(&d_in, n * sizeof(uint32_t)));
    PROBE_HIP(hipMalloc(&d_sum, n_vec * sizeof(uint32_t)));
    PROBE_HIP(hipMalloc(&d_dpp, n_vec * sizeof(uint32_t)));
    PROBE_HIP(hipMalloc(&d_diff, sizeof(unsigned)));
    PROBE_HIP(hipMemcpy(d_in, in_host, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    PROBE_HIP(hipMemset(d_diff, 0, sizeof(unsigned)));
    const dim3 grid((unsigned)((n_vec + 3) / 4)), block(256);                     // four wavefronts = four vectors per workgroup
    hipLaunchKernelGGL(k_wave_total_probe, grid, block, 0, 0, d_in, n_vec, d_sum, d_dpp, d_diff);
    PROBE_HIP(hipGetLastError());
    PROBE_HIP(hipDeviceSynchronize());
    PROBE_HIP(hipMemcpy(sum_host, d_sum, n_vec * sizeof(uint32_t), hipMemcpyDeviceToHost));
    PROBE_HIP(hipMemcpy(dpp_host, d_dpp, n_vec * sizeof(uint32_t), hipMemcpyDeviceToHost));
    PROBE_HIP(hipMemcpy(n_diff_host, d_diff, sizeof(unsigned), hipMemcpyDeviceToHost));
    (void)hipFree(d_in);
    (void)hipFree(d_sum);
    (void)hipFree(d_dpp);
    (void)hipFree(d_diff);
#undef PROBE_HIP
    return 0;
}
