// cb_tile.hpp -- the 16 x 16 x 4 matrix-core step in either arithmetic, shared by kernels_codebook.hip and kernels_quant.hip.
#pragma once
#include "common.hpp"

namespace mcle {

typedef float cb_f32x4 __attribute__((ext_vector_type(4)));
typedef double cb_f64x4 __attribute__((ext_vector_type(4)));

// the 16 x 16 x 4 matrix-core step in either arithmetic: lane l supplies A[l & 15][l >> 4] and B[l >> 4][l & 15]; result i of
// lane l is D[row(l, i)][l & 15] -- the two arithmetics number the rows differently
template <typename T> struct CbTile;
template <> struct CbTile<float> {
    using acc = cb_f32x4;
    static __device__ __forceinline__ acc mma(float a, float b, acc c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row(int lane, int i) { return (lane >> 4) * 4 + i; }
};
template <> struct CbTile<double> {
    using acc = cb_f64x4;
    static __device__ __forceinline__ acc mma(double a, double b, acc c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row(int lane, int i) { return (lane >> 4) + 4 * i; }
};

}  // namespace mcle
