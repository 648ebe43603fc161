// wave_lanes.hpp -- lane-level helpers of the one-wavefront-per-transform link kernels (siso_tdl_wave.hpp, mimo_tdl_wave.hpp):
// the DPP neighbour swap that hands over half of a Philox NOISE block, and v_readlane reads of values parked across the lanes;
// and the fixed-order DPP sum / minimum of a double over a wavefront (the per-drop figures of pipeline_indoor.hip).
#pragma once
#include "common.hpp"

namespace mcle {

template <typename T> __device__ __forceinline__ T dpp_swap1(T v);
template <> __device__ __forceinline__ float dpp_swap1<float>(float v) {         // the value of lane l ^ 1
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true));
}
// lane j's value of a VGPR as a wave-uniform scalar (j wave-uniform)
__device__ __forceinline__ float lane_value(float v, int j) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j)); }
__device__ __forceinline__ double lane_value(double v, int j) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), j), __builtin_amdgcn_readlane(__double2loint(v), j));
}
template <> __device__ __forceinline__ double dpp_swap1<double>(double v) {
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), 0xB1, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), 0xB1, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}

// A double moved by one DPP pattern; a lane the pattern gives no source (or whose row ROW_MASK leaves out) receives `fill`
template <int CTRL, int ROW_MASK> __device__ __forceinline__ double dpp_f64(double v, double fill) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(fill), __double2loint(v), CTRL, ROW_MASK, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(fill), __double2hiint(v), CTRL, ROW_MASK, 0xF, false);
    return __hiloint2double(hi, lo);
}
// Sum / minimum of a double over the 64 lanes as a wave-uniform scalar, on the tree of walk_f64.hpp's walk_wave_total (row_shr 1,
// 2, 4, 8, then row_bcast:15 / row_bcast:31 carry the row results up to lane 63): a FIXED order, the same bits on every launch.
__device__ __forceinline__ double wave_total_f64(double v) {
    v += dpp_f64<0x111, 0xF>(v, 0.0);
    v += dpp_f64<0x112, 0xF>(v, 0.0);
    v += dpp_f64<0x114, 0xF>(v, 0.0);
    v += dpp_f64<0x118, 0xF>(v, 0.0);
    v += dpp_f64<0x142, 0xA>(v, 0.0);
    v += dpp_f64<0x143, 0xC>(v, 0.0);
    return lane_value(v, 63);
}
__device__ __forceinline__ double wave_min_f64(double v) {
    v = fmin(v, dpp_f64<0x111, 0xF>(v, v));
    v = fmin(v, dpp_f64<0x112, 0xF>(v, v));
    v = fmin(v, dpp_f64<0x114, 0xF>(v, v));
    v = fmin(v, dpp_f64<0x118, 0xF>(v, v));
    v = fmin(v, dpp_f64<0x142, 0xA>(v, v));
    v = fmin(v, dpp_f64<0x143, 0xC>(v, v));
    return lane_value(v, 63);
}

}  // namespace mcle
