// wave_draws.hpp -- wave-cooperative use of the mcle-philox-v1 streams for the kernels in which ONE wavefront
// walks the symbol columns of a realization (the record-walking link kernels: k_ia_link, k_bd_link, k_mimo_flat_link,
// k_mimo_pilot_link, k_mimo_large_link, k_comp_link, k_iagl_link; the packed walk of walk_f64.hpp).
//
// The contract fixes which Philox block a draw comes from: symbol n is byte n & 15 of DATA block n >> 4,
// complex normal i is the word pair i & 1 of its stream's block i >> 1.  A lane that takes one column per pass
// spends a full Philox evaluation (40 quarter-rate multiplies) on one byte and one on each half-used noise
// block.  Here a pass covers 128 columns, lane l owning columns t0 + 2l and t0 + 2l + 1:
//   * noise: for an even row stride the two columns are the two samples of ONE block (cn_pair) -- every word used;
//   * symbols: the (at most) 9 blocks that cover a stream's 128 positions are evaluated by 9 different lanes in
//     the SAME Philox call as the blocks of six other streams (7 x 9 = 63 lanes), and each lane fetches the word
//     holding its two bytes with four ds_bpermute.
// Values are identical to symbol_at / cn_sample position by position (tests/test_gpu_pipelines.py compare the
// kernels with the oracle's draws); only who computes them changes.  Needs an even number of columns per row.
//
// Three forms, by who owns which bytes:
//   * wave_symbol_pairs: rows of a C-order matrix (row j at j * stride + column).  A lane's two bytes of a row lie in a block
//     that 7 other lanes need too: the wave evaluates each block once and the lanes fetch their word.  Every lane takes part.
//   * fortran_symbol_pair: Fortran order (column t at t * layers + l).  A lane's two columns are 2 * layers <= 8 consecutive
//     bytes, in one block or two: the lane evaluates them itself and shifts them out of one 64-bit window.
//   * block_symbol: ONE symbol out of a block the caller holds, where the position is lane-dependent with no such structure
//     (k_mimo_large_link: a lane owns antenna 4 p + g of column 2 n).  By 64-bit shifts.
#pragma once
#include "philox.hpp"

namespace mcle {

constexpr int kPairCols = 128;            // columns per wave pass
constexpr int kBlocksPerRun = 9;          // 128 bytes at any alignment touch <= 9 sixteen-byte blocks
constexpr int kStreamsPerRound = 64 / kBlocksPerRun;   // 7

// Symbols of `n_streams` rows (row j at positions j * stride + column) for columns t0 + 2 * lane (+ 1).
// stride even, t0 a multiple of 128.  s0[j], s1[j] valid for j < n_streams.
template <int MAXS>
__device__ __forceinline__ void wave_symbol_pairs(const Rng& rng, int n_streams, uint32_t stride, uint32_t t0,
                                                  uint32_t mask, int lane, int (&s0)[MAXS], int (&s1)[MAXS]) {
    const int jj = lane / kBlocksPerRun, bi = lane - jj * kBlocksPerRun;
#pragma unroll
    for (int j0 = 0; j0 < MAXS; j0 += kStreamsPerRound) {
        if (j0 >= n_streams) break;
        // producer side: lane -> (stream j0 + jj, block bi of that stream's run)
        const uint32_t qb = (uint32_t)(j0 + jj) * stride + t0;
        const Words4 blk = rng.block(STREAM_DATA, (qb >> 4) + (uint32_t)bi);
#pragma unroll
        for (int k = 0; k < kStreamsPerRound; ++k) {
            const int j = j0 + k;
            if (j >= MAXS || j >= n_streams) break;
            const uint32_t base = (uint32_t)j * stride + t0;
            const uint32_t q = base + 2u * (uint32_t)lane;
            const int src = k * kBlocksPerRun + (int)((q >> 4) - (base >> 4));
            const uint32_t w0 = (uint32_t)__shfl((int)blk.w[0], src, 64), w1 = (uint32_t)__shfl((int)blk.w[1], src, 64);
            const uint32_t w2 = (uint32_t)__shfl((int)blk.w[2], src, 64), w3 = (uint32_t)__shfl((int)blk.w[3], src, 64);
            const uint32_t sel = (q >> 2) & 3u;
            const uint32_t word = sel == 0 ? w0 : (sel == 1 ? w1 : (sel == 2 ? w2 : w3));
            const uint32_t sh = (q & 3u) * 8u;          // q even: bytes sh and sh + 8 of the same word
            s0[j] = (int)((word >> sh) & mask);
            s1[j] = (int)((word >> (sh + 8u)) & mask);
        }
    }
}

// Fortran order: the labels of columns t and t + 1 for `layers` <= MAXL layers, from DATA positions t * layers + l.  The
// 2 * layers bytes are consecutive (<= 8 bytes, in one block unless layers == 3).  s0[l], s1[l] are written for l < layers.
template <int MAXL>
__device__ __forceinline__ void fortran_symbol_pair(const Rng& rng, int layers, uint32_t t, uint32_t mask, int (&s0)[MAXL],
                                                    int (&s1)[MAXL]) {
    static_assert(MAXL <= 4, "two columns of MAXL layers are one 64-bit window");
    const uint32_t q = t * (uint32_t)layers;
    const Words4 b0 = rng.block(STREAM_DATA, q >> 4);
    Words4 b1 = b0;
    if ((q & 15u) + 2u * (uint32_t)layers > 16u) b1 = rng.block(STREAM_DATA, (q >> 4) + 1u);
    // the eight bytes from position q & 15 on, as one word: byte e = column e / layers, layer e % layers.  By 64-bit shifts and
    // static indices into s0 / s1: word selects per byte, in a function of its own, end as run-time-indexed stores and park the
    // labels in scratch (24 - 48 bytes in k_mimo_flat_link<double> and k_mimo_pilot_link)
    const uint64_t lo = (uint64_t)b0.w[0] | ((uint64_t)b0.w[1] << 32), hi = (uint64_t)b0.w[2] | ((uint64_t)b0.w[3] << 32);
    const uint64_t nx = (uint64_t)b1.w[0] | ((uint64_t)b1.w[1] << 32);
    const bool up = (q & 8u) != 0u;
    const uint64_t x = up ? hi : lo, y = up ? nx : hi;
    const uint32_t sh = (q & 7u) * 8u;
    const uint64_t v0 = sh ? (x >> sh) | (y << (64u - sh)) : x;
    const uint64_t v1 = v0 >> (8u * (uint32_t)layers);
#pragma unroll
    for (int l = 0; l < MAXL; ++l)
        if (l < layers) {
            s0[l] = (int)((uint32_t)(v0 >> (8 * l)) & mask);
            s1[l] = (int)((uint32_t)(v1 >> (8 * l)) & mask);
        }
}

// symbol n of the data stream out of its block: byte n & 15 of the four words (symbol_at).  By 64-bit shifts, not by selects of
// b.w[i]: the backend turns those into a lane-indexed read of the block parked in scratch (philox.hpp: cn_sample)
__device__ __forceinline__ int block_symbol(const Words4& b, uint32_t n, uint32_t mask) {
    const uint64_t lo = (uint64_t)b.w[0] | ((uint64_t)b.w[1] << 32), hi = (uint64_t)b.w[2] | ((uint64_t)b.w[3] << 32);
    return (int)((uint32_t)(((n & 8u) ? hi : lo) >> ((n & 7u) * 8u)) & mask);
}

}  // namespace mcle
