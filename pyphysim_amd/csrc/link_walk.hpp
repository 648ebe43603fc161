// link_walk.hpp -- what the record-walking link kernels share.  A workgroup of four independent wavefronts walks the symbol
// columns of chunks of realizations, a realization's coefficients coming from the record a set-up kernel wrote:
// k_mimo_flat_link, k_mimo_pilot_link, k_mimo_large_link, k_mimo_large_pilot_link (those two share their whole walk:
// mimo_large_link.hpp), k_ia_link, k_bd_link, k_comp_link, k_iagl_link.  A new link of this kind brings its estimate arithmetic
// and its record layout; the prologue, the draws (wave_draws.hpp), the decisions and the per-realization tail are here.
//
// The decision form of these walks is a RUN-TIME property of the launch (the demodulation method and the constellation pick it
// inside one compiled kernel).  walk_f64.hpp is the other kind: the packed walk, walk_decide<T, DEC, N> with the form a
// template parameter.
#pragma once
#include "modem.hpp"
#include "philox.hpp"
#include "qam_pack.hpp"
#include "totals.hpp"

namespace mcle {

// What the decisions of a column need, fixed for the launch.
template <typename T> struct LinkDecide {
    const ModemParams<T>& mp;
    const cx<T>* s_table;
    const float4* s_tab4;
    const unsigned long long* s_grid;
    QamPack qp;
    uint32_t layer_mask;     // packed form: one byte per live layer
    bool lockstep, packed;   // complex64 only: the layers searched in lockstep / sliced in one packed level-domain pass
    int layers;              // live layers: l < layers is decided and counted
};

template <typename T>
__device__ __forceinline__ LinkDecide<T> link_decide_for(const ModemParams<T>& mp, const cx<T>* s_table, const float4* s_tab4,
                                                         const unsigned long long* s_grid, int layers) {
    LinkDecide<T> w{mp,
                    s_table,
                    s_tab4,
                    s_grid,
                    QamPack{},
                    layers >= 4 ? 0xFFFFFFFFu : ((1u << (8 * layers)) - 1u),
                    sizeof(T) == 4 && mp.method == MCLE_DEMOD_MINDIST && (mp.M <= 8 || mp.grid.G > 0),
                    sizeof(T) == 4 && mp.method == MCLE_DEMOD_QAM_SLICER,
                    layers};
    if constexpr (sizeof(T) == 4) {
        if (w.packed) w.qp = qam_pack(mp);
    }
    return w;
}

// The decisions of one column and their errors.  N: the capacity of est / tx; entries l >= w.layers carry est = 0, tx = 0 and
// are not counted.  Three forms: the packed level-domain slicer (N <= 4: unused lanes at zero and masked), the lockstep search
// through the certificate (plain or candidate grid), demod_one per layer.
template <typename T, int N>
__device__ __forceinline__ void link_decide(const LinkDecide<T>& w, const cx<T> (&est)[N], const int (&tx)[N], unsigned& se,
                                            unsigned& be) {
    if constexpr (sizeof(T) == 4 && N <= 4) {
        if (w.packed) {   // the column's decisions in one packed level-domain slice (qam_pack.hpp)
            f4q er = {0.f, 0.f, 0.f, 0.f}, ei = {0.f, 0.f, 0.f, 0.f};
            uint32_t sent = 0u;
#pragma unroll
            for (int l = 0; l < N; ++l) {
                er[l] = est[l].x;
                ei[l] = est[l].y;
                sent |= (uint32_t)tx[l] << (8 * l);
            }
            qam_count4((qam_levels4(er, ei, w.qp) ^ labels_to_levels(sent, w.qp)) & w.layer_mask, w.qp, se, be);
            return;
        }
    }
    int dec[N];
    bool done = false;
    if constexpr (sizeof(T) == 4) {
        if (w.lockstep) {   // the layers searched in lockstep (same decisions as demod_one)
            if (w.mp.M <= 8) demod_multi_cert(w.mp, est, dec, [&](int (&d_)[N]) { demod_mindist_multi<N>(w.s_tab4, w.mp.M, est, d_); });
            else demod_multi_cert(w.mp, est, dec, [&](int (&d_)[N]) { demod_grid4_multi<N>(w.s_tab4, w.s_grid, w.mp.grid, w.mp.M, est, d_); });
            done = true;
        }
    }
    if (!done) {
#pragma unroll
        for (int l = 0; l < N; ++l) dec[l] = l < w.layers ? demod_one(w.mp, w.s_table, w.s_grid, est[l]) : 0;
    }
#pragma unroll
    for (int l = 0; l < N; ++l)
        if (l < w.layers) {
            const unsigned xr = (unsigned)(tx[l] ^ dec[l]);
            se += (xr != 0u);
            be += __popc(xr);
        }
}

// The walk's opening: the complex128 Box-Muller tables, the constellation, the candidate grid and (complex64, where the kernel
// has one) the lockstep table, into the LDS arrays the KERNEL declares -- its LDS layout and size stay its own.  Before the
// kernel's first __syncthreads().
template <typename T>
__device__ __forceinline__ void link_prologue(const ModemParams<T>& mp, cx<T>* s_table, float4* s_tab4, unsigned long long* s_grid,
                                              double* s_bm) {
    if constexpr (sizeof(T) == 8) bm_tables_to_lds(s_bm, (int)threadIdx.x, (int)blockDim.x);
    load_table(mp, s_table);
    load_grid(mp, s_grid);
    if constexpr (sizeof(T) == 4) {
        if (s_tab4) load_tab4(mp, s_tab4);
    }
}

// The per-realization tail: the wavefront's error counts summed, lane 0 books them (totals.hpp).
__device__ __forceinline__ void link_account(WgTotals& totals, unsigned se, unsigned be, bool skipped, uint64_t rl, int lane,
                                             uint32_t* __restrict__ sym_out, uint32_t* __restrict__ bit_out) {
    se = wave_sum_u32(se);
    be = wave_sum_u32(be);
    if (lane == 0) wg_account(totals, se, be, skipped, rl, sym_out, bit_out);
}

}  // namespace mcle
