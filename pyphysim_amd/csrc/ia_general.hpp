// ia_general.hpp -- what kernels_ia_general.hip offers the other translation units: the argument rules of
// mcle_ia_general_cfg and the launch of the general-geometry IA solver, as mcle_ia_solve_general runs them.  The fused link
// (pipeline_ia_general.hip) goes through these two, so it refuses what the operator refuses, in the operator's words, and its
// solutions come from the operator's own compiled kernel.
#pragma once
#include "common.hpp"

namespace mcle {

constexpr int kIagUsers = 4;        // KM of ia_general_body.hpp

// padded matrices are D x D: 4 while max(Nr, Nt) <= 4, else 6 (the solver's two instantiations)
inline int ia_general_capacity(const mcle_ia_general_cfg* cfg) { return (cfg->nr > 4 || cfg->nt > 4) ? 6 : 4; }

// the envelope of mcle_ia_general_cfg (include/mcle.h); have_start: a start for MCLE_IA_INIT_GIVEN is at hand
int ia_general_check(const mcle_ia_general_cfg* cfg, bool have_start);

// the solver's launch on checked arguments and a bound context (batch >= 1); sets last_kernel to "ia_general<D> ..."
int ia_general_launch(mcle_ctx* ctx, const mcle_ia_general_cfg* cfg, const void* d_bigH, const void* d_F_init, void* d_F,
                      void* d_U, double* d_sinr, double* d_capacity, uint32_t* d_iterations, int32_t* d_ns,
                      uint32_t* d_skipped, double* d_every_capacity, size_t batch);

}  // namespace mcle
