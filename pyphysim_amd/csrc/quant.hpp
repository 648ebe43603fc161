// quant.hpp -- what kernels_quant.hip offers the other translation units (host side)
#pragma once
#include "common.hpp"

namespace mcle {

// the envelope of mcle_quant_cfg (MCLE_E_INVAL with a message that names the argument); needs no context
int quant_check_cfg(int dtype, const mcle_quant_cfg* cfg);

// The search of mcle_quantize_links on the channels mcle_run_ia draws (K = 3, 2 x 2; realizations first .. first + count - 1 of
// `seed`): d_index [count][3][3], d_dist [count][3][3] (may be NULL).  One launch on the context's stream.
int launch_quantize_drawn(mcle_ctx* ctx, int dtype, const mcle_quant_cfg* cfg, const void* d_codebook, uint64_t seed,
                          uint64_t first, uint64_t count, int32_t* d_index, double* d_dist);

}  // namespace mcle
