// Host build of csrc/bm_f64.hpp for tests/test_bm_logq_cpu.py and tests/test_gpu_bm_logq.py: bm_neg_log (the witness) and
// bm_neg_log_q (the form the pipelines draw with) from the same header the device compiles, the two bit-field builtins of the
// latter taking the header's plain C++ fallbacks (MCLE_BM_ALIGNBIT, MCLE_BM_SBFE).
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#define MCLE_BM_TABLE static const
#define MCLE_BM_FN static inline
#define MCLE_BM_RSQ(a) ((double)(1.0f / std::sqrt((float)(a))))
#define MCLE_BM_FMA(a, b, c) std::fma(a, b, c)
#define MCLE_BM_RINT(a) std::nearbyint(a)
#include "../../pyphysim_amd/csrc/bm_f64.hpp"

extern "C" {
void bm_neg_log_batch(const uint32_t* x0, double* out, size_t n) {
    for (size_t i = 0; i < n; ++i) out[i] = mcle::bm_neg_log(x0[i]);
}
void bm_neg_log_q_batch(const uint32_t* x0, double* out, size_t n) {
    for (size_t i = 0; i < n; ++i) out[i] = mcle::bm_neg_log_q(x0[i]);
}
// words on which the two forms differ as 64-bit patterns; the first one, if any, to *first_bad
size_t bm_neg_log_q_mismatches(const uint32_t* x0, size_t n, uint32_t* first_bad) {
    size_t bad = 0;
    for (size_t i = 0; i < n; ++i) {
        const double a = mcle::bm_neg_log(x0[i]), b = mcle::bm_neg_log_q(x0[i]);
        if (std::memcmp(&a, &b, sizeof a) != 0 && bad++ == 0) *first_bad = x0[i];
    }
    return bad;
}
// the same over the whole range [lo, hi) without an array of words
size_t bm_neg_log_q_mismatches_range(uint64_t lo, uint64_t hi, uint32_t* first_bad) {
    size_t bad = 0;
    for (uint64_t w = lo; w < hi; ++w) {
        const double a = mcle::bm_neg_log((uint32_t)w), b = mcle::bm_neg_log_q((uint32_t)w);
        if (std::memcmp(&a, &b, sizeof a) != 0 && bad++ == 0) *first_bad = (uint32_t)w;
    }
    return bad;
}
const double* bm_log_table() { return mcle::kBmLog; }
const double* bm_logq_table() { return mcle::kBmLogQ; }
}
