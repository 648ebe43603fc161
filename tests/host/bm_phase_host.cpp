// Host build of csrc/bm_f64.hpp for tests/test_bm_phase_cpu.py: the complex128 noise sample in two phases (bm_sample_fetch /
// bm_sample_finish, the form the headline kernel's pipelined draw uses) against the one-phase sample -- the expression of
// csrc/philox.hpp's cn_from_words (global tables) and cn_from_words_lds_pairs (a pair-table copy) written out from the header's
// own one-phase functions, which philox.hpp itself cannot be compiled for the host to provide.
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

using namespace mcle;

// the copy bm_tables_to_lds_pairs makes: [kBmLogQ | kBmTrig | kBmTheta], 16-byte aligned
alignas(16) static double g_pairs[(kBmLdsDoubles + 1) & ~1];
static const double* pairs() {
    static bool done = false;
    if (!done) {
        for (int i = 0; i < kBmLogLen; ++i) g_pairs[i] = kBmLogQ[i];
        for (int i = 0; i < kBmTrigLen; ++i) g_pairs[kBmLogLen + i] = kBmTrig[i];
        for (int i = 0; i < kBmThetaLen; ++i) g_pairs[kBmLogLen + kBmTrigLen + i] = kBmTheta[i];
        done = true;
    }
    return g_pairs;
}

// cn_from_words(x0, x1, sigma)
static void one_phase(uint32_t x0, uint32_t x1, double sigma, double* z) {
    const double rad = sigma * bm_sqrt(bm_neg_log_q(x0));
    double s, c;
    bm_sincos(x1, c, s);
    z[0] = rad * c;
    z[1] = rad * s;
}
// cn_from_words_lds_pairs(x0, x1, sigma, s_bm)
static void one_phase_pairs(uint32_t x0, uint32_t x1, double sigma, const double* s_bm, double* z) {
    const double rad = sigma * bm_sqrt(bm_neg_log_q<true>(x0, s_bm));
    double s, c;
    bm_sincos<true>(x1, c, s, s_bm + kBmLogLen + kBmTrigLen, s_bm + kBmLogLen);
    z[0] = rad * c;
    z[1] = rad * s;
}
// cn_finish(cn_fetch_lds_pairs(x0, x1, s_bm), sigma)
static void two_phase(uint32_t x0, uint32_t x1, double sigma, const double* s_bm, double* z) {
    const BmFetched t = bm_sample_fetch(x0, x1, s_bm, s_bm + kBmLogLen + kBmTrigLen, s_bm + kBmLogLen);
    bm_sample_finish(t, sigma, z[0], z[1]);
}

extern "C" {
// pairs (x0[i], x1[i]) on which the two-phase sample differs from either one-phase form in either component, as 64-bit patterns;
// the index of the first one, if any, to *first_bad
size_t bm_phase_mismatches(const uint32_t* x0, const uint32_t* x1, size_t n, double sigma, size_t* first_bad) {
    const double* s_bm = pairs();
    size_t bad = 0;
    for (size_t i = 0; i < n; ++i) {
        double a[2], b[2], c[2];
        one_phase(x0[i], x1[i], sigma, a);
        one_phase_pairs(x0[i], x1[i], sigma, s_bm, b);
        two_phase(x0[i], x1[i], sigma, s_bm, c);
        if ((std::memcmp(a, c, sizeof a) != 0 || std::memcmp(b, c, sizeof b) != 0) && bad++ == 0) *first_bad = i;
    }
    return bad;
}
void bm_phase_one_batch(const uint32_t* x0, const uint32_t* x1, size_t n, double sigma, double* out) {
    for (size_t i = 0; i < n; ++i) one_phase(x0[i], x1[i], sigma, out + 2 * i);
}
void bm_phase_two_batch(const uint32_t* x0, const uint32_t* x1, size_t n, double sigma, double* out) {
    const double* s_bm = pairs();
    for (size_t i = 0; i < n; ++i) two_phase(x0[i], x1[i], sigma, s_bm, out + 2 * i);
}
}
