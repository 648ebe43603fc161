// pilot_block.hpp -- what the two links with pilot-estimated channel state share (pipeline_mimo_pilot.hip: up to 4 x 4, one thread
// per realization; pipeline_mimo_large_pilot.hip: up to 8 x 16, one lane per receive row): on the host the rules of
// mcle_mimo_pilot_cfg and the set-up fields with the fixed pilots' inverse Gram matrix; on the device the Cholesky of the drawn
// pilots' Gram matrix and the row solve of the LS estimate.  Each kernel keeps its own walk over the pilot block, its
// H = alpha L W, the MMSE product with B and the err / pow sums: they differ in who owns what.
#pragma once
#include <cmath>
#include <complex>
#include <vector>

#include "common.hpp"
#include "pipe_common.hpp"

namespace mcle {

constexpr int kPilotMaxPilots = 256;
// a Gram pivot at or below this share of the Gram matrix's trace counts as singular (host and device alike)
constexpr double kGramPivotFloor = 1e-12;

// What a pilot set-up kernel is launched with, for an envelope of MAXNT transmit antennas
template <int MAXNT> struct PilotSetup {
    int P, half;                                // half = ceil(P / 2)
    int random_pilots, mmse_est, gram_ok;
    double amp, sigma, alpha, filter_nv;        // sqrt(pilot_power), sqrt(noise_var)
    double2 ginv[MAXNT * MAXNT];                // fixed pilots: (s s^H)^-1, entry [a][b] at a * MAXNT + b
};

// The rules of mcle_mimo_pilot_cfg behind the entry point's own antenna-count rule (the two envelopes word that one differently)
inline int check_pilot_cfg(const mcle_mimo_pilot_cfg* cfg, const double* d_pilots, const double* d_mmse_matrix, uint64_t count) {
    const int nt = cfg->nt, P = cfg->n_pilots;
    MCLE_REQUIRE(P >= nt && P <= kPilotMaxPilots, "n_pilots must be in [nt, %d] (got %d pilots, nt %d)", kPilotMaxPilots, P, nt);
    MCLE_REQUIRE(cfg->n_symbols >= 1, "n_symbols must be positive");
    MCLE_REQUIRE(cfg->estimator == 0 || cfg->estimator == 1, "estimator must be 0 (LS) or 1 (MMSE) (got %d)", cfg->estimator);
    MCLE_REQUIRE(cfg->random_pilots == 0 || cfg->random_pilots == 1, "random_pilots must be 0 or 1 (got %d)", cfg->random_pilots);
    MCLE_REQUIRE(cfg->mmse_filter == 0 || cfg->mmse_filter == 1, "mmse_filter must be 0 or 1 (got %d)", cfg->mmse_filter);
    MCLE_REQUIRE(std::isfinite(cfg->noise_var) && cfg->noise_var >= 0.0, "Noise variance must be a non-negative value.");
    MCLE_REQUIRE(std::isfinite(cfg->pilot_power) && cfg->pilot_power > 0.0, "pilot_power must be finite and positive");
    MCLE_REQUIRE(std::isfinite(cfg->alpha), "alpha must be finite");
    MCLE_REQUIRE(cfg->random_pilots || d_pilots != nullptr, "null d_pilots with random_pilots = 0");
    MCLE_REQUIRE(cfg->estimator == 0 || nt == 1, "the MMSE estimator needs nt = 1 (got %d)", nt);
    MCLE_REQUIRE(cfg->estimator == 0 || d_mmse_matrix != nullptr, "the MMSE estimator needs d_mmse_matrix (from a covariance)");
    return check_link_draws((uint64_t)cfg->nr, cfg->n_symbols, count);
}

// (s s^H)^-1 of the fixed pilots s [nt][P] by Gauss-Jordan with partial pivoting, complex128, entry [a][b] at ginv[a * MAXNT + b];
// false: numerically singular
template <int MAXNT>
inline bool pilot_gram_inverse(const std::complex<double>* s, int nt, int P, double2* ginv) {
    typedef std::complex<double> zc;
    zc g[MAXNT][MAXNT], inv[MAXNT][MAXNT];
    double tr = 0.0;
    for (int a = 0; a < nt; ++a)
        for (int b = 0; b < nt; ++b) {
            zc acc(0.0, 0.0);
            for (int p = 0; p < P; ++p) acc += s[a * P + p] * std::conj(s[b * P + p]);
            g[a][b] = acc;
            inv[a][b] = a == b ? zc(1.0, 0.0) : zc(0.0, 0.0);
            if (a == b) tr += acc.real();
        }
    if (!std::isfinite(tr) || !(tr > 0.0)) return false;
    for (int k = 0; k < nt; ++k) {
        int piv = k;
        for (int i = k + 1; i < nt; ++i)
            if (std::abs(g[i][k]) > std::abs(g[piv][k])) piv = i;
        if (!(std::abs(g[piv][k]) > kGramPivotFloor * tr)) return false;
        for (int j = 0; j < nt; ++j) {
            std::swap(g[k][j], g[piv][j]);
            std::swap(inv[k][j], inv[piv][j]);
        }
        const zc d = 1.0 / g[k][k];
        for (int j = 0; j < nt; ++j) {
            g[k][j] *= d;
            inv[k][j] *= d;
        }
        for (int i = 0; i < nt; ++i) {
            if (i == k) continue;
            const zc f = g[i][k];
            for (int j = 0; j < nt; ++j) {
                g[i][j] -= f * g[k][j];
                inv[i][j] -= f * inv[k][j];
            }
        }
    }
    for (int a = 0; a < nt; ++a)
        for (int b = 0; b < nt; ++b) ginv[a * MAXNT + b] = make_double2(inv[a][b].real(), inv[a][b].imag());
    return true;
}

// The last steps before the launches of a checked configuration with count > 0: the context is bound and the set-up fields are
// filled; the fixed block is downloaded and its Gram matrix inverted here, once per call (gram_ok = 0: singular, every realization
// is skipped)
template <int MAXNT>
inline int pilot_setup_fill(mcle_ctx* ctx, const mcle_mimo_pilot_cfg* cfg, const double* d_pilots, const mcle_counters* d_counters,
                            PilotSetup<MAXNT>& p) {
    MCLE_REQUIRE(d_counters != nullptr, "null d_counters");
    if (const int rc = ctx->bind()) return rc;
    const int nt = cfg->nt, P = cfg->n_pilots;
    p = PilotSetup<MAXNT>{};
    p.P = P, p.half = (P + 1) / 2;
    p.random_pilots = cfg->random_pilots, p.mmse_est = cfg->estimator, p.gram_ok = 1;
    p.amp = std::sqrt(cfg->pilot_power), p.sigma = std::sqrt(cfg->noise_var), p.alpha = cfg->alpha;
    p.filter_nv = cfg->mmse_filter ? cfg->noise_var : 0.0;
    if (!cfg->random_pilots) {
        std::vector<std::complex<double>> s((size_t)nt * P);
        MCLE_HIP(hipMemcpyAsync(s.data(), d_pilots, s.size() * sizeof(s[0]), hipMemcpyDeviceToHost, ctx->stream));
        MCLE_HIP(hipStreamSynchronize(ctx->stream));
        p.gram_ok = pilot_gram_inverse<MAXNT>(s.data(), nt, P, p.ginv) ? 1 : 0;
    }
    return MCLE_OK;
}

// a - b conj(c) and a - b c with the fusion of every product spelled out.  Under -ffp-contract=fast the compiler chooses per call
// site which of the two products of a component is rounded, and the two kernels below have to round alike -- and as before this
// code was shared (tests/test_gpu_large_walk_parent.py compares err bit for bit).  An explicit fused multiply-add leaves it nothing
// to choose (modem.hpp: dist2).
__device__ __forceinline__ double2 csub_mulc(double2 a, double2 b, double2 c) {
    a.x -= __builtin_fma(b.x, c.x, b.y * c.y);
    a.y -= __builtin_fma(b.y, c.x, -(b.x * c.y));
    return a;
}
__device__ __forceinline__ double2 csub_mul(double2 a, double2 b, double2 c) {
    a.x -= __builtin_fma(b.x, c.x, -(b.y * c.y));
    a.y -= __builtin_fma(b.y, c.x, b.x * c.y);
    return a;
}

// Gram = C C^H of the drawn pilots' Gram matrix s s^H (lower triangle in Gm), C lower triangular, in place; invd[c] = 1 / C[c][c].
// False: a pivot at or below kGramPivotFloor of the trace.
template <int NT>
__device__ __forceinline__ bool pilot_gram_factor(double2 (&Gm)[NT][NT], double (&invd)[NT]) {
    double tr = 0.0;
#pragma unroll
    for (int a = 0; a < NT; ++a) tr += Gm[a][a].x;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < NT; ++c) {
#pragma unroll
        for (int i = c; i < NT; ++i) {
            double2 a = Gm[i][c];
#pragma unroll
            for (int k = 0; k < c; ++k) a = csub_mulc(a, Gm[i][k], Gm[c][k]);
            if (i == c) {
                ok = ok && (a.x > kGramPivotFloor * tr);
                Gm[c][c] = mk<double>(sqrt(a.x), 0.0);
                invd[c] = 1.0 / Gm[c][c].x;
            } else {
                Gm[i][c] = cscale(a, invd[c]);
            }
        }
    }
    return ok;
}

// One row x of H^: x C C^H = R, y C^H = R forwards, x C = y backwards
template <int NT>
__device__ __forceinline__ void pilot_row_solve(const double2 (&C)[NT][NT], const double (&invd)[NT], const double2 (&R)[NT],
                                                double2 (&x)[NT]) {
#pragma unroll
    for (int c = 0; c < NT; ++c) {
        double2 v = R[c];
#pragma unroll
        for (int k = 0; k < c; ++k) v = csub_mulc(v, x[k], C[c][k]);
        x[c] = cscale(v, invd[c]);
    }
#pragma unroll
    for (int c = NT - 1; c >= 0; --c) {
        double2 v = x[c];
#pragma unroll
        for (int k = c + 1; k < NT; ++k) v = csub_mul(v, x[k], C[k][c]);
        x[c] = cscale(v, invd[c]);
    }
}

}  // namespace mcle
