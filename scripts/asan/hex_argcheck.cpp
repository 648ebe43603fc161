// Stand-alone host program for the sanitizer build of the hexagonal-cell system-level entry points: every argument rule of
// mcle_hex_gains and mcle_run_hex_drops is driven with a context built on the host, and the corners of the envelope (19 cells
// with wrap around: all 61 slots of the position tables and the last slot of pos_start are read and written; 256 users; 256
// bins; 8 interferer columns) go through the host-side set-up up to the empty-range return.  No device is opened.  Built by
// `make -C pyphysim_amd/csrc asan-hex-argcheck SAN=...` ("Host sanitizer runs"), exits non-zero on the first
// unexpected return code.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../pyphysim_amd/csrc/common.hpp"

static int failures = 0;
#define EXPECT(call, want_ok, word)                                                                        \
    do {                                                                                                   \
        const int rc_ = (call);                                                                            \
        const char* msg_ = mcle_last_error();                                                              \
        const bool ok_ = (want_ok) ? rc_ == MCLE_OK : (rc_ == MCLE_E_INVAL && std::strstr(msg_, word));    \
        if (!ok_) {                                                                                        \
            std::printf("FAIL %s:%d rc=%d msg=%s\n", __FILE__, __LINE__, rc_, msg_);                       \
            ++failures;                                                                                    \
        }                                                                                                  \
    } while (0)

// a cluster of K cells with made-up centres (the rules look at the tables' shape, not at the geometry); with wrap the lists of
// the 19-cell cluster: cell 1 alone, cells 2 .. 7 with two copies, cells 8 .. 19 with three and two in turn -- 61 positions
static mcle_hex_cfg make_cfg(int K, bool wrap) {
    mcle_hex_cfg c;
    std::memset(&c, 0, sizeof(c));
    c.num_cells = K, c.users_per_cell = 2, c.model = MCLE_HEX_PL_GENERAL, c.wrap_around = wrap, c.n_ext = 1, c.hist_bins = 16;
    c.cell_radius = 1.0, c.min_dist_ratio = 0.1, c.pl_n = 3.76, c.pl_C = 128.1, c.dist_scale = 1.0;
    c.tx_power = 0.1, c.noise_power = 2e-14, c.ext_power = 1e-9, c.hist_lo_dB = -10.0, c.hist_step_dB = 2.5;
    c.external_radius = 5.0;
    int n = 0;
    for (int i = 0; i < K; ++i) {
        c.pos_start[i] = n;
        const int len = !wrap || i == 0 ? 1 : i < 7 ? 3 : (i % 2 ? 4 : 3);
        for (int j = 0; j < len; ++j, ++n) c.pos_x[n] = 1.5 * i + 10.0 * j, c.pos_y[n] = 0.5 * i;
    }
    c.pos_start[K] = c.n_pos = n;
    return c;
}

static int gains(mcle_ctx* ctx, int dtype, const mcle_hex_cfg* c, size_t n) {
    return mcle_hex_gains(ctx, dtype, c, nullptr, n, nullptr, nullptr, nullptr, nullptr);
}
static int run(mcle_ctx* ctx, int dtype, const mcle_hex_cfg* c, uint64_t count) {
    return mcle_run_hex_drops(ctx, dtype, c, 1, 0, count, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                              nullptr);
}
// both entry points refuse the configuration with a message that holds `word`
static void both(const mcle_hex_cfg& c, mcle_ctx* ctx, const char* word) {
    EXPECT(gains(ctx, MCLE_F64, &c, 4), false, word);
    EXPECT(run(ctx, MCLE_F32, &c, 4), false, word);
}
static void drops(const mcle_hex_cfg& c, mcle_ctx* ctx, const char* word) { EXPECT(run(ctx, MCLE_F64, &c, 4), false, word); }

int main() {
    mcle_ctx ctx;                               // host-side bookkeeping only
    const mcle_hex_cfg good = make_cfg(7, false);
    mcle_hex_cfg c = good;
    both(good, nullptr, "null context");
    EXPECT(gains(&ctx, 7, &good, 4), false, "dtype");
    EXPECT(gains(&ctx, MCLE_F64, nullptr, 4), false, "null hex cfg");
    EXPECT(run(&ctx, MCLE_F64, nullptr, 4), false, "null hex cfg");
    EXPECT(gains(&ctx, MCLE_F64, &good, 4), false, "null d_points");
    EXPECT(gains(&ctx, MCLE_F64, &good, (size_t)1 << 31), false, "2^31-1");
    EXPECT(run(&ctx, MCLE_F64, &good, 1ull << 31), false, "2^31-1");
    c = good, c.num_cells = 0, both(c, &ctx, "num_cells");
    c = good, c.num_cells = 20, both(c, &ctx, "num_cells");
    c = good, c.model = 2, both(c, &ctx, "model");
    c = good, c.model = -1, both(c, &ctx, "model");
    c = good, c.wrap_around = 2, both(c, &ctx, "wrap_around must be");
    c = good, c.wrap_around = 1, both(c, &ctx, "wrap_around needs");
    c = good, c.n_ext = -1, both(c, &ctx, "n_ext");
    c = good, c.n_ext = 9, both(c, &ctx, "n_ext");
    c = good, c.cell_radius = 0.0, both(c, &ctx, "cell_radius");
    c = good, c.cell_radius = std::nan(""), both(c, &ctx, "cell_radius");
    c = good, c.pl_n = 0.0, both(c, &ctx, "pl_n");
    c = good, c.pl_C = HUGE_VAL, both(c, &ctx, "pl_C");
    c = good, c.dist_scale = 0.0, both(c, &ctx, "dist_scale");
    c = good, c.tx_power = 0.0, both(c, &ctx, "tx_power");
    c = good, c.noise_power = -1.0, both(c, &ctx, "noise_power");
    c = good, c.ext_power = -1.0, both(c, &ctx, "ext_power");
    c = good, c.n_pos = 6, both(c, &ctx, "n_pos");
    c = good, c.n_pos = 65, both(c, &ctx, "n_pos");
    c = good, c.pos_start[0] = 1, both(c, &ctx, "pos_start must run");
    c = good, c.n_pos = 8, both(c, &ctx, "pos_start must run");
    c = good, c.pos_start[3] = 4, both(c, &ctx, "pos_start: cell 3");
    c = good, c.pos_start[3] = 2, both(c, &ctx, "pos_start: cell 3");
    c = good, c.pos_x[6] = HUGE_VAL, both(c, &ctx, "pos_x / pos_y");
    c = good, c.pos_y[0] = std::nan(""), both(c, &ctx, "pos_x / pos_y");
    c = good, c.external_radius = 0.0, both(c, &ctx, "external_radius");
    c = good, c.centre_x = HUGE_VAL, both(c, &ctx, "centre_x");
    c = make_cfg(19, true), c.pos_start[5] += 2, c.pos_start[6] += 2, both(c, &ctx, "pos_start: cell 5");      // five positions
    c = good, c.noise_power = 1e-40;            // no normal f32 number: refused in f32 only
    EXPECT(gains(&ctx, MCLE_F32, &c, 4), false, "normal f32");
    EXPECT(gains(&ctx, MCLE_F64, &c, 0), true, "");
    c = good, c.tx_power = 1e39;
    EXPECT(run(&ctx, MCLE_F32, &c, 4), false, "normal f32");
    c = good, c.ext_power = 1e-40;
    EXPECT(run(&ctx, MCLE_F32, &c, 4), false, "ext_power must be 0 or");
    c = good, c.ext_power = 0.0;
    EXPECT(run(&ctx, MCLE_F32, &c, 0), true, "");
    // the drops' own rules; the operator ignores these fields
    c = good, c.users_per_cell = 0, drops(c, &ctx, "users_per_cell");
    EXPECT(gains(&ctx, MCLE_F64, &c, 0), true, "");
    c = good, c.users_per_cell = 37, drops(c, &ctx, "users_per_cell");              // 7 x 37 = 259
    c = good, c.users_per_cell = 0x7fffffff, drops(c, &ctx, "users_per_cell");
    c = good, c.min_dist_ratio = -0.1, drops(c, &ctx, "min_dist_ratio");
    c = good, c.min_dist_ratio = 0.71, drops(c, &ctx, "min_dist_ratio");
    c = good, c.min_dist_ratio = std::nan(""), drops(c, &ctx, "min_dist_ratio");
    c = good, c.hist_bins = -1, drops(c, &ctx, "hist_bins");
    c = good, c.hist_bins = 257, drops(c, &ctx, "hist_bins");
    c = good, c.hist_step_dB = 0.0, drops(c, &ctx, "hist_step_dB");
    c = good, c.hist_bins = 0, c.hist_lo_dB = HUGE_VAL, drops(c, &ctx, "hist_lo_dB");
    c = good, c.model = MCLE_HEX_PL_NONE, c.pl_n = 0.0, c.dist_scale = -1.0;        // the model's constants are not looked at
    EXPECT(run(&ctx, MCLE_F64, &c, 0), true, "");
    // the corners of the envelope through the whole host-side set-up: an empty range returns before the device is touched
    for (int K = 1; K <= 19; ++K)
        for (int wrap = 0; wrap <= (K == 19 ? 1 : 0); ++wrap)
            for (int dtype : {MCLE_F32, MCLE_F64}) {
                c = make_cfg(K, wrap != 0);
                c.users_per_cell = 256 / K, c.hist_bins = 256, c.n_ext = 8, c.min_dist_ratio = 0.7;
                if (wrap && c.n_pos != 61) {
                    std::printf("FAIL: the wrapped tables hold %d positions\n", c.n_pos);
                    ++failures;
                }
                EXPECT(gains(&ctx, dtype, &c, 0), true, "");
                EXPECT(run(&ctx, dtype, &c, 0), true, "");
                c.min_dist_ratio = 0.0, c.hist_bins = 0, c.n_ext = 0, c.users_per_cell = 1;
                EXPECT(run(&ctx, dtype, &c, 0), true, "");
            }
    c = make_cfg(19, true);                                                         // all 64 slots: four cells alone, fifteen with four
    for (int i = 0, n = 0; i <= 19; n += i < 4 ? 1 : 4, ++i) c.pos_start[i] = n;
    c.n_pos = c.pos_start[19];
    for (int i = 61; i < 64; ++i) c.pos_x[i] = c.pos_y[i] = (double)i;
    EXPECT(c.n_pos == 64 ? run(&ctx, MCLE_F64, &c, 0) : MCLE_E_INVAL, true, "");
    char name[64] = "x";
    mcle_ctx_last_kernel(&ctx, name, sizeof(name));
    if (name[0] != 0) {
        std::printf("FAIL: a refused or empty call left the kernel tag '%s'\n", name);
        ++failures;
    }
    std::printf("hex argument checks: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
