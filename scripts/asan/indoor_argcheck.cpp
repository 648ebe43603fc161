// Stand-alone host program for the sanitizer build of the indoor system-level entry points: every argument rule of
// mcle_indoor_sinr and mcle_run_indoor_drops is driven with a context built on the host, and the corners of the envelope
// (16 rooms per side: the last slot of the room-centre arrays is written and read) go through the host-side set-up up to the
// empty-range return.  No device is opened.  Built by `make -C pyphysim_amd/csrc asan-indoor-argcheck SAN=...` (INTEGRATION.md,
// "Host sanitizer runs"), exits non-zero on the first unexpected return code.
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

static mcle_indoor_cfg good_cfg() {
    mcle_indoor_cfg c;
    std::memset(&c, 0, sizeof(c));
    c.rooms_per_side = 12, c.ap_decimation = 2, c.model = MCLE_INDOOR_PL_METIS_PS7, c.assoc = 1, c.n_users = 100, c.hist_bins = 16;
    c.side_length = 10.0, c.wall_loss_dB = 5.0, c.pl_n = 3.76, c.pl_C = 128.1, c.dist_scale = 1e-3, c.fc_MHz = 900.0;
    c.tx_power = 0.1, c.noise_power = 2e-14, c.hist_lo_dB = -10.0, c.hist_step_dB = 2.5;
    return c;
}

// both entry points refuse the configuration with a message that holds `word`
static void both(const mcle_indoor_cfg& c, mcle_ctx* ctx, const char* word) {
    EXPECT(mcle_indoor_sinr(ctx, MCLE_F64, &c, nullptr, 4, nullptr, nullptr), false, word);
    EXPECT(mcle_run_indoor_drops(ctx, MCLE_F32, &c, 1, 0, 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                 nullptr, nullptr),
           false, word);
}
static void drops(const mcle_indoor_cfg& c, mcle_ctx* ctx, const char* word) {
    EXPECT(mcle_run_indoor_drops(ctx, MCLE_F64, &c, 1, 0, 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                 nullptr, nullptr),
           false, word);
}

int main() {
    mcle_ctx ctx;                               // host-side bookkeeping only
    const mcle_indoor_cfg good = good_cfg();
    mcle_indoor_cfg c = good;
    both(good, nullptr, "null context");
    EXPECT(mcle_indoor_sinr(&ctx, 7, &good, nullptr, 4, nullptr, nullptr), false, "dtype");
    EXPECT(mcle_indoor_sinr(&ctx, MCLE_F64, nullptr, nullptr, 4, nullptr, nullptr), false, "null indoor cfg");
    EXPECT(mcle_indoor_sinr(&ctx, MCLE_F64, &good, nullptr, 4, nullptr, nullptr), false, "null d_points");
    EXPECT(mcle_indoor_sinr(&ctx, MCLE_F64, &good, nullptr, (size_t)1 << 31, nullptr, nullptr), false, "2^31-1");
    c = good, c.rooms_per_side = 0, both(c, &ctx, "rooms_per_side");
    c = good, c.rooms_per_side = 17, both(c, &ctx, "rooms_per_side");
    c = good, c.ap_decimation = 3, both(c, &ctx, "ap_decimation");
    c = good, c.rooms_per_side = 1, c.ap_decimation = 9, both(c, &ctx, "without an access point");
    c = good, c.model = 3, both(c, &ctx, "model");
    c = good, c.assoc = 2, both(c, &ctx, "assoc");
    c = good, c.side_length = 0.0, both(c, &ctx, "side_length");
    c = good, c.side_length = std::nan(""), both(c, &ctx, "side_length");
    c = good, c.wall_loss_dB = -1.0, both(c, &ctx, "wall_loss_dB");
    c = good, c.model = MCLE_INDOOR_PL_GENERAL, c.pl_n = 0.0, both(c, &ctx, "pl_n");
    c = good, c.model = MCLE_INDOOR_PL_GENERAL, c.pl_C = HUGE_VAL, both(c, &ctx, "pl_C");
    c = good, c.model = MCLE_INDOOR_PL_GENERAL, c.dist_scale = 0.0, both(c, &ctx, "dist_scale");
    c = good, c.fc_MHz = 0.0, both(c, &ctx, "fc_MHz");
    c = good, c.tx_power = 0.0, both(c, &ctx, "tx_power");
    c = good, c.noise_power = -1.0, both(c, &ctx, "noise_power");
    c = good, c.noise_power = 1e-40;            // no normal f32 number: refused in f32 only
    EXPECT(mcle_indoor_sinr(&ctx, MCLE_F32, &c, nullptr, 4, nullptr, nullptr), false, "normal f32");
    EXPECT(mcle_indoor_sinr(&ctx, MCLE_F64, &c, nullptr, 0, nullptr, nullptr), true, "");
    c = good, c.tx_power = 1e39;
    EXPECT(mcle_indoor_sinr(&ctx, MCLE_F32, &c, nullptr, 4, nullptr, nullptr), false, "normal f32");
    c = good, c.active = 1;
    EXPECT(mcle_indoor_sinr(&ctx, MCLE_F64, &c, nullptr, 4, nullptr, nullptr), false, "active must be 0");
    c = good, c.active = 2, drops(c, &ctx, "active");
    c = good, c.n_users = 0, drops(c, &ctx, "n_users");
    c = good, c.n_users = 257, drops(c, &ctx, "n_users");
    c = good, c.hist_bins = 257, drops(c, &ctx, "hist_bins");
    c = good, c.hist_step_dB = 0.0, drops(c, &ctx, "hist_step_dB");
    c = good, c.hist_bins = 0, c.hist_lo_dB = HUGE_VAL, drops(c, &ctx, "hist_lo_dB");
    EXPECT(mcle_run_indoor_drops(&ctx, MCLE_F64, &good, 1, 0, 1ull << 31, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                 nullptr, nullptr, nullptr, nullptr),
           false, "2^31-1");
    // the corners of the envelope through the whole host-side set-up: an empty range returns before the device is touched
    for (int n = 1; n <= 16; ++n)
        for (int dec : {1, 2, 4, 9})
            for (double L : {7.0, 7.5, 10.0}) {
                c = good, c.rooms_per_side = n, c.ap_decimation = dec, c.side_length = L, c.n_users = 256, c.hist_bins = 256;
                if (n == 1 && dec != 1) continue;
                EXPECT(mcle_indoor_sinr(&ctx, MCLE_F32, &c, nullptr, 0, nullptr, nullptr), true, "");
                c.active = 1;
                EXPECT(mcle_run_indoor_drops(&ctx, MCLE_F64, &c, 1, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                             nullptr, nullptr, nullptr, nullptr),
                       true, "");
            }
    char name[64] = "x";
    mcle_ctx_last_kernel(&ctx, name, sizeof(name));
    if (name[0] != 0) {
        std::printf("FAIL: a refused or empty call left the kernel tag '%s'\n", name);
        ++failures;
    }
    std::printf("indoor argument checks: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
