// Stand-alone host program for the sanitizer build of the C ABI's channel-estimation entry points: every argument rule of
// mcle_cazac_estimate, mcle_run_chanest, mcle_cazac_cancel and mcle_run_chanest_ic is driven with a context built on the host (no device is opened: each call returns
// from its checks, or fails at the first device call after them).  Built by `make -C pyphysim_amd/csrc asan-argcheck SAN=...`
// ("Host sanitizer runs"), exits non-zero on the first unexpected return code.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

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

int main() {
    mcle_ctx ctx;                               // host-side bookkeeping only
    std::vector<double> buf(64, 0.0);           // stands in for device arrays: never dereferenced by the checks
    void* p = buf.data();
    const double cover[2] = {1.0, -1.0};
    EXPECT(mcle_cazac_estimate(nullptr, MCLE_F64, p, 48, p, 1, 1, nullptr, 5, 2, 0, p), false, "null context");
    EXPECT(mcle_cazac_estimate(&ctx, 7, p, 48, p, 1, 1, nullptr, 5, 2, 0, p), false, "dtype");
    EXPECT(mcle_cazac_estimate(&ctx, MCLE_F64, p, 1, p, 1, 1, nullptr, 0, 2, 0, p), false, "at least 2");
    EXPECT(mcle_cazac_estimate(&ctx, MCLE_F64, p, 48, p, 1, 1, nullptr, 5, 0, 0, p), false, "size_multiplier");
    EXPECT(mcle_cazac_estimate(&ctx, MCLE_F64, p, 2049, p, 1, 1, nullptr, 5, 2, 0, p), false, "4096");
    EXPECT(mcle_cazac_estimate(&ctx, MCLE_F64, p, 48, p, 1, 1, nullptr, 48, 2, 0, p), false, "num_taps_to_keep");
    EXPECT(mcle_cazac_estimate(&ctx, MCLE_F64, p, 48, p, 1, 1, nullptr, -1, 2, 0, p), false, "num_taps_to_keep");
    EXPECT(mcle_cazac_estimate(&ctx, MCLE_F64, p, 48, p, 1, 9, cover, 5, 2, 0, p), false, "cover");
    EXPECT(mcle_cazac_estimate(&ctx, MCLE_F64, p, 48, p, 1, 0, cover, 5, 2, 0, p), false, "cover");
    EXPECT(mcle_cazac_estimate(&ctx, MCLE_F64, p, 48, p, 1, 2, nullptr, 5, 2, 0, p), false, "null cover");
    EXPECT(mcle_cazac_estimate(&ctx, MCLE_F32, p, 48, nullptr, 1, 2, cover, 5, 2, 0, p), false, "null array");
    EXPECT(mcle_cazac_estimate(&ctx, MCLE_F32, p, 48, p, 0, 2, cover, 5, 2, 0, p), true, "");

    mcle_chanest_cfg good;
    std::memset(&good, 0, sizeof(good));
    good.ne = 48, good.size_multiplier = 2, good.num_taps_to_keep = 5, good.n_users = 3, good.n_rx = 2, good.n_taps = 2;
    good.noise_var = 0.1, good.tap_power[0] = 1.0, good.tap_power[1] = 0.5, good.tap_delay[1] = 3, good.d_ref_seq = p;
    double* d = buf.data();
    EXPECT(mcle_run_chanest(nullptr, MCLE_F64, &good, 1, 0, 4, d, d), false, "null argument");
    EXPECT(mcle_run_chanest(&ctx, MCLE_F64, nullptr, 1, 0, 4, d, d), false, "null argument");
    EXPECT(mcle_run_chanest(&ctx, 5, &good, 1, 0, 4, d, d), false, "dtype");
    mcle_chanest_cfg c = good;
    c.ne = 1;
    EXPECT(mcle_run_chanest(&ctx, MCLE_F64, &c, 1, 0, 4, d, d), false, "at least 2");
    c = good, c.size_multiplier = 0;
    EXPECT(mcle_run_chanest(&ctx, MCLE_F64, &c, 1, 0, 4, d, d), false, "size_multiplier");
    c = good, c.ne = 2049;
    EXPECT(mcle_run_chanest(&ctx, MCLE_F64, &c, 1, 0, 4, d, d), false, "4096");
    c = good, c.num_taps_to_keep = 48;
    EXPECT(mcle_run_chanest(&ctx, MCLE_F64, &c, 1, 0, 4, d, d), false, "num_taps_to_keep");
    c = good, c.n_users = 9;
    EXPECT(mcle_run_chanest(&ctx, MCLE_F64, &c, 1, 0, 4, d, d), false, "n_users");
    c = good, c.n_rx = 5;
    EXPECT(mcle_run_chanest(&ctx, MCLE_F64, &c, 1, 0, 4, d, d), false, "n_rx");
    c = good, c.n_taps = MCLE_MAX_TAPS + 1;
    EXPECT(mcle_run_chanest(&ctx, MCLE_F64, &c, 1, 0, 4, d, d), false, "n_taps");
    c = good, c.n_taps = MCLE_MAX_TAPS, c.tap_delay[MCLE_MAX_TAPS - 1] = 48;      // the last slot of the arrays is read
    EXPECT(mcle_run_chanest(&ctx, MCLE_F64, &c, 1, 0, 4, d, d), false, "tap delays");
    c = good, c.noise_var = -1.0;
    EXPECT(mcle_run_chanest(&ctx, MCLE_F64, &c, 1, 0, 4, d, d), false, "noise variance");
    c = good, c.tap_power[0] = 0.0, c.tap_power[1] = 0.0;
    EXPECT(mcle_run_chanest(&ctx, MCLE_F64, &c, 1, 0, 4, d, d), false, "sum to zero");
    EXPECT(mcle_run_chanest(&ctx, MCLE_F64, &good, 1, 0, 1ull << 31, d, d), false, "2^31");
    c = good, c.d_ref_seq = nullptr;
    EXPECT(mcle_run_chanest(&ctx, MCLE_F64, &c, 1, 0, 4, d, d), false, "null array");
    EXPECT(mcle_run_chanest(&ctx, MCLE_F32, &good, 1, 0, 0, d, d), true, "");

    EXPECT(mcle_cazac_cancel(nullptr, MCLE_F64, p, 48, p, p, 1, 2, p), false, "null context");
    EXPECT(mcle_cazac_cancel(&ctx, 7, p, 48, p, p, 1, 2, p), false, "dtype");
    EXPECT(mcle_cazac_cancel(&ctx, MCLE_F64, p, 1, p, p, 1, 2, p), false, "at least 2");
    EXPECT(mcle_cazac_cancel(&ctx, MCLE_F64, p, 48, p, p, 1, 0, p), false, "size_multiplier");
    EXPECT(mcle_cazac_cancel(&ctx, MCLE_F64, p, 2049, p, p, 1, 2, p), false, "4096");
    EXPECT(mcle_cazac_cancel(&ctx, MCLE_F64, p, 48, p, nullptr, 1, 2, p), false, "null array");
    EXPECT(mcle_cazac_cancel(&ctx, MCLE_F32, p, 48, p, p, 1, 2, nullptr), false, "null array");
    EXPECT(mcle_cazac_cancel(&ctx, MCLE_F32, p, 48, nullptr, nullptr, 0, 2, nullptr), true, "");

    mcle_chanest_ic_cfg ig;
    std::memset(&ig, 0, sizeof(ig));
    ig.base = good, ig.mode = 2, ig.direct_user = 1;
    for (int u = 0; u < 3; ++u) ig.link_gain[u] = 0.5;          // users 3 .. 7 stay 0: not read
    int32_t* o = reinterpret_cast<int32_t*>(buf.data());
    EXPECT(mcle_run_chanest_ic(nullptr, MCLE_F64, &ig, 1, 0, 4, d, d, o), false, "null argument");
    EXPECT(mcle_run_chanest_ic(&ctx, MCLE_F64, nullptr, 1, 0, 4, d, d, o), false, "null argument");
    EXPECT(mcle_run_chanest_ic(&ctx, 5, &ig, 1, 0, 4, d, d, o), false, "dtype");
    mcle_chanest_ic_cfg ic = ig;
    ic.base.ne = 1;
    EXPECT(mcle_run_chanest_ic(&ctx, MCLE_F64, &ic, 1, 0, 4, d, d, o), false, "at least 2");
    ic = ig, ic.base.size_multiplier = 0;
    EXPECT(mcle_run_chanest_ic(&ctx, MCLE_F64, &ic, 1, 0, 4, d, d, o), false, "size_multiplier");
    ic = ig, ic.base.ne = 2049;
    EXPECT(mcle_run_chanest_ic(&ctx, MCLE_F64, &ic, 1, 0, 4, d, d, o), false, "4096");
    ic = ig, ic.base.num_taps_to_keep = 48;
    EXPECT(mcle_run_chanest_ic(&ctx, MCLE_F64, &ic, 1, 0, 4, d, d, o), false, "num_taps_to_keep");
    ic = ig, ic.base.n_users = 9;
    EXPECT(mcle_run_chanest_ic(&ctx, MCLE_F64, &ic, 1, 0, 4, d, d, o), false, "n_users");
    ic = ig, ic.base.n_rx = 0;
    EXPECT(mcle_run_chanest_ic(&ctx, MCLE_F64, &ic, 1, 0, 4, d, d, o), false, "n_rx");
    ic = ig, ic.base.n_taps = 0;
    EXPECT(mcle_run_chanest_ic(&ctx, MCLE_F64, &ic, 1, 0, 4, d, d, o), false, "n_taps");
    ic = ig, ic.base.tap_delay[1] = 48;
    EXPECT(mcle_run_chanest_ic(&ctx, MCLE_F64, &ic, 1, 0, 4, d, d, o), false, "tap delays");
    ic = ig, ic.base.tap_power[1] = -0.5;
    EXPECT(mcle_run_chanest_ic(&ctx, MCLE_F64, &ic, 1, 0, 4, d, d, o), false, "tap powers");
    ic = ig, ic.base.noise_var = -1.0;
    EXPECT(mcle_run_chanest_ic(&ctx, MCLE_F64, &ic, 1, 0, 4, d, d, o), false, "noise variance");
    ic = ig, ic.base.tap_power[0] = 0.0, ic.base.tap_power[1] = 0.0;
    EXPECT(mcle_run_chanest_ic(&ctx, MCLE_F64, &ic, 1, 0, 4, d, d, o), false, "sum to zero");
    EXPECT(mcle_run_chanest_ic(&ctx, MCLE_F64, &ig, 1, 0, 1ull << 31, d, d, o), false, "2^31");
    ic = ig, ic.mode = 3;
    EXPECT(mcle_run_chanest_ic(&ctx, MCLE_F64, &ic, 1, 0, 4, d, d, o), false, "mode");
    ic = ig, ic.mode = -1;
    EXPECT(mcle_run_chanest_ic(&ctx, MCLE_F64, &ic, 1, 0, 4, d, d, o), false, "mode");
    ic = ig, ic.direct_user = 3;
    EXPECT(mcle_run_chanest_ic(&ctx, MCLE_F64, &ic, 1, 0, 4, d, d, o), false, "direct_user");
    ic = ig, ic.direct_user = -1;
    EXPECT(mcle_run_chanest_ic(&ctx, MCLE_F64, &ic, 1, 0, 4, d, d, o), false, "direct_user");
    ic = ig, ic.link_gain[2] = 0.0;                             // the last gain that is read
    EXPECT(mcle_run_chanest_ic(&ctx, MCLE_F64, &ic, 1, 0, 4, d, d, o), false, "link gains");
    ic = ig, ic.link_gain[0] = -1.0;
    EXPECT(mcle_run_chanest_ic(&ctx, MCLE_F64, &ic, 1, 0, 4, d, d, o), false, "link gains");
    ic = ig, ic.link_gain[1] = std::nan("");
    EXPECT(mcle_run_chanest_ic(&ctx, MCLE_F64, &ic, 1, 0, 4, d, d, o), false, "link gains");
    ic = ig, ic.link_gain[1] = HUGE_VAL;
    EXPECT(mcle_run_chanest_ic(&ctx, MCLE_F64, &ic, 1, 0, 4, d, d, o), false, "link gains");
    ic = ig, ic.base.d_ref_seq = nullptr;
    EXPECT(mcle_run_chanest_ic(&ctx, MCLE_F64, &ic, 1, 0, 4, d, d, o), false, "null array");
    EXPECT(mcle_run_chanest_ic(&ctx, MCLE_F64, &ig, 1, 0, 4, d, nullptr, o), false, "null array");
    // one realization beyond the LDS of a compute unit: 8 users x 4 antennas x 2048 kept taps of complex128 (decided on the host)
    ic = ig, ic.base.ne = 2048, ic.base.num_taps_to_keep = 2047, ic.base.n_users = 8, ic.base.n_rx = 4;
    for (int u = 0; u < 8; ++u) ic.link_gain[u] = 1.0;
    EXPECT(mcle_run_chanest_ic(&ctx, MCLE_F64, &ic, 1, 0, 4, d, d, o), false, "does not fit");
    EXPECT(mcle_run_chanest_ic(&ctx, MCLE_F32, &ig, 1, 0, 0, d, d, nullptr), true, "");
    char name[64] = "x";
    mcle_ctx_last_kernel(&ctx, name, sizeof(name));
    if (name[0] != 0) {
        std::printf("FAIL: a refused call left the kernel tag '%s'\n", name);
        ++failures;
    }
    std::printf("chanest argument checks: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
