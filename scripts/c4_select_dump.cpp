// c4_select_dump.cpp -- the config-4 kernel selection (pyphysim_amd/csrc/c4_select.hpp) on a CPU, for tests/test_c4_select_cpu.py.
//
//   c++ -std=c++17 -I include -I pyphysim_amd/csrc scripts/c4_select_dump.cpp -o c4_select_dump
//
// One query per line on standard input, thirteen integers:
//   f64 fft_size nt nr num_used cp_size M dec f64_threads f64_generic no_mfma f32_mfma mfma_variant
// (dec: the WDEC_* decision form, 0 = none .. 4 = on-axis certificate).  One line per query on standard output: the tag of
// mcle_ctx_last_kernel for the plan c4_select answers with, or "refused".
#include <cstdio>
#include "c4_select.hpp"

int main() {
    long long v[13];
    char tag[64];
    for (;;) {
        int got = 0;
        while (got < 13 && std::scanf("%lld", &v[got]) == 1) ++got;
        if (got == 0) return 0;
        if (got < 13) {
            std::fprintf(stderr, "c4_select_dump: a query is thirteen integers\n");
            return 2;
        }
        mcle::C4Query q{};
        q.f64 = v[0] != 0;
        q.fft_size = (int)v[1], q.nt = (int)v[2], q.nr = (int)v[3], q.num_used = (int)v[4], q.cp_size = (int)v[5];
        q.M = (int)v[6], q.dec = (int)v[7];
        q.f64_threads = v[8], q.f64_generic = v[9], q.no_mfma = v[10], q.f32_mfma = v[11], q.mfma_variant = v[12];
        const mcle::C4Plan plan = mcle::c4_select(q);
        mcle::c4_plan_tag(plan, tag, (int)sizeof(tag));
        std::puts(plan.family == mcle::C4_REFUSED_SHAPE ? "refused" : tag);
    }
}
