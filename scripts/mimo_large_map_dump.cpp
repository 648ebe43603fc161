// mimo_large_map_dump.cpp -- the operand maps of the large-array Blast link (pyphysim_amd/csrc/mimo_large_map.hpp) on a CPU, for
// tests/test_mimo_large_cpu.py.
//
//   c++ -std=c++17 -I pyphysim_amd/csrc scripts/mimo_large_map_dump.cpp -o mimo_large_map_dump
//
// One query per line on standard input, three integers: f64 nt nr.  Per query on standard output
//   steps S
//   L step lane src i col part sign        64 S lines: record entry (step, lane) = sign * (part ? Im : Re) src[i][col];
//                                          src 0 = padding (zero), 1 = A, 2 = G
//   R step g kind idx part                 4 S lines: input row 4 step + g; kind 0 = padding, 1 = symbol of transmit antenna idx,
//                                          2 = noise sample of receive antenna idx; part 0 = Re, 1 = Im
//   D lane i row stream part               256 lines: result i of a lane is output row `row`, part of the estimate of `stream`
//                                          (-1: padding)
#include <cstdio>
#include "mimo_large_map.hpp"

int main() {
    int f64, nt, nr;
    while (std::scanf("%d %d %d", &f64, &nt, &nr) == 3) {
        if (nt < 1 || nt > mcle::kLargeMaxNt || nr < nt || nr > mcle::kLargeMaxNr) {
            std::fprintf(stderr, "mimo_large_map_dump: 1 <= nt <= %d, nt <= nr <= %d\n", mcle::kLargeMaxNt, mcle::kLargeMaxNr);
            return 2;
        }
        const int S = mcle::mimo_large_steps(nt, nr);
        std::printf("steps %d\n", S);
        for (int s = 0; s < S; ++s)
            for (int lane = 0; lane < 64; ++lane) {
                const mcle::MimoLargeEntry e = mcle::mimo_large_entry(f64 != 0, nt, nr, s, lane);
                std::printf("L %d %d %d %d %d %d %d\n", s, lane, e.src, e.i, e.col, e.part, e.sign);
            }
        for (int s = 0; s < S; ++s)
            for (int g = 0; g < 4; ++g) {
                const mcle::MimoLargeInput in = mcle::mimo_large_input(nt, nr, s, g);
                std::printf("R %d %d %d %d %d\n", s, g, in.kind, in.idx, in.part);
            }
        for (int lane = 0; lane < 64; ++lane)
            for (int i = 0; i < 4; ++i) {
                const mcle::MimoLargeOutput o = mcle::mimo_large_output(nt, lane, i);
                std::printf("D %d %d %d %d %d\n", lane, i, mcle::mimo_large_row(f64 != 0, lane >> 4, i), o.stream, o.part);
            }
    }
    return 0;
}
