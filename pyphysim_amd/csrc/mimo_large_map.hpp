// mimo_large_map.hpp -- the operand maps of the large-array Blast link (pipeline_mimo_large.hip), HIP-free: the set-up kernel
// writes a realization's record by mimo_large_entry, the link kernel feeds the matrix cores by mimo_large_input and reads them by
// mimo_large_output; scripts/mimo_large_map_dump.cpp prints all three for tests/test_mimo_large_cpu.py.
//
// The link's estimate z = A x + G n (A = G H / sqrt(Nt): Nt x Nt, G: Nt x Nr) for 16 symbol columns is ONE real product
//     D [16 x 16] = L [16 x 4 S] . R [4 S x 16]
// on v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32, S K-steps of 4 rows.  A complex input q enters as two rows of R, Re q and
// Im q, and M = [A | G] as the real embedding: the column of Re q is [Mr; Mi], the column of Im q is [-Mi; Mr].
//   Inputs.  Lane l = 16 g + n supplies R[4 s + g][n] in step s.  Steps 2 p and 2 p + 1 carry Re and Im of ONE complex input per
//   lane group g, so a lane draws whole complex samples: the symbol of transmit antenna 4 p + g while p < PS = ceil(Nt / 4), the
//   noise sample of receive antenna 4 (p - PS) + g after that, PN = ceil(Nr / 4) pairs.  Each kind is padded to whole pairs (an input
//   beyond Nt / Nr is a zero row of R and a zero column of L): a step is then all symbols or all noise for the whole wavefront.
//   S = 2 (PS + PN) <= 12.
//   Outputs.  Result i of lane l is D[row(l, i)][n]: row = g + 4 i in complex128, 4 g + i in complex64 (the two instructions number
//   the rows differently).  Result i = h + 2 part is part (0 Re, 1 Im) of stream g + 4 h in either: a lane holds both parts of the
//   streams g and g + 4 of its column and decides them without a lane exchange.  In complex128 that is Re z_i in row i, Im z_i in
//   row i + 8.
#pragma once

namespace mcle {

constexpr int kLargeMaxNt = 8, kLargeMaxNr = 16;

constexpr int mimo_large_sym_pairs(int nt) { return (nt + 3) / 4; }
constexpr int mimo_large_noise_pairs(int nr) { return (nr + 3) / 4; }
constexpr int mimo_large_steps(int nt, int nr) { return 2 * (mimo_large_sym_pairs(nt) + mimo_large_noise_pairs(nr)); }
// values of the link's arithmetic per realization: S steps of 64 lanes
constexpr int mimo_large_record_len(int nt, int nr) { return 64 * mimo_large_steps(nt, nr); }

enum { LARGE_ZERO = 0, LARGE_A = 1, LARGE_G = 2 };          // source of a record entry
enum { LARGE_NONE = 0, LARGE_SYMBOL = 1, LARGE_NOISE = 2 };  // kind of an input row

// record entry (step, lane) = sign * (part ? Im : Re) src[i][col]; src == LARGE_ZERO: padding, exactly zero
struct MimoLargeEntry {
    int src, i, col, part, sign;
};
// input row 4 step + g: part (0 Re, 1 Im) of the symbol of transmit antenna idx / the noise sample of receive antenna idx
struct MimoLargeInput {
    int kind, idx, part;
};
// result i of a lane: part of the estimate of `stream`; stream < 0: padding
struct MimoLargeOutput {
    int stream, part;
};

constexpr MimoLargeInput mimo_large_input(int nt, int nr, int step, int g) {
    const int p = step >> 1, part = step & 1, ps = mimo_large_sym_pairs(nt);
    if (p < ps) {
        const int a = 4 * p + g;
        return a < nt ? MimoLargeInput{LARGE_SYMBOL, a, part} : MimoLargeInput{LARGE_NONE, 0, part};
    }
    const int r = 4 * (p - ps) + g;
    return r < nr ? MimoLargeInput{LARGE_NOISE, r, part} : MimoLargeInput{LARGE_NONE, 0, part};
}

// (lane group g, result i) -> output row of the matrix-core instruction
constexpr int mimo_large_row(bool f64, int g, int i) { return f64 ? g + 4 * i : 4 * g + i; }

// (the same in both arithmetics: only the instruction's row of (g, i) differs, mimo_large_row)
constexpr MimoLargeOutput mimo_large_output(int nt, int lane, int i) {
    const int stream = (lane >> 4) + 4 * (i & 1);
    return stream < nt ? MimoLargeOutput{stream, i >> 1} : MimoLargeOutput{-1, i >> 1};
}

constexpr MimoLargeEntry mimo_large_entry(bool f64, int nt, int nr, int step, int lane) {
    const int row = lane & 15;
    const int g = f64 ? (row & 3) : (row >> 2), i = f64 ? (row >> 2) : (row & 3);     // inverse of mimo_large_row
    const int stream = g + 4 * (i & 1), out_part = i >> 1;
    const MimoLargeInput in = mimo_large_input(nt, nr, step, lane >> 4);
    if (stream >= nt || in.kind == LARGE_NONE) return MimoLargeEntry{LARGE_ZERO, 0, 0, 0, 0};
    // Re z += Mr qr - Mi qi, Im z += Mi qr + Mr qi
    return MimoLargeEntry{in.kind == LARGE_SYMBOL ? LARGE_A : LARGE_G, stream, in.idx, out_part != in.part ? 1 : 0,
                          (out_part == 0 && in.part == 1) ? -1 : 1};
}

}  // namespace mcle
