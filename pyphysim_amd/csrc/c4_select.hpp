// c4_select.hpp -- config 4 (mcle_run_mimo_ofdm): which kernel serves a call, as a pure function of the call.
//
// Host-only and HIP-free (include/mcle.h and the standard library): pipelines.hip builds a C4Query from the configuration and the
// context's options, c4_select() answers with a C4Plan, and the family's launcher (launch_mimo_ofdm_<family>(ctx, plan, cfg, ...))
// maps the plan's integers onto the instantiation they name.  A launcher cannot decline: a plan outside its instantiations is an
// internal error.  c4_plan_tag() formats the tag of mcle_ctx_last_kernel (grammar: include/mcle.h).  scripts/c4_select_dump.cpp
// runs the same function on a CPU; tests/test_c4_select_cpu.py compares it with the replay of tests/test_gpu_c4_edges.py over the
// whole cross product.  The measurements behind each default: DESIGN.md 5.5 - 5.28.
#pragma once
#include <cstdio>
#include "../../include/mcle.h"

namespace mcle {

// The decision form a wave kernel or a symbol walk compiles to (walk_f64.hpp: walk_dec_kind); GENERIC = the table search.
enum : int { WDEC_GENERIC = 0, WDEC_SLICER = 1, WDEC_QAM_CERT = 2, WDEC_QUAD_CERT = 3, WDEC_AXIS4_CERT = 4 };

// MCLE_OPT_F64_THREADS, every accepted value (the table of what each selects per size, geometry and arithmetic: include/mcle.h)
enum : int {
    C4_THR_DEFAULT = 0,
    C4_THR_R4_AH4 = 256,      // (1024, 4x4): planar radix-4 stages, four antennas per thread
    C4_THR_R16_ALT = 257,     // (1024, 4x4): planar radix-16, complex128 with a separate channel stage / complex64 bounded for three wavefronts
    C4_THR_R16_TABLE = 258,   // (1024, 4x4) complex128: planar radix-16, every layer-1 twiddle from the table
    C4_THR_R16_FUSED = 259,   // (1024, 4x4) complex64: planar radix-16 with the fused channel stage
    C4_THR_WAVE = 260,        // the wave kernel of round 6: full-wave (256), part-wave (512, 2048), quarter-wave (1024)
    C4_THR_PLANAR = 261,      // the planar family (the generic kernel at (256, 2x2))
    C4_THR_WAVE_ALT = 262,    // 260 at the other wavefront bound (2048: the one bound)
    C4_THR_PW4 = 263,         // (1024, 4x4): part-wave, explicit
    C4_THR_PW4_W2 = 264,      // (1024, 4x4): part-wave bounded for two wavefronts per SIMD
    C4_THR_PW_TIME = 265,     // part-wave, time-domain form
    C4_THR_PW_CLASS = 266,    // part-wave, a wavefront owns a time class ("/a")
    C4_THR_PW_PLANES = 267,   // part-wave, ownership by lane row, exchange by re / im planes ("/x")
    C4_THR_PW_HALVES = 268,   // part-wave, ownership by lane row, exchange in complex halves ("/h")
    C4_THR_512 = 512,         // (1024, 4x4): radix-4, two antennas per thread; (2048, Nr = 4): four antennas per thread
    C4_THR_1024 = 1024,       // (2048, Nr = 4): two antennas per thread
};
constexpr bool c4_threads_accepted(long long v) {
    return v == C4_THR_DEFAULT || (v >= C4_THR_R4_AH4 && v <= C4_THR_PW_HALVES) || v == C4_THR_512 || v == C4_THR_1024;
}

// Everything the choice depends on.
struct C4Query {
    bool f64;                                   // arithmetic
    int fft_size, nt, nr, num_used, cp_size;
    int M;                                      // constellation size
    int dec;                                    // WDEC_*: walk_dec_kind of the call's modem parameters
    long long f64_threads, f64_generic, no_mfma, f32_mfma, mfma_variant;
#ifdef MCLE_EXPERIMENTS
    long long f64_variant;
#endif
};

enum : int { C4_REFUSED_SHAPE = 0, C4_GENERIC, C4_PLANAR, C4_FW, C4_QW, C4_PW, C4_MFMA };

// The family and its instantiation parameters.  n / nt / nr: planar <N, NT, NR>, generic <N, NA = nt>, full-wave <NA = nt>,
// part-wave <NW = n / 256>.
struct C4Plan {
    int family = C4_REFUSED_SHAPE;
    bool f64 = true;
    int n = 0, nt = 0, nr = 0;
    int ah = 0;                  // planar: antennas per thread
    int wps = 0;                 // planar / full-wave / quarter-wave / part-wave: wavefronts per SIMD the registers are bounded for
    int variant = 0;             // planar: VAR; matrix-core: MCLE_OPT_MFMA_VARIANT resolved
    bool td = false, rows = false, halves = false;   // part-wave: time-domain form, ownership by lane row, exchange in complex halves
    char asked = 0;              // part-wave: 'x' / 'h' = that exchange asked for by value (what the default picks has no suffix)
    int abl = 0;                 // section ablation of the wave kernels (MCLE_EXPERIMENTS builds; always 0 otherwise)
};

// complex64 at 256 points (not 4 x 4), and at 512 with two receive antennas: two more wavefronts per SIMD than the complex128 table
// (those kernels hold 78 - 93 registers and a quarter of the planes: +5 ... +18 %, profiles/r06/c4_pmc.log.  NOT elsewhere: 512 points
// with three receive antennas LOSE 14 - 37 % at four wavefronts per SIMD, 1024 / 2048 do not move -- profiles/r06/planar_f32_wps_ab.log)
#ifndef MCLE_PLANAR_F32_WPS_PLUS
#define MCLE_PLANAR_F32_WPS_PLUS 2
#endif
#ifndef MCLE_PLANAR_F64_256_WPS3
#define MCLE_PLANAR_F64_256_WPS3 0      // (A/B: +1.5 ... -1.5 %, not adopted)
#endif
constexpr int planar_wps(bool f64, int n, int nt, int nr, int w64) {
    if (!f64 && w64 <= 3 && ((n == 256 && !(nt == 4 && nr == 4)) || (n == 512 && nr == 2))) return w64 + MCLE_PLANAR_F32_WPS_PLUS;
    if (MCLE_PLANAR_F64_256_WPS3 && f64 && n == 256 && nr <= 3 && w64 == 2) return 3;
    return w64;
}

// The planar radix-4 geometry table, (fft_size, Nt x Nr) -> antennas per thread, wavefronts per SIMD: Nr = 2 / 4 two antennas per
// thread ((N / 4) * (Nr / 2) threads), Nr = 3 three (one group); antenna groups past Nt idle in the IFFT.  complex64 keeps the
// complex128 bound (doubling it spilled 10 - 77 registers in every 4-receive-antenna shape) but for planar_wps above.
//     Nr = 2:  256 -> 2   512 -> 3   1024 -> 3   2048 -> 4        Nr = 3: 2        Nr = 4:  256 -> 3   512 -> 3   1024 -> 4   2048 -> 4
constexpr int planar_r4_ah(int nr) { return nr == 3 ? 3 : 2; }
constexpr int planar_r4_wps(bool f64, int n, int nt, int nr) {
    const int w64 = nr == 3 ? 2 : nr == 2 ? (n == 256 ? 2 : n == 2048 ? 4 : 3) : (n <= 512 ? 3 : 4);
    return planar_wps(f64, n, nt, nr, w64);
}

#ifdef MCLE_EXPERIMENTS
// section ablations (f64_variant = 32 | 64 | ... | 1024, the combinations listed): WRONG counters by construction, never in the product build
constexpr bool c4_abl_wave(long long v) { return (v >= 32 && v <= 1024 && (v & (v - 1)) == 0) || v == 2016; }    // one section, or all six
constexpr bool c4_abl_qw(long long v) { return c4_abl_wave(v) || v == 384; }
constexpr bool c4_abl_planar(long long v) { return c4_abl_qw(v) || v == 1920; }
#endif

// the planar family's kernel for a shape, or false: no planar kernel ((256, 2x2), one receive antenna, below 256 points)
inline bool c4_select_planar(const C4Query& q, C4Plan& p) {
    const int n = q.fft_size, nt = q.nt, nr = q.nr;
    const long long thr = q.f64_threads;
    if (!(n == 256 || n == 512 || n == 1024 || n == 2048) || nr < 2 || nr > 4 || nt < 1 || nt > nr) return false;
    if (n == 256 && nt == 2 && nr == 2) return false;
    p.family = C4_PLANAR;
    p.ah = planar_r4_ah(nr);
    p.wps = planar_r4_wps(q.f64, n, nt, nr);
    p.variant = 0;
    if (n == 1024 && nr == 4) {
        // the benchmark size with four receive antennas: radix-16 passes, one transform per wavefront, 256 threads -- complex128 with
        // the channel fused into the span-1 butterflies at two wavefronts per SIMD, complex64 with a separate channel stage at four
        // (profiles/r04/c4_f64_r16_ab.log, c4_f32_planar_ab.log).  Nt < 4: any value but 0 = the radix-4 table.
        const int r16_wps = q.f64 ? 2 : 4, r16_var = q.f64 ? 12 : 4;
        if (nt < 4) {
            if (thr == C4_THR_DEFAULT) p.ah = 4, p.wps = r16_wps, p.variant = r16_var;
            return true;
        }
#ifdef MCLE_EXPERIMENTS
        if (q.f64 && q.f64_variant >= 1 && q.f64_variant <= 3) {          // timing bounds on the 512-thread radix-4 form
            p.variant = (int)q.f64_variant;
            return true;
        }
        if (q.f64 && c4_abl_planar(q.f64_variant)) {
            p.ah = 4, p.wps = 2, p.variant = 12 | (int)q.f64_variant;
            return true;
        }
#endif
        if (thr == C4_THR_512) return true;                               // radix-4, two antennas per thread: the table's entry
        p.ah = 4, p.wps = r16_wps, p.variant = r16_var;
        if (thr == C4_THR_R4_AH4) p.wps = 2, p.variant = 0;               // radix-4, four antennas per thread, twiddles in registers
        else if (q.f64 && thr == C4_THR_R16_TABLE) p.variant = 28;
        else if (q.f64 && thr == C4_THR_R16_ALT) p.variant = 4;
        else if (!q.f64 && thr == C4_THR_R16_ALT) p.wps = 3;
        else if (!q.f64 && thr == C4_THR_R16_FUSED) p.variant = 12;
        return true;
    }
    // 2048 with four receive antennas: 1 024 threads (two antennas per thread) are four wavefronts per SIMD by themselves, a
    // 128-register bound the complex128 form does not meet.  Four antennas per thread (512 threads, nothing spilled) where it is the
    // faster form -- 4 x 4 in both arithmetics, every Nt in complex64; complex128 Nt < 4 keeps the 1 024-thread form WITH its spills
    // (profiles/r05/planar_2048_ab.log).  512 / 1024 force either.
    if (n == 2048 && nr == 4 && (thr == C4_THR_512 || (thr != C4_THR_1024 && (nt == 4 || !q.f64)))) p.ah = 4, p.wps = 2;
    return true;
}

inline C4Plan c4_select(const C4Query& q) {
    const int n = q.fft_size, nt = q.nt, nr = q.nr;
    const long long thr = q.f64_threads;
    const bool sq4 = nt == 4 && nr == 4;
    C4Plan p;
    p.f64 = q.f64, p.n = n, p.nt = nt, p.nr = nr;
    if (!q.f64 && q.f32_mfma && !q.no_mfma && n == 1024 && sq4) {       // the complex64 matrix-core kernel, on request only
        p.family = C4_MFMA;
        p.variant = q.mfma_variant ? (int)q.mfma_variant : 36;
        return p;
    }
    // f64_generic = 1 (either arithmetic) and no_mfma = 1 (complex64) keep the call on the generic kernel WHERE THAT ONE EXISTS
    // (Nt = Nr in {2, 4}); every other geometry still runs the planar family: an option selects a kernel, it does not shrink the envelope
    const bool has_generic = nt == nr && (nt == 2 || nt == 4);
    const bool want_generic = has_generic && (q.f64_generic || (!q.f64 && q.no_mfma));
    if (!want_generic) {
        // the wave kernels' envelope: full band, even prefix, decisions by the slicer or a certificate
        const bool wave = q.num_used == n && (q.cp_size & 1) == 0 && q.M <= 256 && q.dec != WDEC_GENERIC;
        const bool wave_thr = thr == C4_THR_DEFAULT || thr == C4_THR_WAVE || thr == C4_THR_WAVE_ALT;
        if (wave && n == 256 && has_generic && wave_thr) {
            // full-wave: a realization (2 x 2: two) per wavefront, either arithmetic.  complex128 bounded for three wavefronts per
            // SIMD, complex64 for two (nothing spilled: 1.46e8 realizations/s at 4 x 4 against 1.30e8 at three); 262 = the other bound
            p.family = C4_FW;
            p.wps = (thr == C4_THR_WAVE_ALT) == q.f64 ? 2 : 3;
#ifdef MCLE_EXPERIMENTS
            if (q.f64 && sq4 && c4_abl_wave(q.f64_variant)) p.wps = 3, p.abl = (int)q.f64_variant;
#endif
            return p;
        }
        const bool pw_thr = thr == C4_THR_DEFAULT || (thr >= C4_THR_PW_TIME && thr <= C4_THR_PW_HALVES) ||
                            (n == 1024 ? thr == C4_THR_PW4 || thr == C4_THR_PW4_W2 : thr == C4_THR_WAVE || thr == C4_THR_WAVE_ALT);
        if (wave && q.f64 && sq4 && (n == 512 || n == 1024 || n == 2048) && pw_thr) {
            // part-wave: NW = n / 256 wavefronts per realization, three per SIMD (2048: 512 threads, the one bound of two).  The
            // default form adds the signal after the receive transform, deals the partial transforms by lane row and exchanges the
            // partial spectra in complex halves at 1024 / 2048, by re / im planes at 512 (profiles/r20/f64_family_rates.json)
            p.family = C4_PW;
            p.wps = n == 2048 ? 2 : 3;
            p.td = thr == C4_THR_PW_TIME;
            p.rows = !p.td && thr != C4_THR_PW_CLASS;
            p.halves = p.rows && (thr == C4_THR_PW_HALVES || (thr != C4_THR_PW_PLANES && n != 512));
            p.asked = thr == C4_THR_PW_PLANES ? 'x' : thr == C4_THR_PW_HALVES ? 'h' : 0;
            if (n != 2048) {
                if (thr == C4_THR_WAVE_ALT || thr == C4_THR_PW4_W2) p.wps = 2;
#ifdef MCLE_EXPERIMENTS     // on the time-domain form and on the default form with the exchange by planes
                if ((thr < C4_THR_PW_CLASS || thr > C4_THR_PW_HALVES) && c4_abl_wave(q.f64_variant))
                    p.wps = 3, p.halves = false, p.abl = (int)q.f64_variant;
#endif
            }
            return p;
        }
        // quarter-wave (VALU decode, no on-axis certificate): by value only, the part-wave kernel took the default
        if (wave && q.f64 && sq4 && n == 1024 && wave_thr && (q.dec == WDEC_SLICER || q.dec == WDEC_QAM_CERT || q.dec == WDEC_QUAD_CERT)) {
            p.family = C4_QW;
            p.wps = thr == C4_THR_WAVE_ALT ? 2 : 3;
#ifdef MCLE_EXPERIMENTS
            if (c4_abl_qw(q.f64_variant)) p.wps = 3, p.abl = (int)q.f64_variant;
#endif
            return p;
        }
        if (c4_select_planar(q, p)) return p;
    }
    // the generic radix-4 kernel: 2 x 2 / 4 x 4 at 64 .. 2048 -- what is asked for by option, the shapes below 256 points, and
    // (256, 2 x 2) outside the full-wave envelope (faster there than a planar kernel would be: profiles/r05/f32_family_rates.json)
    if (has_generic) p.family = C4_GENERIC;          // (its launcher refuses an fft_size it has no kernel for)
    return p;
}

// The tag of mcle_ctx_last_kernel: one per kernel instantiation of the product build (the decision form and an ablation are not in it).
inline void c4_plan_tag(const C4Plan& p, char* out, int len) {
    const char* dt = p.f64 ? "f64" : "f32";
    switch (p.family) {
        case C4_GENERIC: std::snprintf(out, (size_t)len, "mimo_ofdm_generic<%d,%d> %s", p.n, p.nt, dt); break;
        case C4_PLANAR: std::snprintf(out, (size_t)len, "mimo_ofdm_planar<%d,%d,%d> %s ah%d w%d v%d", p.n, p.nt, p.nr, dt, p.ah, p.wps, p.variant); break;
        case C4_FW: std::snprintf(out, (size_t)len, "mimo_ofdm_fw<%d> %s w%d", p.nt, dt, p.wps); break;
        case C4_QW: std::snprintf(out, (size_t)len, "mimo_ofdm_qw w%d", p.wps); break;
        case C4_PW:
            std::snprintf(out, (size_t)len, "mimo_ofdm_pw<%d>/%s%s%s", p.n / 256, p.td ? "time" : "freq", p.wps == (p.n == 2048 ? 2 : 3) ? "" : "/w2",
                          !p.td && !p.rows ? "/a" : p.asked == 'x' ? "/x" : p.asked == 'h' ? "/h" : "");
            break;
        case C4_MFMA: std::snprintf(out, (size_t)len, "mimo_ofdm_mfma v%d", p.variant); break;
        default: if (len > 0) out[0] = 0; break;
    }
}

}  // namespace mcle
