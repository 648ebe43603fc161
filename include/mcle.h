/*
 * mcle.h -- C ABI of libmcle: the MI355X (gfx950) Monte Carlo link-level engine.
 *
 * The reference (darcamo/pyphysim v0.7.2) is pure Python/NumPy and has no FFI; its
 * "operator interface" for the hot path is a set of Python method signatures.  Each entry
 * point below names the reference method it stands in for (paths relative to the reference).
 * A maintainer-side ctypes binding is sketched in INTEGRATION.md.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error (MCLE_E_*); mcle_last_error() gives the
 *     message for the calling thread.  No exception crosses the ABI.
 *   - `d_` arguments are DEVICE pointers (hipMalloc'ed by anyone: mcle_malloc, PyTorch, ...);
 *     everything else is host memory or passed by value.
 *   - complex arrays are interleaved (re, im) of the context dtype: MCLE_F32 -> float,
 *     MCLE_F64 -> double (the parity instantiation; reference arithmetic is complex128).
 *   - symbol indices are int32 on the device (the reference uses int64 on the host).
 *   - all work is enqueued on the context's stream; only mcle_ctx_sync / mcle_memcpy_d2h and
 *     the *_host helpers block.  A context is not thread-safe; distinct contexts are.
 */
#ifndef MCLE_H
#define MCLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCLE_VERSION 1

enum { MCLE_OK = 0, MCLE_E_INVAL = -1, MCLE_E_HIP = -2, MCLE_E_NOMEM = -3, MCLE_E_STATE = -4,
       MCLE_E_UNSUPPORTED = -5 /* valid request outside a fused kernel's envelope and no generic kernel behind the same entry
                                  point: returned by mcle_run_mimo_ofdm_tdl only (compose the staged operators); every other
                                  mcle_run_* falls back internally or reports its envelope as MCLE_E_INVAL */ };
enum { MCLE_F32 = 0, MCLE_F64 = 1 };
/* demodulation method: exhaustive minimum distance over the constellation held in LDS
 * (any constellation), or the per-axis slicer (square Gray QAM only; same decisions). */
enum { MCLE_DEMOD_MINDIST = 0, MCLE_DEMOD_QAM_SLICER = 1 };
/* constellation kinds (tell the library what structure it may exploit) */
enum { MCLE_CONST_GENERIC = 0, MCLE_CONST_QAM = 1, MCLE_CONST_BPSK = 2 };

typedef struct mcle_ctx mcle_ctx;

/* Integer result block of one parameter variation.  Every field is an exact integer sum over
 * realizations, so reductions are order-independent and identical for any GPU count.  It carries
 * what Result.update()/merge() accumulate (simulations/results.py:469-623): value = sum of
 * errors, total = n_realizations * units per realization, sum / sum-of-squares of the
 * per-realization ratio = {sum, sum_sq} / units^k. */
typedef struct mcle_counters {
    uint64_t n_realizations;
    uint64_t n_skipped;        /* SkipThisOne analogue (runner.py:151-185): singular filter etc. */
    uint64_t sym_errors;       /* sum_r e_r          */
    uint64_t sym_errors_sq;    /* sum_r e_r^2        */
    uint64_t bit_errors;
    uint64_t bit_errors_sq;
    uint64_t n_symbols;        /* symbols per realization (constant)  */
    uint64_t n_bits;           /* bits per realization (constant)     */
} mcle_counters;

/* ---- context, stream, memory -------------------------------------------------------- */
const char* mcle_last_error(void);
int mcle_version(void);
int mcle_device_count(int* count);
int mcle_ctx_create(int device_id, mcle_ctx** out);
int mcle_ctx_destroy(mcle_ctx* ctx);
/* adopt an external hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = own */
int mcle_ctx_set_stream(mcle_ctx* ctx, void* hip_stream);
int mcle_ctx_get_stream(mcle_ctx* ctx, void** hip_stream);
int mcle_ctx_sync(mcle_ctx* ctx);
/* Releases the context's scratch buffer (fading / filter records of the two-launch pipelines: up to 138 MiB for the
 * complex128 MIMO-OFDM family, 256 MiB + 25 % for mcle_run_mimo_ofdm_tdl; it otherwise lives until mcle_ctx_destroy).
 * Waits for the stream first.  The next call that needs it allocates again. */
int mcle_ctx_trim_scratch(mcle_ctx* ctx);
int mcle_ctx_device_info(mcle_ctx* ctx, int* n_cu, int* lds_bytes, char* name, int name_len);
/* Diagnostic: a short tag naming the kernel that served the context's last mcle_run_ofdm_tdl / mcle_run_mimo_ofdm_tdl call, e.g.
 * "siso_hw K=3", "siso_wave N=1024 K=6", "siso_batched K=9", "siso_mfma", "siso_single", "mimo_wave_parked K=5", "mimo_wave_rt K=3",
 * "mimo_coop" (K: the tap polynomials' order).  Empty before such a call and after one that launched nothing.  Copies at most
 * len - 1 characters and a terminating zero into name.
 * The staged operators with more than one form set it too (cleared on entry, so a call that launches nothing leaves it empty):
 *   mcle_awgn_add / mcle_cmul / mcle_cdiv     "binary pair" (complex64, all three pointers 16-byte aligned), "binary elem"
 *   mcle_modulate / mcle_demodulate           "modulate pair" / "demodulate pair" (complex64, labels 8- and samples 16-byte
 *                                             aligned), "modulate elem" / "demodulate elem"
 *   mcle_randn_c                              "randn_c c64 pair" (complex64, first_sample even, output 16-byte aligned: the
 *                                             whole pairs as 16-byte stores), "randn_c elem"
 *   mcle_rand_modulate_batch(_u8)             "rand_modulate pair" (n even, labels 8- and samples 16-byte aligned), "rand_modulate
 *                                             elem"; "rand_modulate_u8 x16" (n % 16 == 0, both 16-byte aligned), "rand_modulate_u8
 *                                             elem"
 *   mcle_blast_encode                         "blast_encode pairs" (nt 2 or 4, even columns, both pointers aligned to a pair of
 *                                             elements), "blast_encode elem"
 *   mcle_blast_filter                         "blast_filter staged" (matrix a multiple of 16 bytes, H and G 16-byte aligned,
 *                                             batch >= 64), "blast_filter direct"
 *   mcle_blast_decode                         "blast_decode c64 4x4 x4" (16-byte stores: estimates 16-byte aligned),
 *                                             "blast_decode 4x4", "blast_decode generic"
 *   mcle_mimo_channel                         "mimo_channel c64 4x4 pair" (even columns, X, Y and noise 16-byte aligned),
 *                                             "mimo_channel 4x4", "mimo_channel generic"
 *   mcle_mimo_channel_philox                  "mimo_channel_philox c64 4x4 pair" (as above without the noise array),
 *                                             "mimo_channel_philox f64 4x4 lane" (even columns), "mimo_channel_philox generic"
 *   mcle_alamouti_decode                      "alamouti_decode pair" (Y and out aligned to a pair), "alamouti_decode elem"
 *   mcle_jakes_taps_philox                    "jakes_taps c64 x4" (complex64, even n, taps 16-byte aligned), "jakes_taps elem"
 * MCLE_OPT_STAGED_GENERIC = 1 selects the last-named (generic) form of each.
 * Config 4 (mcle_run_mimo_ofdm): every launcher names itself, one tag per kernel instantiation of the product build (the decision
 * form -- slicer or which certificate -- is a template argument of the wave kernels too and is NOT in the tag):
 *   "mimo_ofdm_pw<NW>/freq", ".../time"        part-wave, NW = 2 / 4 / 8 wavefronts per realization (512 / 1024 / 2048), the round-7 form /
 *                                             the time-domain form; suffix "/w2" = registers bounded for two wavefronts per SIMD where
 *                                             three is the default (NW = 2: f64_threads 262, NW = 4: 264; NW = 8 has the one bound);
 *                                             suffix "/a" (after "/freq" only) = the ownership map of rounds 6 - 9, wavefront = time
 *                                             class and lane row = antenna (f64_threads 266); suffix "/x" (after "/freq" only) = ownership
 *                                             by lane row with the exchange by re / im planes of rounds 10 - 19 asked for (f64_threads
 *                                             267), suffix "/h" = with the exchange in complex halves asked for (268); no suffix =
 *                                             ownership by lane row, the exchange the default picks (halves at 1024 / 2048, planes at 512)
 *   "mimo_ofdm_fw<NA> f64|f32 w<WPS>"          full-wave at 256 points, NA x NA antennas, wavefronts per SIMD the registers are bounded for
 *   "mimo_ofdm_qw w<WPS>"                      quarter-wave (complex128, 1024, 4x4)
 *   "mimo_ofdm_planar<N,NT,NR> f64|f32 ah<AH> w<WPS> v<VARIANT>"   the planar family: antennas per thread, wavefronts per SIMD, variant
 *                                             (0 = radix-4 stages; radix-16 passes: 4 = separate channel stage, 12 = fused, 28 = fused
 *                                             with every layer-1 twiddle from the table)
 *   "mimo_ofdm_mfma v<36|32|30|21>"            the complex64 matrix-core kernel and its variant
 *   "mimo_ofdm_generic<N,NA> f64|f32"          the generic radix-4 kernel (2x2 / 4x4, 64 .. 2048)
 * "" after a refused call. */
int mcle_ctx_last_kernel(mcle_ctx* ctx, char* name, int len);
int mcle_malloc(mcle_ctx* ctx, size_t bytes, void** d_ptr);
int mcle_free(mcle_ctx* ctx, void* d_ptr);
int mcle_memset(mcle_ctx* ctx, void* d_ptr, int value, size_t bytes);
int mcle_memcpy_h2d(mcle_ctx* ctx, void* d_dst, const void* src, size_t bytes);
int mcle_memcpy_d2h(mcle_ctx* ctx, void* dst, const void* d_src, size_t bytes); /* blocks */
/* device-to-device strided row copy (rows of row_bytes; pitches in bytes), enqueued on the stream */
int mcle_memcpy_2d(mcle_ctx* ctx, void* d_dst, size_t dst_pitch, const void* d_src, size_t src_pitch,
                   size_t row_bytes, size_t rows);
/* Per-context kernel-selection options (round 3: they used to be environment variables read inside the launch
 * path, which made a context's behaviour depend on the caller's environment).  Every option is an integer, 0 is the
 * default, and none of them changes a result beyond the rounding-level differences documented per kernel:
 * they exist for A/B measurements and for tests that compare the matrix-core kernels with the VALU kernels they
 * replace.  set: MCLE_E_INVAL for an unknown option or a value outside its range. */
enum {
    MCLE_OPT_NO_MFMA = 0,          /* 1: every fused pipeline / operator runs its VALU kernel (no matrix-core form) */
    MCLE_OPT_MFMA_VARIANT = 1,     /* config-4 matrix-core kernel variant: 0 (= 36), 36, 32, 30, 21 */
    MCLE_OPT_GRID_OVERSUB = 2,     /* persistent grids = this multiple of the resident set; 0: automatic (<= 8) */
    MCLE_OPT_FLAT_WGS_PER_CU = 3,  /* single-carrier kernels: workgroups started per CU; 0: 64 */
    MCLE_OPT_SINGLE_TDL = 4,       /* 1: config 3 on the one-realization-per-workgroup kernel */
    MCLE_OPT_TDL_MFMA_WAVES = 5,   /* config-3 matrix-core kernel: 0 / 2 = two waves per SIMD, 3 = three, 32 = three with two
                                      realizations per pass instead of four */
    MCLE_OPT_JAKES_DIRECT = 6,     /* 1: one sincos per ray and sample (jakes_generate: k_jakes; complex128 flat-fading pipeline: no rotation recurrence) */
    MCLE_OPT_F64_GENERIC = 7,      /* 1: config 4 on the generic radix-4 kernel instead of the planar family and the wave kernels (either
                                      arithmetic) WHERE THAT KERNEL EXISTS: Nt = Nr in {2, 4}; every other geometry still runs the planar
                                      family -- like no_mfma, the option selects a kernel and does not shrink the envelope.  (2048, 4x4)
                                      in complex128 is refused with it: the generic kernel needs 168 KiB of LDS there.  f32_mfma = 1
                                      comes first at complex64 (1024, 4x4). */
    MCLE_OPT_F64_THREADS = 8,      /* which of the kept config-4 kernels serves mcle_run_mimo_ofdm (A/B runs, kernel-vs-kernel tests: same
                                      results contract).  Read off csrc/c4_select.hpp (c4_select: the one place that reads the value; a
                                      name per value there); why each form exists and what it measured: DESIGN.md 5.5 - 5.28.  The wave
                                      kernels (fw / pw / qw) need their envelope -- full band, even cyclic prefix, decisions by the
                                      slicer or a certificate (qw: no on-axis certificate) -- and OUTSIDE it every value that names one
                                      selects what 261 selects.  "P" = the planar family's kernel of the shape, tag
                                      "mimo_ofdm_planar<N,NT,NR> f64|f32 ah<AH> w<WPS> v<VAR>" (ah, w, v below); pw<NW> = tag
                                      "mimo_ofdm_pw<NW>/freq", fw<NA> = "mimo_ofdm_fw<NA> f64|f32 w<WPS>", qw = "mimo_ofdm_qw w<WPS>".

                                      value | (256, 2x2 / 4x4)     | c128 (512, 4x4) | c128 (1024, 4x4)  | c64 (1024, 4x4) | c128 (2048, 4x4)
                                      ------+----------------------+-----------------+-------------------+-----------------+-----------------
                                          0 | fw w3 (c64: w2)      | pw<2>           | pw<4>             | P ah4 w4 v4     | pw<8>
                                        256 | as 261               | as 261          | P ah4 w2 v0       | P ah4 w2 v0     | as 261
                                        257 | as 261               | as 261          | P ah4 w2 v4       | P ah4 w3 v4     | as 261
                                        258 | as 261               | as 261          | P ah4 w2 v28      | as 0            | as 261
                                        259 | as 261               | as 261          | as 261            | P ah4 w4 v12    | as 261
                                        260 | as 0                 | as 0            | qw w3             | as 0            | as 0
                                        261 | 4x4: P ah2 w3 v0,    | P ah2 w3 v0     | P ah4 w2 v12      | as 0            | P ah4 w2 v0
                                            | 2x2: generic kernel  |                 |                   |                 |
                                        262 | fw w2 (c64: w3)      | pw<2> + "/w2"   | qw w2             | as 0            | as 0 (one bound)
                                        263 | as 261               | as 261          | as 0              | as 0            | as 261
                                        264 | as 261               | as 261          | pw<4> + "/w2"     | as 0            | as 261
                                        265 | as 261               | "mimo_ofdm_pw<NW>/time": the time-domain form      | as 0 | (as 512, 1024)
                                        266 | as 261               | pw<NW> + "/a": a wavefront owns a time class        | as 0 | (as 512, 1024)
                                        267 | as 261               | pw<NW> + "/x": lane rows, exchange by re / im planes | as 0 | (as 512, 1024)
                                        268 | as 261               | pw<NW> + "/h": lane rows, exchange in complex halves | as 0 | (as 512, 1024)
                                        512 | as 261               | as 261          | P ah2 w4 v0       | P ah2 w4 v0     | as 261
                                       1024 | as 261               | as 261          | as 261            | as 0            | P ah2 w4 v0

                                      What the default (0) of the part-wave kernel is: lane rows, the exchange in complex halves at 1024 and
                                      2048 points and by re / im planes at 512 -- 267 / 268 name an exchange and carry the suffix also
                                      where it is the default's.  complex64 at (512, 4x4) and (2048, 4x4): P at every value (2048: ah4 w2 v0,
                                      and ah2 w4 v0 for 1024).  Other geometries, either arithmetic: (1024, Nt < 4, Nr = 4): 0 = radix-16
                                      passes (complex128 ah4 w2 v12, complex64 ah4 w4 v4), any other value the radix-4 form ah2 w4 v0;
                                      (2048, Nt < 4, Nr = 4): 512 = ah4 w2 v0 (the default in complex64), 1024 = ah2 w4 v0 (the default
                                      in complex128); every other shape has one kernel and ignores the value.  f64_generic, no_mfma and
                                      f32_mfma come first (see there). */
    MCLE_OPT_BD_RUNTIME_SOLVE = 9, /* 1: the block-diagonalisation pipeline solves with the run-time-sized routine (private
                                      arrays in scratch) also where the compile-time-sized one (K nr <= 6) applies */
    MCLE_OPT_DEMOD_NOCERT = 10,    /* 1: min-distance decisions of a square Gray QAM always through the table search (candidate
                                      grid / sweep); 0: through the margin certificate of modem.hpp (demod_qam_cert: the
                                      closed-form nearest level per axis, accepted when the received point is farther than
                                      2^-30 (complex64: 2^-15) of a level spacing from every decision boundary -- and, in
                                      complex64, no farther than 16 spacings outside the outermost level -- the table search
                                      otherwise: no table gathers, and the decisions of the exhaustive sweep by a margin argument
                                      that holds for |re|, |im| up to ~2^11 level spacings in complex128 (beyond that -- an
                                      equaliser output in a fade of -66 dB -- the identity rests on test coverage: the chance that
                                      such a point also sits within 2^-30 of a boundary is ~1e-14 per symbol).  complex128, four
                                      decisions at a time (walk_f64.hpp: walk_qam_fixed4): the margin is first tested in FIXED
                                      POINT -- q = (int) fma(e, hs 2^24, (hl + 1/2) 2^24) clamped to [2^23, lm1 2^24 + 2^23],
                                      level q >> 24, accepted when the fraction q & (2^24 - 1) keeps 2 counts off either end,
                                      i.e. 2^-23 of a spacing off every boundary; the multiply-add rounds by <= 2^-25 counts, so
                                      an accepted axis has |t - level| < 1/2 - (2 - 2^-25) 2^-24 < 1/2 - 2^-30 for the f64 t as
                                      well: the f64 certificate accepts it too, with the same level (NaN / out of range saturate
                                      onto a clamped end, accepted on both sides); a group with an axis inside 2^-23 takes the f64
                                      certificate above, unchanged, and behind it the table search); likewise for a
                                      four-point constellation with one point per quadrant at (+-a, +-b) -- QPSK -- decided by the
                                      signs (demod_quad_cert: certified for 2^-30 min(a, b) <= |re|, |im| <= 2^8 max(a, b)), and for
                                      8- / 16-PSK inside the table search itself (demod_psk_cert: the sector by sign masks and one
                                      compare per sector boundary of an octant, certified at an angular margin of 2^-28
                                      (complex64: 2^-12) inside a magnitude window of 2^-8 .. 2^8 (1/8 .. 8) radii) */
    MCLE_OPT_F64_VARIANT = 11,     /* (builds with -DMCLE_EXPERIMENTS only; the product library accepts 0 and refuses anything else)
                                      complex128 config-4 kernel (1024, 4x4), TIMING BOUNDS ONLY on its 512-thread radix-4 form --
                                      results are wrong by construction: bit 0 = the LDS stores of the last transmit stage and of
                                      the channel stage dropped, bit 1 = the two workgroup barriers around the channel stage
                                      dropped */
    MCLE_OPT_F32_MFMA = 12,        /* complex64 config 4 at (1024, 4x4): 1 = the matrix-core kernel k_run_mimo_ofdm_mfma (the default of
                                      rounds 2-3) instead of the planar VALU family (k_run_mimo_ofdm_planar<float>: the complex128
                                      kernels on planes of floats, 10-20 % faster at this geometry and the only fast complex64 kernel
                                      at every other one; default since round 4) */
    MCLE_OPT_TDL_KERNEL = 13,      /* config 3 at fft_size 256 / 512 / 1024 / 2048 with <= 8 taps reaching <= 256 samples back (inside the cyclic prefix or,
                                      since round 6, beyond it; polynomial order <= 8): 0 = one realization per WAVEFRONT (k_run_ofdm_tdl_wave: no
                                      workgroup barrier in the loop; radix-16 register passes at 1024, radix-4 stages otherwise) WHERE IT
                                      IS THE FASTER KERNEL (1024; 2048 in complex64; 256 / 512 in complex128 -- default since round 4),
                                      1 = the batched kernels of rounds 1-3 everywhere (four / two realizations per workgroup pass;
                                      complex64 at 1024: matrix cores), 2 = the wavefront kernel wherever it exists, 3 = the same, but at
                                      2048 points the one-wavefront kernel instead of the round-6 default there, TWO wavefronts per
                                      realization (k_run_ofdm_tdl_hw: every delay inside the prefix, orders 2 .. 5; A/B), 4 = as 2 with
                                      the complex64 registers at 1024 bounded for four wavefronts per SIMD instead of three (A/B) */
    MCLE_OPT_MIMO_TDL_KERNEL = 14, /* frequency-selective MIMO-OFDM (mcle_run_mimo_ofdm_tdl) at fft_size 256 / 512 / 1024 / 2048 with <= 8 taps
                                      reaching <= min(256, fft_size / 2) samples back (inside the cyclic prefix or, since round 6, beyond it): 0 = one receive antenna per WAVEFRONT
                                      (k_run_mimo_ofdm_tdl_wave, every 1 <= Nt <= Nr <= 4; default since round 5), 1 = the
                                      workgroup-cooperative kernel of rounds 1-4 (Nt = Nr in {2, 4}), 2 = the wavefront kernels with the
                                      tap polynomials' order at run time also where the parked-coefficient kernel applies (A/B) */
    MCLE_OPT_WALK_LEGACY = 15,     /* symbol walks of mcle_run_ia / mcle_run_bd (either arithmetic) with an even number of columns >= 128 (and, for
                                      block diagonalisation, two or three users of <= 2 antennas): 0 = the packed walk of round 6
                                      (csrc/walk_f64.hpp: the lane pairs of a chunk of realizations as one index space, decision form
                                      fixed at compile time, records in LDS), 1 = the per-realization walks of rounds 2-5 (A/B and
                                      kernel-vs-kernel tests: identical counters) */
    MCLE_OPT_STAGED_GENERIC = 16,  /* 1: every staged operator with more than one form (mcle_ctx_last_kernel lists them) takes its
                                      generic form whatever the pointers and the shape (A/B and form-vs-form tests) */
    MCLE_OPT_CODEBOOK_NO_PACK = 17, /* 1: the codebook kernels (mcle_chordal_min_dist, mcle_codebook_generate, mcle_run_codebook_search) take one
                                      candidate per wavefront trip whatever its size (form-vs-form tests: identical outputs) */
    MCLE_OPT_COUNT = 18
};
int mcle_ctx_set_option(mcle_ctx* ctx, int option, long long value);
int mcle_ctx_get_option(mcle_ctx* ctx, int option, long long* value);

/* kernel timing on the context stream with HIP events (used by bench.py's roofline leg) */
int mcle_timer_start(mcle_ctx* ctx);
int mcle_timer_stop_ms(mcle_ctx* ctx, float* ms);                               /* blocks */

/* What the box's HBM delivers to a streaming kernel, measured by the library (csrc/kernels_hbm.hip): `reps` launches of a
 * 16-byte-per-access grid-stride kernel over arrays of `bytes` bytes each (in the context's scratch), n_cu * blocks_per_cu
 * workgroups of 256 threads; *gbps = bytes moved (read + written) per second / 1e9.  The denominator of the
 * "fraction of the achievable HBM rate" figures of bench.py (both the 8 TB/s specification and the rate
 * measured on the box are quoted).  Nothing in the reference corresponds to it. */
enum { MCLE_HBM_COPY = 0, MCLE_HBM_READ = 1, MCLE_HBM_TRIAD = 2, MCLE_HBM_WRITE = 3,
       MCLE_HBM_NONTEMPORAL = 4 /* | : non-temporal loads / stores */, MCLE_HBM_UNROLL8 = 8 /* | : eight accesses in flight per thread instead of four */ };
int mcle_hbm_stream_rate(mcle_ctx* ctx, int kind, size_t bytes, int reps, int blocks_per_cu, double* gbps);

/* ---- multi-GPU: realization sharding + ONE all-reduce of the integer counters.
 *      The reference's only multi-process mechanism is ipyparallel, one parameter variation per engine
 *      (simulations/runner.py:1836-1846 simulate_in_parallel); here every rank takes a slice of every
 *      variation (realizations are addressed by index) and the exact integer sums are reduced over RCCL / xGMI.
 *      One process and one context per GPU.  RCCL is bound at run time (dlopen), so a host without it can still
 *      load the library; mcle_comm_load names the librccl to use (NULL: librccl.so.1 as the loader finds it --
 *      the copy PyTorch has loaded, if any). ------------------------------------------------------------------ */
int mcle_comm_load(const char* rccl_path);
/* rank 0 draws the 128-byte id (ncclGetUniqueId) and hands it to the other ranks by any means (a socket, a file,
 * MPI, torch.distributed ...); every rank then joins.  world == 1 is allowed (all-reduces become no-ops).
 * Draw an id only to use it: RCCL starts a bootstrap listener per id that ends when all ranks have joined. */
int mcle_comm_unique_id(void* id_out, size_t bytes);
int mcle_comm_init(mcle_ctx* ctx, const void* unique_id, int rank, int world);
int mcle_comm_destroy(mcle_ctx* ctx);
int mcle_comm_info(mcle_ctx* ctx, int* rank, int* world);
/* in place, on the context stream: words 0..5 of each of the n blocks are summed over the ranks
 * (ncclUint64 / ncclSum -- exact, order independent), n_symbols / n_bits take the maximum (they are
 * per-realization constants, zero on a rank whose shard was empty).  No-op without a communicator. */
int mcle_counters_allreduce(mcle_ctx* ctx, mcle_counters* d_counters, int n);
/* sum of n doubles over the ranks, in place (the 'sum_capacity' style side results of the IA application) */
int mcle_allreduce_f64(mcle_ctx* ctx, double* d_values, size_t n);

/* ---- pointers of the operators below: any element-aligned device pointer is accepted (8 bytes for complex64, 16 for complex128,
 *      4 for int32 labels, 1 for byte labels), views into a larger allocation included.  An operator picks its form from the
 *      pointers and the shape (mcle_ctx_last_kernel names it; MCLE_OPT_STAGED_GENERIC forces the generic one); the values do not
 *      depend on that choice, bit for bit, except for mcle_mimo_channel_philox in complex64, whose 4x4 pair form adds the noise
 *      before the products (the other forms after the sum: a rounding-level difference). ------------------------------- */

/* ---- constellation (a1: modulators/fundamental.py:131-146 setConstellation, :396-448 PSK,
 *      :659-777 QAM; the table itself is built by the host mirror) ----------------------- */
int mcle_set_constellation(mcle_ctx* ctx, const double* re_im, int M, int kind);

/* Host only (no device needed): the candidate grid the f32 min-distance kernels search instead of all M points
 * (DESIGN.md section 5.1).  cells [32*32] receives G*G words: byte 0 = number of candidates (0xFF: search
 * everything), bytes 1..7 = candidate indices in ascending order; cell (ix, iy) covers
 * [x0 + ix*h, x0 + (ix+1)*h) x [y0 + iy*h, ...), border cells extending to infinity.  2 <= M <= 256. */
int mcle_build_demod_grid(const double* re_im, int M, int* G, double* x0, double* y0, double* h,
                          unsigned long long* cells);

/* ---- a2/a3/a4: Modulator.modulate / demodulate (fundamental.py:175-248), count_bit_errors
 *      (util/misc.py:519-566) and the symbol-error count of user code --------------------- */
int mcle_modulate(mcle_ctx* ctx, int dtype, const int32_t* d_idx, void* d_out, size_t n);
int mcle_demodulate(mcle_ctx* ctx, int dtype, int method, const void* d_rx, int32_t* d_idx,
                    size_t n);
/* n_real blocks of n_per_real indices each; adds into d_counters[0] (may be NULL) and, when
 * non-NULL, writes per-realization counts d_sym_err[n_real] / d_bit_err[n_real]. */
int mcle_count_errors(mcle_ctx* ctx, const int32_t* d_tx_idx, const int32_t* d_rx_idx,
                      size_t n_per_real, size_t n_real, int bits_per_symbol,
                      mcle_counters* d_counters, uint32_t* d_sym_err, uint32_t* d_bit_err);
/* fused demodulate + count (no index array written) */
int mcle_demod_count(mcle_ctx* ctx, int dtype, int method, const void* d_rx,
                     const int32_t* d_tx_idx, size_t n_per_real, size_t n_real,
                     mcle_counters* d_counters, uint32_t* d_sym_err, uint32_t* d_bit_err);
/* the same against byte labels (mcle_rand_modulate_batch_u8) */
int mcle_demod_count_u8(mcle_ctx* ctx, int dtype, int method, const void* d_rx,
                        const uint8_t* d_tx_idx, size_t n_per_real, size_t n_real,
                        mcle_counters* d_counters, uint32_t* d_sym_err, uint32_t* d_bit_err);

/* ---- a5: randn_c (util/misc.py:327-355) under the mcle-philox-v1 contract, and AWGN ----- */
/* out[i] = sqrt(variance) * CN(0,1) sample (first_sample + i) of (seed, realization, stream) */
int mcle_randn_c(mcle_ctx* ctx, int dtype, uint64_t seed, uint64_t realization, uint32_t stream,
                 uint64_t first_sample, double variance, void* d_out, size_t n);
int mcle_rand_symbols(mcle_ctx* ctx, uint64_t seed, uint64_t realization, uint64_t first_symbol,
                      int M, int32_t* d_idx, size_t n);
/* y = x + sqrt(noise_var) * noise (injected noise array: parity against golden vectors) */
int mcle_awgn_add(mcle_ctx* ctx, int dtype, const void* d_x, const void* d_noise,
                  double noise_var, void* d_y, size_t n);

/* ---- a6/a9: JakesSampleGenerator (channels/fading_generators.py:289-553) and
 *      TdlChannel.corrupt_data (channels/fading.py:1046-1124) --------------------------- */
/* h[s, n] = L^-1/2 sum_l exp(j(2 pi Fd cos(phi[l,s]) t_n + psi[l,s])) * sqrt(tap_power[s]),
 * t_n = t0 + n*dt.  phi/psi: host doubles [L, n_streams]; tap_power: host [n_streams] or NULL. */
int mcle_jakes_generate(mcle_ctx* ctx, int dtype, const double* phi, const double* psi, int L,
                        int n_streams, double Fd, double t0, double dt, const double* tap_power,
                        void* d_h, size_t n_samples);
/* same, at explicit sample times (block-static use of TdlChannel.corrupt_data_in_freq_domain) */
int mcle_jakes_generate_at(mcle_ctx* ctx, int dtype, const double* phi, const double* psi, int L,
                           int n_streams, double Fd, const double* times, const double* tap_power,
                           void* d_h, size_t n_samples);
/* SISO time-varying sparse convolution: y[d_i + n] += g[i, n] x[n]; y has n + max_delay */
int mcle_tdl_apply(mcle_ctx* ctx, int dtype, const void* d_x, const void* d_taps,
                   const int32_t* delays, int n_taps, void* d_y, size_t n);
/* MIMO branch of corrupt_data (fading.py:1107-1117): x [nt][n], taps [n_taps][nr][nt][n] ->
 * y [nr][n + max_delay] */
int mcle_tdl_apply_mimo(mcle_ctx* ctx, int dtype, const void* d_x, const void* d_taps,
                        const int32_t* delays, int n_taps, int nr, int nt, void* d_y, size_t n,
                        size_t batch);
/* per-OFDM-symbol mean frequency response on the used subcarriers for n_links parallel links:
 * taps [n_taps][n_links][n_sym*(fft+cp)] -> H [n_sym][num_used][n_links]
 * (TdlImpulseResponse.get_freq_response fading.py:513-536 averaged like ofdm.py:545-547).
 * num_used = -g (g >= 1): all fft_size bins in natural order, averaging groups of g samples
 * (taps [n_taps][n_links][n_sym*g]); g = 1 is the per-block response of corrupt_data_in_freq_domain. */
int mcle_tdl_mean_freq_response(mcle_ctx* ctx, int dtype, const void* d_taps, const int32_t* delays,
                                int n_taps, int n_links, size_t n_sym, int fft_size, int cp_size,
                                int num_used, void* d_H, size_t batch);
/* batched Jakes taps with the phases drawn on-chip (PHASE stream of realization first + r, draw order of
 * fading_generators.py:421-425): taps [count][n_streams][n]; stream_amp = sqrt(tap power / L) per stream */
int mcle_jakes_taps_philox(mcle_ctx* ctx, int dtype, uint64_t seed, uint64_t first, uint64_t count,
                           int L, int n_streams, double Fd, double t0, double dt,
                           const double* stream_amp, void* d_taps, size_t n_samples);
/* y[r][i] = x[r][i] + sqrt(noise_var) * CN(0,1) sample i of (seed, first + r, NOISE); rows of row_len */
int mcle_awgn_philox(mcle_ctx* ctx, int dtype, const void* d_x, uint64_t seed, uint64_t first,
                     uint64_t count, size_t row_len, double noise_var, void* d_y);
/* out[r][i] = sqrt(variance) * CN(0,1) sample i of (seed, first + r, stream): mcle_randn_c for a batch of realizations
 * (e.g. the flat channel matrices H = randn_c(Nr, Nt) of count realizations from the CHAN stream,
 * apps/mimo/simulate_mimo.py:78) */
int mcle_randn_c_batch(mcle_ctx* ctx, int dtype, uint64_t seed, uint64_t first, uint64_t count,
                       uint32_t stream, size_t row_len, double variance, void* d_out);
/* d_idx[r][i] = symbol i of realization first_realization + r (DATA stream) */
int mcle_rand_symbols_batch(mcle_ctx* ctx, uint64_t seed, uint64_t first_realization, uint64_t count,
                            int M, int32_t* d_idx, size_t n);
/* mcle_rand_symbols_batch + mcle_modulate in one pass (the "gen + modulate" operator of SURVEY 8(d)'s staged model, one
 * write of the labels and one of the samples): d_idx[r][i] as above for the bound constellation's M, d_sym[r][i] =
 * table[d_idx[r][i]] (randint + Modulator.modulate, modulators/fundamental.py:175-199) */
int mcle_rand_modulate_batch(mcle_ctx* ctx, int dtype, uint64_t seed, uint64_t first_realization, uint64_t count,
                             int32_t* d_idx, void* d_sym, size_t n);
/* the same with BYTE labels (M <= 256): SURVEY 8(d)'s staged model counts an index as one byte; the int32 form above moves
 * four.  Consumed by mcle_demod_count_u8. */
int mcle_rand_modulate_batch_u8(mcle_ctx* ctx, int dtype, uint64_t seed, uint64_t first_realization, uint64_t count,
                                uint8_t* d_idx, void* d_sym, size_t n);
/* element-wise complex product (frequency-domain channel application, fading.py:1259) */
int mcle_cmul(mcle_ctx* ctx, int dtype, const void* d_a, const void* d_b, void* d_out, size_t n);
/* element-wise complex divide (flat-fading equalisation y / h of the C2 template) */
int mcle_cdiv(mcle_ctx* ctx, int dtype, const void* d_num, const void* d_den, void* d_out,
              size_t n);

/* ---- a11/a10: OFDM.modulate / demodulate (modulators/ofdm.py:394-466) and
 *      OfdmOneTapEqualizer.equalize_data (ofdm.py:515-552) ------------------------------- */
/* n_in data symbols (zero padded to n_sym*num_used) -> n_sym*(fft+cp) samples; batch rows */
int mcle_ofdm_modulate(mcle_ctx* ctx, int dtype, const void* d_in, size_t n_in, int fft_size,
                       int cp_size, int num_used, void* d_out, size_t batch);
/* n_sym*(fft+cp) samples -> n_sym*num_used symbols; batch rows */
int mcle_ofdm_demodulate(mcle_ctx* ctx, int dtype, const void* d_in, size_t n_sym, int fft_size,
                         int cp_size, int num_used, void* d_out, size_t batch);
/* d_taps [n_taps, n_sym*(fft+cp)] sparse taps of the samples the OFDM symbols rode on */
int mcle_onetap_equalize(mcle_ctx* ctx, int dtype, const void* d_data, const void* d_taps,
                         const int32_t* delays, int n_taps, size_t n_sym, int fft_size,
                         int cp_size, int num_used, void* d_out);

/* ---- a12: Blast (mimo/mimo.py:465-660) --------------------------------------------------- */
/* x[n] -> X[a, c] = x[c*nt + a] / sqrt(nt)   (encode, :639-641); batch rows of n */
int mcle_blast_encode(mcle_ctx* ctx, int dtype, const void* d_x, int nt, size_t n, void* d_X,
                      size_t batch);
/* G = sqrt(nt) * solve(H^H H + noise_var I, H^H) per batch item (noise_var = 0: ZF / pinv for
 * full column rank); d_H [batch, nr, nt] row-major, d_G [batch, nt, nr]; d_skipped[batch]
 * (may be NULL) is 1 iff A = H^H H + noise_var I is numerically rank deficient in the CALL's
 * arithmetic, and then G means nothing: some Cholesky pivot is <= tol * A[j][j] (or not a number),
 * tol = 2^-42 for MCLE_F64 and 2^-34 for MCLE_F32 (a complex64 H is a rank-deficient one moved by
 * eps32).  pivot_j / A[j][j] >= 1 / cond(A), so a channel with cond(H) <= 1e6 (MCLE_F64) or <= 1e2
 * (MCLE_F32) is never flagged at noise_var = 0, and none with noise_var >= 2 tol nr max|h|^2.
 * Accuracy: the MMSE filter is within a small multiple of NumPy's solve at the same dtype.  The ZF
 * filter comes from the normal equations, not from a pseudo-inverse, so it may lose ONE more power
 * of the condition number than numpy.linalg.pinv at the same dtype and no more:
 * |G - G_exact|_max <= 8 cond(H) max(|pinv_dtype - G_exact|_max, eps_dtype |G_exact|_max).
 * Magnitudes: the squared column norms must stay inside the double range (|h| from 1e-150 to 1e150). */
int mcle_blast_filter(mcle_ctx* ctx, int dtype, const void* d_H, int nr, int nt,
                      double noise_var, void* d_G, uint32_t* d_skipped, size_t batch);
/* est[c*nt + a] = sum_r G[a, r] Y[r, c]      (decode, :658-660) */
int mcle_blast_decode(mcle_ctx* ctx, int dtype, const void* d_G, const void* d_Y, int nr, int nt,
                      size_t ns, void* d_est, size_t batch);
/* one receive filter per column (per-subcarrier MMSE): G [b][ns][nt][nr], Y [b][nr][ns] -> est[b][c*nt + a] */
int mcle_blast_decode_per_subcarrier(mcle_ctx* ctx, int dtype, const void* d_G, const void* d_Y,
                                     int nr, int nt, size_t ns, void* d_est, size_t batch);
/* Y = H X  (+ sqrt(noise_var) * noise when d_noise != NULL): apps/mimo/simulate_mimo.py:96-98 */
int mcle_mimo_channel(mcle_ctx* ctx, int dtype, const void* d_H, const void* d_X,
                      const void* d_noise, double noise_var, int nr, int nt, size_t ns, void* d_Y,
                      size_t batch);
/* the same with the noise drawn on-chip: Y[b][r][c] = sum_a H[b][r][a] X[b][a][c] + sqrt(noise_var) * CN(0,1)
 * sample r*ns + c of (seed, first + b, NOISE) -- the (Nr, Ns) row-major randn_c of simulate_mimo.py:97 under the
 * mcle-philox-v1 contract; one pass over X and Y (the "H T + awgn" operator of SURVEY.md 8(d)'s staged model) */
int mcle_mimo_channel_philox(mcle_ctx* ctx, int dtype, const void* d_H, const void* d_X, uint64_t seed,
                             uint64_t first, double noise_var, int nr, int nt, size_t ns, void* d_Y,
                             size_t batch);

/* ---- a13: further MIMO schemes of mimo/mimo.py ---------------------------------------------- */
/* Alamouti (mimo.py:1168-1269): x [batch][n] -> X [batch][2][n] (n even); decode with H [batch][nr][2] */
int mcle_alamouti_encode(mcle_ctx* ctx, int dtype, const void* d_x, size_t n, void* d_X,
                         size_t batch);
int mcle_alamouti_decode(mcle_ctx* ctx, int dtype, const void* d_H, const void* d_Y, int nr, size_t n,
                         void* d_out, size_t batch);
/* MRT (mimo.py:666-783), MISO h [batch][nt]: X = exp(-1j angle(h)).T / sqrt(nt) * x; decode y * sqrt(nt)/sum|h| */
int mcle_mrt_encode(mcle_ctx* ctx, int dtype, const void* d_h, const void* d_x, int nt, size_t n,
                    void* d_X, size_t batch);
int mcle_mrt_decode(mcle_ctx* ctx, int dtype, const void* d_h, const void* d_y, int nt, size_t n,
                    void* d_out, size_t batch);
/* SVDMimo (mimo.py:833-946), square H [batch][n][n]: W = V/sqrt(n) (precoder), G = diag(1/S) U^H sqrt(n)
 * (receive filter), S descending (d_S may be NULL, always double).  encode = W @ x.reshape(n,-1), decode = G @ Y
 * via mcle_mimo_channel.  One-sided Jacobi in f64 for both dtypes; every threshold is relative, so H times a power of
 * two gives S times it, the same W bit for bit and G divided by it.  Supported magnitudes: 1e-150 < |h| < 1e150 --
 * the routine works on squared column norms, which underflow or overflow outside that range and then S is silently
 * wrong; scale such channels first.  No flag: a zero singular value gives a row of G that is not finite (diag(1/S),
 * as the reference), S, W and the other rows of G stay valid. */
int mcle_svd_filters(mcle_ctx* ctx, int dtype, const void* d_H, int n_ant, void* d_W, void* d_G,
                     double* d_S, size_t batch);

/* GMDMimo (mimo.py:952-1067) + util.misc.gmd (misc.py:18-159), square H: W = P/sqrt(n), G = Blast filter
 * (ZF for noise_var = 0, else MMSE) on the equivalent channel Q R; d_R [batch][n][n] (real upper
 * triangular with constant diagonal; may be NULL).  d_skipped[batch] (may be NULL) is 1 iff H is numerically rank
 * deficient in the call's arithmetic, and then W, G and R mean nothing: sigma_min <= sqrt(tol) sigma_max (the
 * decomposition divides by the geometric mean of the singular values whatever noise_var is), or the filter's system
 * Heq^H Heq + noise_var I is flagged as in mcle_blast_filter (the same tol, the same Cholesky and the same ZF accuracy
 * contract, on Heq = Q R).  So cond(H) <= 1e6 (MCLE_F64) / 1e2 (MCLE_F32) is never flagged.  With a repeated singular
 * value or one AT the geometric mean R is one of several valid factors (the rotation is 0/0 and is skipped or taken at
 * an arbitrary angle): triangular, constant diagonal, Q and P unitary hold, the entries are not unique.  Magnitudes as
 * mcle_svd_filters, and the product of the singular values must stay inside the double range. */
int mcle_gmd_filters(mcle_ctx* ctx, int dtype, const void* d_H, int n_ant, double noise_var, void* d_W,
                     void* d_G, double* d_R, uint32_t* d_skipped, size_t batch);
/* calc_post_processing_linear_SINRs (mimo/mimo.py:62-118; MimoBase.calc_linear_SINRs :311-345): complex128
 * H [batch][nr][nt], precoder W [batch][nt][ns], receive filter G_H [batch][ns][nr] -> linear SINR [batch][ns]:
 * |E_ii|^2 / (|sum_{j != i} E_ij|^2 + noise_var ||G_H row i||^2) with E = G_H H W (the reference's formula,
 * modulus of the summed off-diagonal entries included). */
int mcle_post_processing_sinrs(mcle_ctx* ctx, const void* d_H, const void* d_W, const void* d_G, double noise_var,
                               int nr, int nt, int ns, double* d_sinr, size_t batch);

/* ---- K-user interference channel: covariance matrices and post-filter SINRs ------------------
 * MultiUserChannelMatrix / MultiUserChannelMatrixExtInt (channels/multiuser.py): calc_Q / calc_JP_Q (:1314-1450,
 * :2530-2634), _calc_Bkl_cov_matrix_all_l and its JP form (:1452-1826, :2676-2742), calc_SINR / calc_JP_SINR
 * (:1828-2008, :2636-2807), calc_cov_matrix_extint_plus_noise (:2469-2520), path loss on the block matrix (:1264-1312).
 * complex128.  d_bigH [batch][sum nr][sum nt + n_ext]; d_pathloss (may be NULL) [sum nr][sum nt + n_ext] LINEAR power
 * ratio per entry (the reference's _pathloss_big_matrix; shared by the batch); d_F [batch][K][16][4]: user j's
 * precoder in the top-left corner (nt[j] x ns[j], or (sum nt) x ns[j] when `joint`); d_U [batch][K][4][4]
 * (nr[k] x ns[k], may be NULL).  Outputs (each may be NULL), zero padded: d_Q [batch][K][4][4] interference from
 * the other users + Re_k; d_Re [batch][K][4][4] = pe ext ext^H + noise_var I; d_B [batch][K][4][4][4] (stream l:
 * everything received minus stream l's own covariance); d_sinr [batch][K][4] (linear).
 * Edges: a user with ns[k] = 0 contributes nothing and gets zero B / sinr rows; d_F may be NULL only when no user has
 * streams; d_sinr needs d_U; a zero path-loss entry removes that link exactly; noise_var = 0 and n_ext = 0 give Re = 0
 * exactly; a refused call and batch = 0 write nothing.  Accuracy: every entry is within c eps of its MAGNITUDE (the
 * same formula on absolute values), c the length of the accumulation chain (81 for Q at sum Nt = 16 in joint mode with a path loss);
 * B_kl = (sum) - g g^H is formed by subtraction, so where one stream dominates it is accurate relative to the sum, not
 * to the difference.  tests/test_gpu_multiuser_envelope.py holds this against a 50-digit oracle. */
typedef struct mcle_mu_stats_cfg {
    int32_t K;                  /* users (with receive antennas), <= 4 */
    int32_t n_ext;              /* external interferer antennas: trailing columns of big_H, <= 8 */
    int32_t joint;              /* 0: per-link precoders (calc_Q, calc_SINR); 1: joint processing (calc_JP_*) */
    int32_t reserved;
    int32_t nr[4], nt[4], ns[4];
    double noise_var;           /* 0: no noise term */
    double pe;                  /* power of the external interference */
} mcle_mu_stats_cfg;
int mcle_mu_link_stats(mcle_ctx* ctx, const mcle_mu_stats_cfg* cfg, const void* d_bigH, const double* d_pathloss,
                       const void* d_F, const void* d_U, void* d_Q, void* d_Re, void* d_B, double* d_sinr,
                       size_t batch);

/* ---- fused pipelines: whole realizations on-chip (randomness: mcle-philox-v1) ----------- */
typedef struct mcle_awgn_cfg {          /* C1: apps/awgn_modulators/simulate_psk.py:51-115 */
    int32_t n_symbols;
    int32_t demod_method;
    double noise_var;
} mcle_awgn_cfg;

typedef struct mcle_flat_cfg {          /* C2: flat Jakes fading, y = h s + n, equalise y/h */
    int32_t n_symbols;
    int32_t demod_method;
    double noise_var;
    double Fd, Ts;
    int32_t L;
    int32_t rayleigh_iid;               /* 1: h ~ randn_c per sample (RayleighSampleGenerator) */
} mcle_flat_cfg;

#define MCLE_MAX_TAPS 24
typedef struct mcle_ofdm_tdl_cfg {      /* C3: notebooks/TDL_and_OFDM.ipynb OfdmTdlSimulator */
    int32_t fft_size, cp_size, num_used, n_ofdm_sym;
    int32_t demod_method;
    int32_t n_taps;
    int32_t L;
    int32_t reserved;
    double noise_var;
    double Fd, Ts;
    double tap_power[MCLE_MAX_TAPS];    /* linear, discretised profile (sum 1) */
    int32_t tap_delay[MCLE_MAX_TAPS];   /* sample indexes, increasing */
} mcle_ofdm_tdl_cfg;

typedef struct mcle_mimo_ofdm_cfg {     /* C4: apps/mimo/simulate_mimo.py:68-142 + OFDM */
    int32_t nt, nr;
    int32_t fft_size, cp_size, num_used, n_ofdm_sym;
    int32_t demod_method;
    int32_t mmse;                       /* 1: Blast.set_noise_var(noise_var); 0: zero forcing */
    double noise_var;
} mcle_mimo_ofdm_cfg;

typedef struct mcle_mimo_ofdm_tdl_cfg { /* TdlMimoChannel (fading.py:1290-1333) + per-antenna OFDM +
                                         * one Blast filter per used subcarrier (mimo.py:577-607) */
    int32_t nt, nr;                     /* fused: every 1 <= nt <= nr <= 4 at fft_size 256 .. 2048 with the last delay <= min(256, fft_size / 2)
                                         * (inside the prefix or beyond it); nt == nr in {2, 4} at 64 .. 2048 otherwise */
    int32_t fft_size, cp_size, num_used, n_ofdm_sym;
    int32_t demod_method;
    int32_t mmse;                       /* 1: MMSE with noise_var; 0: zero forcing */
    int32_t n_taps, L;                  /* discretised profile taps; Jakes rays per fading process */
    double noise_var, Fd, Ts;
    double tap_power[MCLE_MAX_TAPS];    /* linear */
    int32_t tap_delay[MCLE_MAX_TAPS];   /* samples, ascending, < fft_size */
} mcle_mimo_ofdm_tdl_cfg;

enum { MCLE_MIMO_BLAST = 0,     /* mimo.Blast     mimo/mimo.py:463-660   (Nt <= Nr <= 4) */
       MCLE_MIMO_MRC = 1,       /* mimo.MRC       mimo/mimo.py:789-830   (Nt = 1)        */
       MCLE_MIMO_MRT = 2,       /* mimo.MRT       mimo/mimo.py:666-783   (Nr = 1)        */
       MCLE_MIMO_ALAMOUTI = 3,  /* mimo.Alamouti  mimo/mimo.py:1073-1287 (Nt = 2)        */
       MCLE_MIMO_SVD = 4,       /* mimo.SVDMimo   mimo/mimo.py:833-946   (square, 2..4)  */
       MCLE_MIMO_GMD = 5 };     /* mimo.GMDMimo   mimo/mimo.py:952-1067  (square, 2..4)  */

typedef struct mcle_mimo_flat_cfg {     /* apps/mimo/simulate_mimo.py:68-142: flat H = randn_c(Nr, Nt), single carrier */
    int32_t scheme;                     /* MCLE_MIMO_* */
    int32_t nt, nr;
    int32_t n_symbols;                  /* NSymbs per layer (layers: Nt for Blast / MRC / SVD / GMD, 1 otherwise) */
    int32_t demod_method;
    int32_t mmse;                       /* Blast / MRC / GMD: 1 = set_noise_var(noise_var); 0 = zero forcing (the app) */
    double noise_var;
} mcle_mimo_flat_cfg;

enum { MCLE_IA_CLOSED_FORM = 0,  /* ClosedFormIASolver      ia/algorithms.py:42-265    */
       MCLE_IA_ALT_MIN = 1,      /* AlternatingMinIASolver  ia/algorithms.py:885-1129  */
       MCLE_IA_MIN_LEAKAGE = 2,  /* MinLeakageIASolver      ia/algorithms.py:1132-1240 */
       MCLE_IA_MAX_SINR = 3,     /* MaxSinrIASolver         ia/algorithms.py:1243-1507 */
       MCLE_IA_MMSE = 4 };       /* MMSEIASolver            ia/algorithms.py:1510-1850 */

enum { MCLE_IA_INIT_GIVEN = 0,        /* 'random' (pipelines: drawn on-chip) or 'fix' (operator: injected) */
       MCLE_IA_INIT_CLOSED_FORM = 1,  /* 'closed_form': F and W of ClosedFormIASolver                      */
       MCLE_IA_INIT_ALT_MIN = 2,      /* 'alt_min': AlternatingMinIASolver run first, same max_iterations */
       MCLE_IA_INIT_SVD = 3 };        /* 'svd': dominant right singular vector of each direct channel (phase: ours) */

typedef struct mcle_ia_cfg {            /* C5: apps/ia/simulate_ia.py:94-245, ClosedFormIASolver */
    int32_t K, nr, nt, ns;              /* supported: K = 3, nr = nt = 2, ns = 1 */
    int32_t n_symbols;                  /* NSymbs per stream */
    int32_t demod_method;
    double noise_var;
    int32_t solver;                     /* MCLE_IA_*: closed form or an iterative solver (initialize_with='random') */
    int32_t max_iterations;             /* iterative solvers: IterativeIASolverBaseClass.max_iterations */
    double relative_factor;             /* ... and .relative_factor (algorithms.py:316-322) */
    int32_t initialize_with;            /* MCLE_IA_INIT_*: 'random' / 'closed_form' / 'alt_min' / 'svd' (algorithms.py:633-663) */
    int32_t reserved;
} mcle_ia_cfg;

/* Each run_* processes realizations [first, first+count) of `seed`, ADDS into d_counters[0]
 * and, when non-NULL, writes per-realization d_sym_err / d_bit_err [count]. */
int mcle_run_awgn(mcle_ctx* ctx, int dtype, const mcle_awgn_cfg* cfg, uint64_t seed,
                  uint64_t first, uint64_t count, mcle_counters* d_counters,
                  uint32_t* d_sym_err, uint32_t* d_bit_err);
/* Jakes fading (JakesSampleGenerator, fading_generators.py:427-493) in the complex128 instantiation: by default the ray
 * phasors of a thread's run of 16 symbols advance by a rotation recurrence (one exact sincos per ray and run, then <= 15
 * complex products: <= 3e-15 relative drift against evaluating sin / cos at every sample, which is what NumPy does).  The
 * per-realization error counts equal the oracle's on every tested case incl. the full 10^5-symbol config 2, but that is by
 * test coverage, not by construction: a symbol within 3e-15 of a decision boundary may flip.  MCLE_OPT_JAKES_DIRECT = 1
 * evaluates every sample (the literal parity statement, 3.3 x slower).  Fd may have either sign (as in the reference) and must be
 * finite. */
int mcle_run_flat_fading(mcle_ctx* ctx, int dtype, const mcle_flat_cfg* cfg, uint64_t seed,
                         uint64_t first, uint64_t count, mcle_counters* d_counters,
                         uint32_t* d_sym_err, uint32_t* d_bit_err);
/* Config 3.  Fd may have either sign (as in the reference's JakesSampleGenerator; the kernels use |Fd| wherever they choose by
 * it) and must be finite.  Kernel chain (mcle_ctx_last_kernel names the one that ran): at 2048 points the two-wavefront kernel takes
 * every delay inside the prefix at polynomial orders 2 .. 5; a delay beyond the prefix (dmax > cp_size) falls back to the
 * one-wavefront kernel, which takes <= 8 taps reaching <= min(256, fft_size / 2) samples back at orders 2 .. 5 (2 .. 8 at 1024);
 * then the batched kernels (orders <= 12, delays < fft_size; complex64 at 1024 with every delay inside the prefix: the matrix-core
 * kernel first), then the one-realization-per-workgroup kernel.  All of them give the same counts (complex128: exactly).
 * complex64 counts can change with n_ofdm_sym alone: the quarter-turn rule at mcle_run_mimo_ofdm_tdl counts every symbol of the
 * run, so adding symbols can move the rays' frequencies from float to double for the symbols already there. */
int mcle_run_ofdm_tdl(mcle_ctx* ctx, int dtype, const mcle_ofdm_tdl_cfg* cfg, uint64_t seed,
                      uint64_t first, uint64_t count, mcle_counters* d_counters,
                      uint32_t* d_sym_err, uint32_t* d_bit_err);
/* Envelope: 1 <= Nt <= Nr <= 4, either arithmetic: fft_size 256 / 512 / 1024 / 2048 with every Nt <= Nr (Blast takes any Nr x Nt,
 * mimo/mimo.py:264-309) on the planar kernel family (pipeline_mimo_planar.hip; in complex128 2048 with 4 receive antennas exists
 * there only: 148 KiB of LDS) -- Nr >= 2: the family has no 1x1 geometry, which is refused at every size; 2x2 / 4x4 at 64 and 128 on
 * the generic kernel.  complex64 at (1024, 4x4): the planar radix-16
 * kernel by default, the matrix-core kernel with MCLE_OPT_F32_MFMA = 1.  Anything else: MCLE_E_INVAL. */
int mcle_run_mimo_ofdm(mcle_ctx* ctx, int dtype, const mcle_mimo_ofdm_cfg* cfg, uint64_t seed,
                       uint64_t first, uint64_t count, mcle_counters* d_counters,
                       uint32_t* d_sym_err, uint32_t* d_bit_err);

/* The reference's MIMO application, any of its six schemes, fused.  max(nt, nr) * n_symbols <= 2^31 - 1 (draw positions are
 * 32-bit) and count <= 2^31 - 1 per call; anything else: MCLE_E_INVAL. */
int mcle_run_mimo_flat(mcle_ctx* ctx, int dtype, const mcle_mimo_flat_cfg* cfg, uint64_t seed,
                       uint64_t first, uint64_t count, mcle_counters* d_counters,
                       uint32_t* d_sym_err, uint32_t* d_bit_err);

/* The flat Blast link of mcle_run_mimo_flat(MCLE_MIMO_BLAST) for large arrays (csrc/pipeline_mimo_large.hip; nt = 1 is mimo.MRC): the
 * same link, draws (CHAN sample r nt + a = H[r][a], DATA symbol t nt + a, NOISE sample r n_symbols + t), counters, n_skipped and
 * 0xFFFFFFFF mark of a realization whose Gram matrix is not positive definite, so for shapes up to 4 x 4 the two entry points run
 * the same realizations; mcle_run_mimo_flat keeps its 4 x 4 envelope.  est = A x + G n runs on the matrix cores
 * (v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32); the filter is always built in f64.
 * Envelope: 1 <= nt <= 8, nt <= nr <= 16, n_symbols >= 1 with nr * n_symbols <= 2^31 - 1 (draw positions are 32-bit),
 * noise_var >= 0 and finite, mmse 0 (zero forcing) or 1 (set_noise_var(noise_var)), reserved 0, count <= 2^31 - 1, either
 * arithmetic, every demodulator of mcle_run_mimo_flat.  Anything else: MCLE_E_INVAL with a message, nothing touched.
 * Device memory: the context's scratch buffer holds the records of one launch slice, 512 bytes per K-step and realization in
 * complex128, 2 (ceil(nt / 4) + ceil(nr / 4)) K-steps (6 KiB at 8 x 16), half of that in complex64, at most 128 MiB in all.
 * mcle_ctx_last_kernel: "mimo_large_link f64|f32 <nr>x<nt> s<K-steps>". */
typedef struct mcle_mimo_large_cfg {
    int32_t nt, nr;
    int32_t n_symbols;                  /* NSymbs per transmit antenna */
    int32_t demod_method;
    int32_t mmse;                       /* 1 = set_noise_var(noise_var); 0 = zero forcing (the app) */
    int32_t reserved;                   /* 0 */
    double noise_var;
} mcle_mimo_large_cfg;
int mcle_run_mimo_large(mcle_ctx* ctx, int dtype, const mcle_mimo_large_cfg* cfg, uint64_t seed,
                        uint64_t first, uint64_t count, mcle_counters* d_counters,
                        uint32_t* d_sym_err, uint32_t* d_bit_err);

/* Fused frequency-selective MIMO-OFDM (round 5: one receive antenna per wavefront, csrc/mimo_tdl_wave.hpp; the workgroup-cooperative
 * kernel of rounds 1-4 behind MCLE_OPT_MIMO_TDL_KERNEL = 1 and for square geometries outside the wavefront kernel's envelope).
 * Returns MCLE_E_UNSUPPORTED (and touches nothing) when the Doppler phase across half an OFDM symbol is beyond the kernels'
 * polynomial tap model, or for a rectangular geometry outside the envelope named at mcle_mimo_ofdm_tdl_cfg: run the staged operators
 * then.  Device memory: the context's scratch buffer grows to hold the fading records of one launch slice -- 2.5 KiB per
 * realization and symbol in complex64 at five taps of 4 x 4, 7.5 KiB in complex128, at most 4 GiB (+ 25 %) per slice
 * (mcle_run_ofdm_tdl: at most 2 GiB) -- and is kept until the context is destroyed.
 * complex64 (this function and mcle_run_ofdm_tdl): while the largest Doppler phase of the run, Fd x (Ts + dt x samples of all symbols),
 * stays below a quarter turn the rays' Doppler frequencies are evaluated in float (v_cos_f32: < 4e-7 turns of phase, below the float
 * phasor's own rounding); beyond that in double as in complex128.  The threshold counts every symbol of the run, so complex64 counts
 * of the first symbols can change with n_ofdm_sym across it (within the complex64 tolerance of the oracle on both sides).
 * Fd must be >= 0 here (MCLE_E_INVAL otherwise; mcle_run_ofdm_tdl takes either sign). */
int mcle_run_mimo_ofdm_tdl(mcle_ctx* ctx, int dtype, const mcle_mimo_ofdm_tdl_cfg* cfg, uint64_t seed,
                           uint64_t first, uint64_t count, mcle_counters* d_counters,
                           uint32_t* d_sym_err, uint32_t* d_bit_err);

/* d_sum_capacity (may be NULL): per-realization sum_k log2(1 + SINR_k) of the chosen solution */
/* d_iterations (may be NULL): per-realization runned_iterations of an iterative solver.  Iterative solvers
 * draw their random initial precoders (randomizeF, iabase.py:538-540) from stream 3 of the realization.
 * 6 * n_symbols <= 2^31 - 1 (six receive antennas' noise rows; draw positions are 32-bit) and count <= 2^31 - 1 per call. */
int mcle_run_ia(mcle_ctx* ctx, int dtype, const mcle_ia_cfg* cfg, uint64_t seed, uint64_t first,
                uint64_t count, mcle_counters* d_counters, uint32_t* d_sym_err, uint32_t* d_bit_err,
                double* d_sum_capacity, uint32_t* d_iterations);

/* ---- a15: ClosedFormIASolver.solve (ia/algorithms.py:194-265) on injected channels, f64 only:
 *      d_bigH [batch][6][6] (MultiUserChannelMatrix.big_H, K = 3, 2x2) -> precoders d_F
 *      [batch][3][2] (full_F, P = 1), receive filters d_U [batch][3][2] (full_W_H), per-user SINR
 *      d_sinr [batch][3] and sum capacity d_capacity [batch] (both may be NULL).
 *      d_skipped [batch] (may be NULL; both entry points): 1 iff the realization has no solution to report -- one of the four
 *      inverted cross channels (H31, H12, H23, H32) is singular relative to its entries (|det| <= 1e-140 |H|_F^2; an
 *      iterative solver: a matrix it inverts on the way), the alignment is infeasible for a user (|W_k^H H_kk F_k| <=
 *      2^-33 |W_k| |H_kk|_F |F_k|: the wanted signal lies in the interference subspace, e.g. with every block diagonal), or
 *      an output is not finite.  The other outputs of such a realization are unspecified (they may be NaN); the fused
 *      pipelines count it in n_skipped.  Every other realization has finite outputs with U_k H_kk F_k = 1.
 *      A 2x2 eigenproblem with a repeated eigenvalue (a multiple of the identity to 2^-44: E with every cross channel equal,
 *      H_kk^H H_kk of a unitary direct channel under MCLE_IA_INIT_SVD, two orthogonal interferers of equal norm) HAS an
 *      answer: the canonical basis, e1 for the first (smaller) and e2 for the second (larger) eigenvalue, as LAPACK returns;
 *      MCLE_IA_INIT_SVD then starts from e1, the first right singular vector, as the reference does.  mcle_ia_closed_form
 *      and the iterative solvers return that answer.  The fused pipelines' closed-form solve (mcle_run_ia and
 *      mcle_run_ia_quantized with MCLE_IA_CLOSED_FORM) keeps its inlined body and FLAGS a realization whose E is a multiple
 *      of the identity, or whose chosen candidate is infeasible beside a feasible one, instead of answering it.
 *      Ties: the closed form keeps the first candidate unless the second one's capacity is strictly larger.  Where the two
 *      capacities agree to rounding -- real channels whose E has a complex-conjugate eigenvalue pair: the candidates are
 *      conjugates of one another -- the capacity is that of both and F, U are those of either one; which, rounding decides,
 *      here as in the reference.  Conditioning: the results are held to 16 x max(the f64 reference's own error, the
 *      measured sensitivity of the answer x 2^-52) (DESIGN.md "IA 2x2 envelope").  In mcle_ia_closed_form an
 *      ill-conditioned H31 (|det| < 2^-12 |H31|_F^2) does not enter: H31 F0 is then taken as H32 N F0 / lambda, F0 being an
 *      eigenvector of H31^-1 H32 N.  The other three inverted cross channels (H12, H23, H32), and H31 in the fused
 *      pipelines, enter with their condition number (about cond x 2^-52); nothing is flagged for conditioning short of
 *      the singularity above.
 *      Scale: H -> c H with noise_var -> c^2 noise_var is the same problem.  The closed form holds it while |H|^4 is
 *      representable (tested at c = 2^-250 ... 2^250); the iterative solvers form fourth powers of the entries and hold it
 *      while |H|^8 is (tested at 2^-100 ... 2^100; at 2^+-250 they flag every realization).
 *      An empty batch needs no arrays. ------------------------------------------------------------ */
int mcle_ia_closed_form(mcle_ctx* ctx, const void* d_bigH, double noise_var, void* d_F, void* d_U,
                        double* d_sinr, double* d_capacity, uint32_t* d_skipped, size_t batch);
/* Iterative solvers (solver = MCLE_IA_ALT_MIN / MIN_LEAKAGE / MAX_SINR / MMSE) from injected initial precoders
 * d_F_init [batch][3][2] (unit norm): the starting precoders for MCLE_IA_INIT_GIVEN ('fix' / a captured
 * 'random' start), the alternating-minimisation solver's start for MCLE_IA_INIT_ALT_MIN, ignored for
 * MCLE_IA_INIT_CLOSED_FORM.  IterativeIASolverBaseClass.solve (algorithms.py:802-883).  d_iterations [batch]
 * (may be NULL) = runned_iterations.
 * Reproducibility against the reference (complex128): the device eigen-solver is a cyclic Jacobi sweep, the reference's is
 * LAPACK (numpy.linalg.eig / eigh); both are backward stable, so precoders, filters and SINRs agree to <= 1e-9 relative
 * where the iteration is well conditioned, and the decisions of a link built on them are then identical.  Where the
 * iteration ends badly conditioned -- a stream in outage, an eighth or more of a realization's symbols wrong -- the
 * rounding-level difference is amplified over the iterations and decisions at near-ties may differ: bound asserted by
 * tests/test_gpu_fuzz.py on such realizations: |symbol errors - reference's| <= max(2, 2 %), |bit errors| <= max(8, 4 %);
 * every other realization is exact.  The closed-form solver (mcle_ia_closed_form) iterates nothing and has no such
 * amplification; its own caveats are the tie rule and the conditioning rule above (tests/test_gpu_ia3_envelope.py). */
int mcle_ia_iterative(mcle_ctx* ctx, int solver, int initialize_with, const void* d_bigH,
                      const void* d_F_init, double noise_var, int max_iterations, double relative_factor,
                      void* d_F, void* d_U, double* d_sinr, double* d_capacity, uint32_t* d_iterations,
                      uint32_t* d_skipped, size_t batch);

/* ---- block diagonalisation with external interference (comm/blockdiagonalization.py:666-1469): WhiteningBD
 *      (:722-836: whiten every user's rows with the interference-plus-noise covariance, block-diagonalise, receive
 *      filter = pinv(newH) x whitening filter) and EnhancedBD (:839-1469: BD directions, then per user a stream
 *      reduction onto the directions least hit by the external interference; number of streams fixed ('naive',
 *      'fixed') or chosen per user by a metric).  The channel is MultiUserChannelMatrixExtInt.big_H
 *      (channels/multiuser.py:2011-2520): d_bigH [batch][K r][K r + n_ext], the last n_ext columns being the
 *      interferers' antennas; covariance = pe H_ext H_ext^H + noise_var I (:2469-2520).
 *      Outputs, zero padded: d_Ms [batch][K][K r][r] (user k's precoder MsPk, K r x Ns), d_W [batch][K][r][r]
 *      (receive filter, Ns x r), d_ns [batch][K]; d_cand_sinr [batch][K][r][r] (metric 4 only: row ns-1 = the
 *      post-filter SINRs with ns streams, EnhancedBD._calc_linear_SINRs :1101-1138, for caller-side metrics such
 *      as 'effective_throughput').  Singular-vector phases are ours (see mcle_block_diagonalize).
 *      d_skipped [batch] (may be NULL) is 1 iff the channel of the K users is numerically singular, or -- WhiteningBD
 *      only -- some Re_k is: an eigenvalue of Re_k <= 2^-42 of its largest (mcle_blast_filter's tolerance; relative, so
 *      big_H times a power of two flags the same items; a rank-deficient pe H_ext H_ext^H at noise_var = 0 comes out
 *      of the Jacobi sweep at about 1e-17 of the largest, not at 0).  The outputs of a flagged item mean nothing.
 *      Receive filters: W_k = pinv(H_k Ms_k) (None; times the whitening filter for WhiteningBD) goes through the
 *      Jacobi pseudo-inverse and loses ONE power of cond(H_k Ms_k), as numpy.linalg.pinv does; W_k H_k Ms_k = I to
 *      eps ||W_k|| ||H_k|| ||Ms_k||.
 *      Repeated eigenvalues of Re_k (decided here, not in the reference):
 *      - pe = 0 or n_ext = 0: Re_k = noise_var I, V = I, and the cut V[:, :ns] keeps the FIRST ns block-diagonalising
 *        directions (those with the smallest singular values of H_k Ms_k): 'fixed' and the per-user rule then return
 *        bit for bit what 'naive' returns for ns < r.
 *      - rank(H_ext,k) < r - ns: the cut lies inside the noise eigenspace, in the basis the Jacobi sweep leaves; any
 *        basis is a valid answer, and every one has W_k H_ext,k = 0, W_k H_k MsPk = I, ||MsPk||_F^2 = iPu.
 *      - the whitening filter is V diag(L^-1/2) with ORTHONORMAL V in every case, so the whitened equivalent channels
 *        are orthogonal; the reference's numpy.linalg.eig returns a non-orthogonal basis of a repeated eigenvalue's
 *        space, for which its filter does not whiten (Ms Ms^H, W^H W and |W H_k Ms| are the same either way).
 *      - noise_var = pe = 0 (EnhancedBD only; WhiteningBD is refused or flagged): Re_k = 0, the one-stream candidate
 *        has an infinite SINR (d_cand_sinr holds +inf) and, the first maximum deciding, 'capacity' returns Ns = 1.
 *        With noise_var = 0 and pe > 0 a candidate whose cut lies in the null space of Re_k has an infinite exact SINR
 *        and a computed one that is a rounding residue: the selection among such candidates is the
 *        first maximum of those residues.
 *      Held to a 50-digit oracle over every geometry with K r <= 8 by tests/test_gpu_bd_extint_envelope.py. */
typedef struct mcle_bd_extint_cfg {
    int32_t num_users, n_ant_per_user, n_ext;
    int32_t method;             /* 0: WhiteningBD, 1: EnhancedBD */
    int32_t metric;             /* EnhancedBD: 0 None, 1 'naive', 2 'fixed', 3 'capacity', 4 report candidate SINRs,
                                   5 stream counts given per user (ns_user) */
    int32_t num_streams;        /* 'naive' / 'fixed' */
    int32_t ns_user[4];
    double iPu, noise_var, pe;
} mcle_bd_extint_cfg;
int mcle_bd_extint(mcle_ctx* ctx, const mcle_bd_extint_cfg* cfg, const void* d_bigH, void* d_Ms, void* d_W,
                   int32_t* d_ns, double* d_cand_sinr, uint32_t* d_skipped, size_t batch);

/* ---- iterative interference alignment for general geometries (SURVEY 8(f).3 tail): 2 <= K <= 4 users with
 *      Nr x Nt <= 6 x 6 antennas each (the reference's own application runs K = 3, Nr = 5, Nt = 3, Ns = 2,
 *      apps/ia/IA_Results_NrxNt(Ns).py:130-133) and per-user stream counts; AlternatingMinIASolver / MinLeakageIASolver /
 *      MaxSinrIASolver .solve (ia/algorithms.py:802-883, 885-1507) from injected precoders ('fix') or the 'svd'
 *      start (:503-547, Nr == Nt), optionally inside GreedStreamIASolver.solve (:1905-2010: drop the worst stream
 *      while the sum capacity grows) or BruteForceStreamIASolver.solve (:2147-2260: every stream combination up to
 *      ns[], 'svd' start, best sum capacity).  One lane per channel realization, f64.
 *      Padded arrays are D x D with D = 4 when max(Nr, Nt) <= 4 and D = 6 otherwise (two instantiations of the solver).
 *      d_bigH [batch][K nr][K nt]; d_F_init [batch][4][D][D] = user k's nt x ns[k] start in the top-left corner
 *      (ignored for 'svd' and for brute force).  Outputs, same padded layout: d_F (nt x ns, unit Frobenius norm =
 *      full_F for P = 1), d_U (full_W_H, ns x nr), d_sinr [batch][4][D] (linear, per stream), d_capacity [batch],
 *      d_iterations [batch] (all runs of a selection wrapper added up), d_ns [batch][4] (streams kept per user),
 *      d_skipped [batch] (a singular system met on the way), d_every_capacity [batch][256] (brute force only: the sum
 *      capacity of every stream combination in itertools.product order, last user fastest --
 *      BruteForceStreamIASolver.every_sum_capacity :2135-2145); every output but d_F / d_U may be NULL.
 *      Eigenvector phases are ours, not LAPACK's: SINRs, capacity and decisions do not depend on them.
 *      The envelope, refused with MCLE_E_INVAL before anything is launched: K in [2, 4]; Nr, Nt in [1, 6]; ns[k] in
 *      [1, min(Nr, Nt)]; max_iterations >= 1; noise_var >= 0 (0 is allowed: a max-SINR matrix that loses its rank without
 *      the noise term is solved as it is, and a realization whose result is not finite is flagged in d_skipped);
 *      relative_factor >= 0; the 'svd' start and brute force (which starts from it) need Nr == Nt; brute force takes at
 *      most 256 stream combinations (prod ns[k]).  min-leakage with more than one stream -- beyond the reference, whose
 *      calc_Q_rev asserts -- scales its precoder (ns orthonormal eigenvectors) to unit Frobenius norm like the other two.
 *      alt-min and min-leakage read each precoder from the right singular vectors of the stacked factor [X_k^H H_kl]_k
 *      (one-sided Jacobi), not from the eigenvectors of the formed matrix: a leakage below eps |A|^2 keeps its digits.
 *      d_skipped is set by a singular system in an update (max-SINR's B, alt-min's [H F, C]), in full_W_H, and by a sum
 *      capacity that is not finite.  Sets mcle_ctx_last_kernel to "ia_general<D> K=.. NrxNt" (D = 4 or 6). */
typedef struct mcle_ia_general_cfg {
    int32_t K, nr, nt;
    int32_t ns[4];
    int32_t solver;             /* MCLE_IA_ALT_MIN / MCLE_IA_MIN_LEAKAGE / MCLE_IA_MAX_SINR */
    int32_t initialize_with;    /* MCLE_IA_INIT_GIVEN or MCLE_IA_INIT_SVD */
    int32_t max_iterations;
    int32_t stream_selection;   /* 0: none, 1: greedy, 2: brute force */
    int32_t reserved;
    double noise_var, relative_factor;
} mcle_ia_general_cfg;
int mcle_ia_solve_general(mcle_ctx* ctx, const mcle_ia_general_cfg* cfg, const void* d_bigH, const void* d_F_init,
                          void* d_F, void* d_U, double* d_sinr, double* d_capacity, uint32_t* d_iterations,
                          int32_t* d_ns, uint32_t* d_skipped, double* d_every_capacity, size_t batch);

/* ---- the IA link on general geometries, fused (apps/ia/simulate_ia.py:94-245 with Nr, Nt, Ns as parameters;
 *      apps/ia/IA_Results_NrxNt(Ns).py: K = 3, 5 x 3, Ns = 2; apps/ia/simulate_greedy_ia.py: 3 x 3, Ns = 3 under the greedy
 *      wrapper, its 'NoPathLoss' scenario = this link with P = 1, noise_var = 1 / SNR).  Per realization: draw big_H and -- for
 *      MCLE_IA_INIT_GIVEN, which here means "drawn on chip" as in mcle_run_ia -- the random start (randomizeF, iabase.py:538-540);
 *      solve with the kernel of mcle_ia_solve_general (stream_selection 0 / 1 / 2 included: the solution is bit-identical to
 *      the operator's on the same inputs); send n_symbols per KEPT stream at unit power per user; add noise of variance
 *      cfg->noise_var; apply full_W_H; demodulate; count.
 * cfg: the envelope and the refusals of mcle_ia_solve_general, word for word; additionally n_symbols >= 1, a constellation of
 *      M <= 256 and a known demod_method.  count = 0 returns MCLE_OK and launches nothing; nothing is written on a refusal.
 * Draws (mcle-philox-v1, realization index = subsequence):
 *   stream 2 (channel)  big_H[i][c], row-major over [K nr][K nt]: CN sample i K nt + c
 *   stream 3 (start)    F_k[i][j] (nt x ns[k], the CONFIGURED ns): CN sample nt sum_{k' < k} ns[k'] + i ns[k] + j, then the
 *                       matrix is divided by its Frobenius norm
 *   stream 0 (data)     kept streams numbered q = 0, 1, .. in user order, in the order the solver leaves them; symbol j of
 *                       stream q: byte q n_symbols + j
 *   stream 1 (noise)    receive antenna a = k nr + i, symbol j: CN sample a n_symbols + j, scaled by sqrt(noise_var)
 *   At K = 3, Nr = Nt = 2, Ns = 1 these are exactly the positions of mcle_run_ia.  Channel and start are drawn in f64 for
 *   either dtype (the solver is f64 only); the walk draws in the call's dtype.
 * Outputs, each NULL or: d_sym_err / d_bit_err [count] (0xFFFFFFFF: flagged by the solver -- mcle_ia_solve_general's d_skipped
 *   -- counted in n_skipped and nowhere else, its stream slots 0); d_stream_sym_err / d_stream_bit_err [count][4][6] by slot
 *   (user, kept stream), 0 on an inactive slot; d_ns [count][4] streams kept per user; d_sinr [count][4][6] linear, 0 on an
 *   inactive slot; d_capacity, d_iterations [count]; d_bigH [count][K nr][K nt] and d_F_init / d_F / d_U [count][4][D][D]
 *   complex128 in the solver's padded layout (d_F_init all zero when no start is drawn).
 *   d_counters: n_symbols / n_bits are the figures with every CONFIGURED stream active (n_symbols sum_k ns[k] per realization,
 *   the mcle_run_comp convention); a realization sent n_symbols sum_k d_ns[.][k].
 * The per-realization arrays do not depend on the slice, the grid or how [first, first + count) is split.  Scratch for the
 * channels, starts, solutions and link records of one slice stays <= 1 GiB.
 * mcle_ctx_last_kernel: "ia_general_link f64|f32 D<4|6> pairs|single" (pairs: n_symbols even, two columns per lane). */
int mcle_run_ia_general(mcle_ctx* ctx, int dtype, const mcle_ia_general_cfg* cfg, int n_symbols, int demod_method,
                        uint64_t seed, uint64_t first, uint64_t count, mcle_counters* d_counters, uint32_t* d_sym_err,
                        uint32_t* d_bit_err, uint32_t* d_stream_sym_err, uint32_t* d_stream_bit_err, int32_t* d_ns,
                        double* d_sinr, double* d_capacity, uint32_t* d_iterations, void* d_bigH, void* d_F_init, void* d_F,
                        void* d_U);

/* ---- block diagonalisation of a multi-user downlink (SURVEY 8(f).3 tail) --------------------
 * comm/waterfilling.py:15-92 doWF: d_gains [batch][n] channel POWER gains -> optimum powers
 * d_powers [batch][n] (same order) and the water level d_mu [batch] (may be NULL); n <= 64. */
int mcle_waterfilling(mcle_ctx* ctx, const double* d_gains, int n, double total_power, double noise_var,
                      double* d_powers, double* d_mu, size_t batch);
/* comm/blockdiagonalization.py:466-508 BlockDiagonalizer.block_diagonalize (waterfilling = 1: water-filling
 * over all streams normalised to the strongest user block, :403-464) or :510-566
 * block_diagonalize_no_waterfilling (waterfilling = 0), plus :568-585 calc_receive_filter, f64 only, on
 * injected channels d_H [batch][n][n] (row-major, n = num_users * n_rx_per_user <= 8, square: as many
 * transmit as receive antennas).  Outputs (each may be NULL): precoder d_Ms [batch][n][n], d_newH = H Ms
 * [batch][n][n], zero-forcing filter d_W = pinv(newH) [batch][n][n], singular values of the users'
 * equivalent channels d_sigma [batch][n] (ascending per user, the reference's Sigma), d_skipped [batch] =
 * 1 for a numerically singular channel.  Singular vectors are unique up to one phase per stream; this
 * entry point returns the representative whose largest entry per Ms column is real positive. */
int mcle_block_diagonalize(mcle_ctx* ctx, const void* d_H, int num_users, int n_rx_per_user, double iPu,
                           double noise_var, int waterfilling, void* d_Ms, void* d_newH, void* d_W,
                           double* d_sigma, uint32_t* d_skipped, size_t batch);

/* np.linalg.pinv (the receive filter of blockdiagonalization.py:568-585 for any newH): d_A [batch][m][n] ->
 * d_out [batch][n][m], f64, m, n <= 8; singular values <= rcond * max are dropped (numpy's default 1e-15). */
int mcle_pinv(mcle_ctx* ctx, const void* d_A, int m, int n, double rcond, void* d_out, size_t batch);

typedef struct mcle_bd_cfg {            /* apps/comp_BD/simulate_comp_simple.py:95-140 (no external interference) */
    int32_t K, nr;                      /* K cells/users of nr x nr antennas: channel (K nr) x (K nr), K nr <= 8 */
    int32_t n_symbols;                  /* NSymbs per stream (K nr streams) */
    int32_t demod_method;
    int32_t waterfilling;               /* 1: block_diagonalize, 0: block_diagonalize_no_waterfilling */
    int32_t has_pathloss;               /* 1: block (rx k, tx l) scaled by sqrt(pathloss[k*K + l]) (multiuser.py:256-292) */
    double iPu;                         /* power per user */
    double noise_var;                   /* channel noise variance */
    double bd_noise_var;                /* noise variance handed to the water-filling (the app passes 1e-50) */
    double pathloss[16];
} mcle_bd_cfg;
/* Fused: channel draw, block diagonalisation, precoding, channel + noise, zero forcing, demodulation, counts.
 * K * nr * n_symbols <= 2^31 - 1 (draw positions are 32-bit) and count <= 2^31 - 1 per call. */
int mcle_run_bd(mcle_ctx* ctx, int dtype, const mcle_bd_cfg* cfg, uint64_t seed, uint64_t first,
                uint64_t count, mcle_counters* d_counters, uint32_t* d_sym_err, uint32_t* d_bit_err);

/* ---- CoMP with an external interferer and per-realization stream reduction, fused (apps/comp_BD/simulate_comp.py:311-621,
 *      simulate_comp_with_ext_int_simple.py): per realization draw big_H [K r][K r + n_ext], apply the path loss (block
 *      (rx k, tx l) times sqrt(pathloss[k*K + l]), interferer column e of user k times sqrt(pathloss_ext[k*n_ext + e])),
 *      solve WhiteningBD or EnhancedBD (the arithmetic of mcle_bd_extint, f64 for either dtype), for 'capacity' /
 *      'effective_throughput' choose every user's stream count on the device (first maximum, as np.argmax), send n_symbols
 *      per kept stream, add the interferers' data (power pe) and noise, filter, demodulate, count.
 *      'effective_throughput' value of a candidate with post-filter SINRs s_i: sum_i Kb (1 - PER_i), PER = 1 - (1 - BER)^
 *      packet_length, BER the closed form of the context's constellation (MCLE_CONST_BPSK, MCLE_CONST_QAM; any other kind is
 *      taken as M-PSK), Q(x) = erfc(x / sqrt 2) / 2.
 *      The app's six variants: None / 'naive' / 'fixed' / 'capacity' / 'effec_throughput' = method 1 with metric 0..4,
 *      'Whitening' = method 0 (metric ignored).
 * Draws (mcle-philox-v1, realization index = subsequence; n = K r):
 *   stream 2 (channel)     user block entry (i, c) at i n + c -- the positions of mcle_run_bd; interferer entry (i, e) at
 *                          n^2 + i n_ext + e
 *   stream 0 (data)        active streams numbered q = 0, 1, .. in user order; symbol j of stream q at q n_symbols + j -- every
 *                          variant sends the same data on its first streams (the app re-seeds its data generator per metric)
 *   stream 1 (noise)       receive antenna i, symbol j at i n_symbols + j -- as mcle_run_bd
 *   stream 3 (interferer)  CN(0, 1) sample e n_symbols + j, scaled by sqrt(pe)
 *   Hence n_ext = 0 (or pe = 0), method 1, metric 0 gives the per-realization counts of mcle_run_bd(waterfilling = 0), and one
 *   seed gives all variants common random numbers (the app draws fresh noise per metric; the statistics are the same).
 * d_pathloss: NULL (the config's static set, has_pathloss = 0: all ones) or [count][K][K + n_ext], one set per realization
 *   (rx user; tx users, then interferer antennas).
 * Outputs, each NULL or: d_sym_err / d_bit_err [count] (0xFFFFFFFF: numerically singular channel, not counted);
 *   d_stream_sym_err / d_stream_bit_err [count][K r] by stream slot k r + j (0 on an inactive stream); d_ns [count][K];
 *   d_sinr [count][K r], linear, 0 on an inactive stream: MultiUserChannelMatrixExtInt.calc_JP_SINR with interferer power
 *   sinr_pe -- the app calls it WITHOUT pe, so its sinr_* results use 1.0 (simulate_comp.py:592); pass sinr_pe = 1 to
 *   reproduce that.  d_counters: n_symbols / n_bits are the figures with every stream active (K r n_symbols per realization);
 *   a realization sent n_symbols * sum_k d_ns[.][k].
 * Envelope: 1 <= K <= 4, 1 <= r <= 4, K r <= 8, 0 <= n_ext <= 8, n_symbols >= 1, M <= 256.  count = 0 returns MCLE_OK and
 * launches nothing.  The per-realization arrays do not depend on the grid or on how [first, first + count) is split.
 * mcle_ctx_last_kernel: "comp_link f64|f32 r<r> pairs|single" (pairs: n_symbols even, two columns per lane). */
typedef struct mcle_comp_cfg {
    int32_t K, r, n_ext, n_symbols, demod_method;
    int32_t method;          /* 0 WhiteningBD, 1 EnhancedBD */
    int32_t metric;          /* 0 None, 1 naive, 2 fixed, 3 capacity, 4 effective_throughput */
    int32_t num_streams;     /* naive / fixed */
    int32_t packet_length;   /* effective_throughput */
    int32_t has_pathloss;
    double iPu, noise_var, pe, sinr_pe;
    double pathloss[16], pathloss_ext[32];
} mcle_comp_cfg;
int mcle_run_comp(mcle_ctx* ctx, int dtype, const mcle_comp_cfg* cfg, uint64_t seed, uint64_t first, uint64_t count,
                  const double* d_pathloss /* NULL or [count][K][K + n_ext], one set per realization */,
                  mcle_counters* d_counters, uint32_t* d_sym_err, uint32_t* d_bit_err,
                  uint32_t* d_stream_sym_err, uint32_t* d_stream_bit_err, int32_t* d_ns, double* d_sinr);

/* ---- pilot-based channel estimation from CAZAC reference signals (reference_signals/channel_estimation.py:73-131
 *      CazacBasedChannelEstimator, :135-251 CazacBasedWithOCCChannelEstimator) ----------------------------------
 * out = FFT_{m ne}( IFFT_{ne}(conj(ref) * y)[0 : num_taps_to_keep + 1] ), times ne when `normalized` (a sequence of unit
 * norm), m = size_multiplier; note the reference keeps num_taps_to_keep + 1 taps.  y = mean_c(cover[c] * rx[c]) over the
 * cover-code axis (n_cover = 1 and cover = NULL: no cover code).  d_ref_seq [ne], d_rx [rows][n_cover][ne], d_out
 * [rows][m ne], complex of `dtype`; cover: HOST pointer, n_cover reals.  A row is one (realization, receive antenna).
 * Both transforms run as pruned direct DFTs (ne (K + 1)(1 + m) complex FMAs per row), so ne is any size >= 2 with
 * m ne <= 4096; 0 <= num_taps_to_keep < ne; 1 <= n_cover <= 8.  rows = 0 returns MCLE_OK and launches nothing.
 * mcle_ctx_last_kernel: "cazac_estimate f64|f32 w<wavefronts per workgroup>" (+ " gtw": table read from global memory). */
int mcle_cazac_estimate(mcle_ctx* ctx, int dtype, const void* d_ref_seq, int ne, const void* d_rx, size_t rows, int n_cover,
                        const double* cover, int num_taps_to_keep, int size_multiplier, int normalized, void* d_out);

/* Fused estimation-error Monte Carlo (the experiment of apps/simple_precoded_srs.py without interference cancellation).  One
 * realization: n_users users send their reference sequences on the same comb; each (user, receive antenna) link is a
 * block-static tapped delay line h_i = sqrt(p_i) randn_c at integer delays d_i of the m ne-point grid (tap powers
 * normalised to sum 1), H[k] = sum_i h_i exp(-2 pi j k d_i / (m ne)); received Y[a][n] = sum_u H_u[a][m n] r_u[n] +
 * sqrt(noise_var) randn_c; every user is estimated as mcle_cazac_estimate does, on chip.  Outputs per realization and
 * user: d_err [count][n_users] = sum_{a,k} |H^ - H|^2, d_pow [count][n_users] = sum_{a,k} |H|^2 (every entry written; the
 * caller sums them in index order, so results do not depend on the grid or on how [first, first + count) is split).
 * Draws: DESIGN section 4 (taps: stream 2, noise: stream 1).  mcle_ctx_last_kernel: "chanest f64|f32 w<n>" (+ " gtw"). */
typedef struct mcle_chanest_cfg {
    int32_t ne;                         /* reference sequence length (comb positions), >= 2 */
    int32_t size_multiplier;            /* m: the channel has m ne subcarriers, m ne <= 4096 */
    int32_t num_taps_to_keep;           /* K: K + 1 taps are kept, 0 <= K < ne */
    int32_t n_users, n_rx;              /* <= 8, <= 4 */
    int32_t n_taps;                     /* <= MCLE_MAX_TAPS */
    int32_t normalized;                 /* 1: the sequences have unit norm (estimates are multiplied by ne) */
    int32_t reserved;
    double noise_var;
    double tap_power[MCLE_MAX_TAPS];    /* linear, any positive sum (normalised by the library) */
    int32_t tap_delay[MCLE_MAX_TAPS];   /* 0 <= d < ne */
    const void* d_ref_seq;              /* DEVICE pointer: the users' sequences [n_users][ne], complex of the call's dtype */
} mcle_chanest_cfg;
int mcle_run_chanest(mcle_ctx* ctx, int dtype, const mcle_chanest_cfg* cfg, uint64_t seed, uint64_t first, uint64_t count,
                     double* d_err, double* d_pow);

/* The staged cancellation operator: out[row][n] = rx[row][n] - est[row][m n] * ref[n], m = size_multiplier -- the contribution
 * of an estimated user taken out of the comb it was estimated from.  d_ref_seq [ne], d_rx and d_out [rows][ne], d_est
 * [rows][m ne] as mcle_cazac_estimate writes it, complex of `dtype`; d_out may be d_rx (in place).  ne >= 2, m >= 1,
 * m ne <= 4096.  rows = 0 returns MCLE_OK and launches nothing.  mcle_ctx_last_kernel: "cazac_cancel f64|f32". */
int mcle_cazac_cancel(mcle_ctx* ctx, int dtype, const void* d_ref_seq, int ne, const void* d_rx, const void* d_est, size_t rows,
                      int size_multiplier, void* d_out);

/* mcle_run_chanest with a path loss per user and interference cancellation at the one receiver (the experiment of
 * apps/simple_precoded_srs.py:127-345).  Same draws; the taps of every link of user u are multiplied by sqrt(link_gain[u]),
 * and the true response H_u (hence d_pow) includes the gain.  With k = m n the comb bins:
 *   mode 0: every user is estimated from the received comb Y, as mcle_run_chanest does.
 *   mode 1: the direct user d is estimated from Y; R0[a][n] = Y[a][n] - H^_d[a][m n] r_d[n]; every other user from R0.
 *   mode 2: mode 1, then an ordered successive cancellation over the others: they are ordered by the Frobenius norm of
 *           their first estimates over all antennas and all m ne bins, descending (an exact tie: the higher user index
 *           counts as stronger); the strongest keeps its first estimate, and for s = 2, 3, ... the s-th strongest is
 *           estimated again from R_{s-1} = R_{s-2} - H^_o[m n] r_o[n], o the (s-1)-th strongest with its final estimate.
 * d_err, d_pow [count][n_users] as mcle_run_chanest; d_order (int32 [count][n_users], may be NULL): the order in which the
 * users received their final estimates, the direct user first, then the others by descending norm (mode 2) or ascending
 * index (mode 1); in mode 0 the row is 0, 1, 2, ... .  Every rule of mcle_run_chanest applies to `base`; mode in {0, 1, 2},
 * 0 <= direct_user < n_users, link_gain[u] > 0 and finite for u < n_users.  count = 0 returns MCLE_OK and launches
 * nothing.  The output arrays do not depend on the grid, on MCLE_OPT_GRID_OVERSUB or on how [first, first + count) is split.
 * A shape whose one realization does not fit the 160 KiB of LDS is refused ("does not fit").
 * mcle_ctx_last_kernel: "chanest_ic f64|f32 w<n>" (+ " gtw"). */
typedef struct mcle_chanest_ic_cfg {
    mcle_chanest_cfg base;
    int32_t mode;                       /* 0: none, 1: direct link removed, 2: direct link removed + ordered SIC */
    int32_t direct_user;                /* the receiver's own user */
    double link_gain[8];                /* linear power gain per user, > 0 */
} mcle_chanest_ic_cfg;
int mcle_run_chanest_ic(mcle_ctx* ctx, int dtype, const mcle_chanest_ic_cfg* cfg, uint64_t seed, uint64_t first,
                        uint64_t count, double* d_err, double* d_pow, int32_t* d_order);

/* ---- LS and MMSE block-pilot channel estimators (channel_estimation/estimators.py:12-61 compute_ls_estimation, :100-174
 *      compute_mmse_estimation; Fodor et al. 2014) ---------------------------------------------------------------
 * Model Y = h s + N: d_Y [batch][nr][n_pilots] row-major, d_out [batch][nr][nt], both complex of `dtype`; d_s [nt][n_pilots]
 * when the pilots are shared (s_per_realization = 0, the reference's 2-D s), [batch][nt][n_pilots] when every realization
 * has its own (s_per_realization = 1, the 3-D s).  The matched filter z = Y s^H is formed on chip, per realization.
 * 1 <= nr <= 128, 1 <= n_pilots <= 1024.  batch = 0 returns MCLE_OK and launches nothing.  Outputs are bit-identical for
 * any split of the batch.
 *
 * mcle_ls_estimate: out[b] = Y[b] s^H (s s^H)^-1; 1 <= nt <= 8, nt <= n_pilots.  The nt x nt Gram matrix is accumulated and
 * inverted in f64 on chip, per realization, or once per workgroup when the pilots are shared.  A SINGULAR Gram matrix gives
 * unspecified values (inf / nan), never a fault; the reference raises LinAlgError there.
 * mcle_ctx_last_kernel: "ls_estimate f64|f32 nt<nt rounded up to a power of two>".
 *
 * mcle_mmse_estimate: nt = 1 (the reference asserts it; d_s is [n_pilots] or [batch][n_pilots]);
 * out[b] = A (Y[b] s^H) n_pilots / |s|^2 with A = (noise_power I + n_pilots C)^-1 C, the reference's literal expression.
 * cov: HOST pointer to C, [nr][nr] complex128 (interleaved re, im); null, noise_power < 0 or a value that is not finite is
 * refused, and so is a singular noise_power I + n_pilots C.  A is computed at most once per call on the host in f64 (the
 * last result is kept and reused while cov, n_pilots and noise_power stay the same) and applied on
 * the matrix cores (v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32) over tiles of 16 realizations per wavefront; it is read
 * from global memory (L2) by every workgroup.  mcle_ctx_last_kernel: "mmse_estimate f64|f32 ga" (ga: A read from global
 * memory, the only form).  Both functions return -1 for a violated rule, with a message that names the argument. */
int mcle_ls_estimate(mcle_ctx* ctx, int dtype, const void* d_Y, const void* d_s, int nr, int nt, int n_pilots,
                     int s_per_realization, size_t batch, void* d_out);
int mcle_mmse_estimate(mcle_ctx* ctx, int dtype, const void* d_Y, const void* d_s, int nr, int n_pilots, int s_per_realization,
                       size_t batch, double noise_power, const double* cov, void* d_out);

/* Fused estimation-error Monte Carlo of the two estimators (the loop of the reference's
 * tests/channel_estimation_package_test.py:246-325).  One realization: pilots s [nt][n_pilots] (drawn, or d_pilots);
 * w [nr][nt] of CN(0, 1) and h = alpha L w; Y = h s + sqrt(noise_power) N with all nr n_pilots noise samples drawn; h^_LS as
 * mcle_ls_estimate; with `cov` (needs nt = 1) h^_MMSE as mcle_mmse_estimate from the same Y.  Y is never stored.
 * d_err_ls, d_err_mmse, d_pow [count]: |h^_LS - h|_F^2, |h^_MMSE - h|_F^2, |h|_F^2 per realization, every entry written;
 * d_err_mmse may be NULL when cov is NULL.  They do not depend on the grid, on MCLE_OPT_GRID_OVERSUB or on how
 * [first, first + count) is split; the caller sums in index order.  count = 0 returns MCLE_OK and launches nothing.
 * Draws: DESIGN section 4 (pilot phases: stream 3, w: stream 2, noise: stream 1).  No shape inside the argument rules
 * exceeds the 160 KiB of LDS: the largest working set of a wavefront is 133 120 bytes (nr = 128, nt = 8, n_pilots = 256,
 * drawn pilots, MCLE_F64).  The launcher still checks the size ("does not fit"), but the argument rules make that refusal
 * unreachable; it is a guard for the day a rule is widened.
 * mcle_ctx_last_kernel: "pilot_mse f64|f32 b<realizations per wavefront> ls|ls+mmse" (+ " gl": L applied from global memory). */
typedef struct mcle_pilot_mse_cfg {
    int32_t nr, nt, n_pilots;           /* 1..128, 1..8, nt..256 */
    int32_t random_pilots;              /* 1: drawn per realization, s = sqrt(pilot_power) e^{2 pi j u}; 0: d_pilots */
    double pilot_power, noise_power, alpha;
    const void* d_pilots;               /* DEVICE [nt][n_pilots], complex of the call's dtype; used when random_pilots = 0 */
    const double* chan_factor;          /* HOST [nr][nr] complex128 L: h = alpha L w; NULL: L = I */
    const double* cov;                  /* HOST [nr][nr] complex128: the C handed to the MMSE estimator; NULL: LS only */
} mcle_pilot_mse_cfg;
int mcle_run_pilot_mse(mcle_ctx* ctx, int dtype, const mcle_pilot_mse_cfg* cfg, uint64_t seed, uint64_t first, uint64_t count,
                       double* d_err_ls, double* d_err_mmse, double* d_pow);

/* Flat MIMO (Blast) link with pilot-estimated channel state next to perfect channel state (csrc/pipeline_mimo_pilot.hip): what an
 * estimation error costs in symbol and bit errors.  One realization: H = alpha L W (W nr x nt of CN(0, 1); L = I when
 * d_chan_factor is NULL); a pilot block s [nt][n_pilots] of power pilot_power (drawn, s = sqrt(pilot_power) e^{2 pi j u}, or
 * d_pilots); Y_p = H s + sqrt(noise_var) N_p; the estimate
 *     LS:    H^ = Y_p s^H (s s^H)^-1
 *     MMSE:  h^ = B (Y_p s^H) n_pilots / |s|^2, nt = 1, B = (noise_var I + n_pilots C)^-1 C formed by the caller in f64;
 * then the data of mcle_run_mimo_flat(MCLE_MIMO_BLAST): X = reshape(sym, (nt, -1), 'F') / sqrt(nt), Y = H X + sqrt(noise_var) N,
 * est = G Y with G = sqrt(nt) solve(A^H A + nu I, A^H) (nu = noise_var if mmse_filter else 0; pinv(A) at nu = 0) for A = H^
 * (d_counters[0], estimated CSI) and for A = H (d_counters[1], perfect CSI).  Both filters see the same symbols and the same
 * noise samples: one walk over the data, one noise draw.  A realization whose pilot Gram matrix (a pivot at or below 1e-12 of
 * its trace) or either filter is numerically singular is skipped in BOTH blocks (n_skipped; 0xFFFFFFFF in the per-realization
 * arrays).
 * Envelope: 1 <= nt <= nr <= 4; nt <= n_pilots <= 256; n_symbols >= 1; noise_var >= 0; pilot_power > 0; alpha finite; the MMSE
 * estimator needs nt = 1 and d_mmse_matrix; fixed pilots (random_pilots = 0) need d_pilots; count <= 2^31-1.  Anything else
 * returns MCLE_E_INVAL with a message naming the rule; count = 0 returns MCLE_OK and launches nothing.
 * d_pilots [nt][n_pilots], d_chan_factor [nr][nr], d_mmse_matrix [nr][nr]: DEVICE, row-major complex128 (interleaved re, im)
 * whatever `dtype`: the channel, the pilot block, the estimate and both filters are formed in f64 per realization (the inverse
 * Gram matrix of a fixed pilot block once per call, on the host); `dtype` is the arithmetic of the walk over the data.
 * d_sym_err, d_bit_err: NULL or [2][count] (block 0 then block 1); d_err, d_pow: NULL or [count], |H^ - H|_F^2 and |H|_F^2 (f64;
 * unspecified for a skipped realization).  Nothing depends on the grid, on MCLE_OPT_GRID_OVERSUB or on how
 * [first, first + count) is split.
 * Draws (mcle-philox-v1), realization first + r of `seed`:
 *     W[r][a]             stream 2 (CHAN)    CN sample r nt + a                     as mcle_run_mimo_flat
 *     data symbol         stream 0 (DATA)    n = t nt + a                           as mcle_run_mimo_flat
 *     data noise (r, t)   stream 1 (NOISE)   CN sample r n_symbols + t              as mcle_run_mimo_flat
 *     pilot phase (a, p)  stream 3 (PHASE)   uniform a n_pilots + p                 random pilots only
 *     pilot noise (r, p)  stream 4 (PILOT)   CN sample 2 ceil(n_pilots / 2) r + p
 * so with L = I and alpha = 1 block 1 is mcle_run_mimo_flat(MCLE_MIMO_BLAST) on the same (seed, realization).
 * mcle_ctx_last_kernel: "mimo_pilot_link f64|f32 ls|mmse". */
typedef struct mcle_mimo_pilot_cfg {
    int32_t nt, nr;            /* 1 <= nt <= nr <= 4 (mcle_run_mimo_large_pilot: 1 <= nt <= 8, nt <= nr <= 16) */
    int32_t n_pilots;          /* nt .. 256 */
    int32_t n_symbols;         /* NSymbs per layer, >= 1 */
    int32_t demod_method;
    int32_t estimator;         /* 0 LS, 1 MMSE (nt = 1, d_mmse_matrix required) */
    int32_t random_pilots;     /* 1: drawn per realization; 0: d_pilots [nt][n_pilots] */
    int32_t mmse_filter;       /* noise_var goes into the Blast filter (set_noise_var) */
    double noise_var, pilot_power, alpha;
} mcle_mimo_pilot_cfg;
int mcle_run_mimo_pilot_link(mcle_ctx* ctx, int dtype, const mcle_mimo_pilot_cfg* cfg, uint64_t seed, uint64_t first,
                             uint64_t count, const double* d_pilots, const double* d_chan_factor, const double* d_mmse_matrix,
                             mcle_counters* d_counters, uint32_t* d_sym_err, uint32_t* d_bit_err, double* d_err, double* d_pow);

/* The same experiment on the large-array link of mcle_run_mimo_large (csrc/pipeline_mimo_large_pilot.hip): how many pilots a
 * large receive array needs before the estimate stops costing symbol errors.  Model, estimators, outputs, skip rules (a pilot
 * Gram pivot at or below 1e-12 of the trace, or either filter failing its > 1e-300 pivot test: skipped in BOTH blocks, counted in
 * n_skipped, 0xFFFFFFFF in the per-realization arrays), the meaning of every field of mcle_mimo_pilot_cfg and of every pointer
 * are those of mcle_run_mimo_pilot_link; d_counters[0] / row 0 of d_sym_err, d_bit_err [2][count]: estimated CSI, [1]: perfect CSI;
 * d_err, d_pow f64.  When d_chan_factor is NULL, H = alpha W with no product by an identity matrix.
 * What differs from mcle_run_mimo_pilot_link is the envelope and the machinery: 1 <= nt <= 8, nt <= nr <= 16 (d_chan_factor and
 * d_mmse_matrix [nr][nr] accordingly), nt <= n_pilots <= 256, n_symbols >= 1 with nr * n_symbols <= 2^31 - 1, noise_var >= 0 and
 * finite, pilot_power > 0, alpha finite, the MMSE estimator needs nt = 1 and d_mmse_matrix, fixed pilots need d_pilots,
 * count <= 2^31 - 1.  Anything else: MCLE_E_INVAL with a message naming the rule, nothing touched; count = 0 returns MCLE_OK and
 * launches nothing.  The set-up (always f64) takes one realization per row of 16 lanes, a lane per receive antenna; the walk is
 * that of mcle_run_mimo_large on the matrix cores with two left operands, every symbol and noise sample drawn once for both.
 * The draw ledger is the pilot link's, word for word (CHAN r nt + a, DATA t nt + a, NOISE r n_symbols + t, PHASE a n_pilots + p,
 * PILOT 2 ceil(n_pilots / 2) r + p), so up to 4 x 4 this entry point runs the realizations of mcle_run_mimo_pilot_link, and with
 * L = I and alpha = 1 block 1 runs those of mcle_run_mimo_large at every shape (the perfect-CSI record is bit-identical to the
 * one k_mimo_large_setup writes).  Nothing depends on the grid, on MCLE_OPT_GRID_OVERSUB or on how [first, first + count) is
 * split.  Device memory: two records of mcle_run_mimo_large's length per realization (at most 12 KiB at 8 x 16 in complex128) in
 * the context's scratch buffer, launch slices of at most 128 MiB.
 * mcle_ctx_last_kernel: "mimo_large_pilot_link f64|f32 <nr>x<nt> s<K-steps> ls|mmse". */
int mcle_run_mimo_large_pilot(mcle_ctx* ctx, int dtype, const mcle_mimo_pilot_cfg* cfg, uint64_t seed, uint64_t first,
                              uint64_t count, const double* d_pilots, const double* d_chan_factor, const double* d_mmse_matrix,
                              mcle_counters* d_counters, uint32_t* d_sym_err, uint32_t* d_bit_err, double* d_err, double* d_pow);

/* ---- Grassmannian codebooks: chordal distances and the random search (subspace/metrics.py:21-113 calc_principal_angles,
 *      calc_chordal_distance_from_principal_angles; apps/find_codebook.py:73-231 CodebookFinder) ---------------------------
 * A codebook is K precoders [Nt][Ns], row-major, complex of the call's dtype.  Q_k: an orthonormal basis of the column space of
 * precoder k (modified Gram-Schmidt with one re-orthogonalisation pass, on chip; the reference takes Householder QR -- the same
 * subspace).  d^2(a, b) = Ns - sum_{s, s'} |q_{a,s}^H q_{b,s'}|^2, clamped at 0 (= sum_i sin^2 theta_i of the principal angles,
 * the square of the reference's chordal distance).  The min distance of a codebook is the smallest d over the pairs a < b and
 * its pair the first such pair in itertools.combinations order; the best candidate of a search is the one with the largest min
 * d^2, ties to the lowest candidate index (the reference's strict >).
 * Envelope: 2 <= Nt <= 8, 1 <= Ns <= min(Nt - 1, 4), 2 <= K, K * Ns <= 256; anything else is MCLE_E_INVAL with a message that
 * names the argument (the shape rules are checked before the context).  The complex Gram matrix of the K Ns basis vectors is
 * formed on the matrix cores (v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32) as real products over the stacked [Re Q; Im Q].
 * Outputs do not depend on the grid, on MCLE_OPT_GRID_OVERSUB, on the form (MCLE_OPT_CODEBOOK_NO_PACK) or on how the candidate
 * range is split, bit for bit.
 *
 * mcle_chordal_min_dist: d_codebooks [n_codebooks][K][Nt][Ns] -> d_min_d2 [n_codebooks] (double), d_pair [n_codebooks][2]
 * (int32); d_d2 (may be NULL) [n_codebooks][K][K]: the symmetric matrix of d^2 with a zero diagonal.  n_codebooks = 0 returns
 * MCLE_OK and launches nothing.  mcle_ctx_last_kernel: "chordal_min_dist f64|f32 p<codebooks per wavefront trip>".
 *
 * mcle_codebook_generate: the candidates [first, first + count) of `seed` as they are BEFORE orthonormalisation, d_out
 * [count][K][Nt][Ns].  Draws (mcle-philox-v1; realization = candidate index, flat entry index
 * i = (k Nt + t) Ns + s): type 0 (complex) CN sample i of stream 2; type 1 (real) sqrt(2) x the real (even i) / imaginary (odd
 * i) part of CN sample i / 2 of stream 2, imaginary part 0; both then divided by the precoder's Frobenius norm; type 2 (qegt)
 * e^{j pi u_i}, u_i = uniform i of stream 3, not normalised (as the reference).
 * mcle_ctx_last_kernel: "codebook_generate f64|f32 complex|real|qegt p<P>".
 *
 * mcle_run_codebook_search: generate, orthonormalise, Gram matrix, block sums, pair minimum and best candidate in one kernel; no
 * codebook is stored.  Each wavefront keeps its running best over its trips and writes one record; a one-wavefront kernel picks
 * among the records.  out (HOST): best_index is the candidate's index in [first, first + count).  d_min_d2 [count] and d_pair
 * [count][2] (either may be NULL): every candidate's min d^2 and pair, every entry written.  count = 0 returns MCLE_OK with
 * n_candidates = 0 and launches nothing.  Blocks until the result is on the host.
 * mcle_ctx_last_kernel: "codebook_search f64|f32 complex|real|qegt p<candidates per wavefront trip>". */
enum { MCLE_CODEBOOK_COMPLEX = 0, MCLE_CODEBOOK_REAL = 1, MCLE_CODEBOOK_QEGT = 2 };
typedef struct mcle_codebook_cfg {
    int32_t K, Nt, Ns, type;
} mcle_codebook_cfg;
typedef struct mcle_codebook_result {
    uint64_t best_index;
    double best_min_d2;
    int32_t pair[2];
    uint64_t n_candidates;
} mcle_codebook_result;
int mcle_chordal_min_dist(mcle_ctx* ctx, int dtype, const void* d_codebooks, size_t n_codebooks, int K, int Nt, int Ns,
                          double* d_min_d2, int32_t* d_pair, double* d_d2);
int mcle_codebook_generate(mcle_ctx* ctx, int dtype, int type, int K, int Nt, int Ns, uint64_t seed, uint64_t first,
                           uint64_t count, void* d_out);
int mcle_run_codebook_search(mcle_ctx* ctx, int dtype, const mcle_codebook_cfg* cfg, uint64_t seed, uint64_t first,
                             uint64_t count, mcle_codebook_result* out, double* d_min_d2, int32_t* d_pair);

/* ---- limited-feedback IA: codebook channel quantizer and fused link (apps/ia/simple_maxsinr_quantized.py) ------------------
 * mcle_quantize_links: quant_small_matrix / my_quant_func (app :90-154) on a batch.  Every nr x nt block (receiver k1,
 * transmitter k2) of d_bigH [batch][K nr][K nt] is flattened row-major to v and takes the nearest row c of d_codebook
 * [n_codewords][dim = nr nt] (row = codeword, entry order = small_matrix.reshape(-1); complex of the call's dtype):
 *     metric 0 (calc_dist, app :40-63):        d = || v / ||v|| - c ||^2, evaluated as 1 + ||c||^2 - 2 Re(c^H v^) so that injected
 *                                              codewords need not have unit norm;
 *     metric 1 (calc_angle_dist, app :66-87):  d = 1 - |c^H v|^2 / (||v||^2 ||c||^2)   (codewords must be non-zero).
 * The lowest index wins a tie (numpy.argmin).  A block whose entries are all zero takes codeword 0 and d = NaN (argmin over the
 * reference's all-NaN distances).  d_index [batch][K][K] (int32); d_bigHq (may be NULL) [batch][K nr][K nt]: every block a bit copy
 * of its codeword; d_dist (may be NULL) [batch][K][K]: the chosen distance (double in either arithmetic).
 * Envelope: 1 <= K <= 4, 1 <= nr, nt <= 6, 1 <= n_codewords <= 4096, metric 0 / 1, batch K^2 <= 2^31-1; anything else is
 * MCLE_E_INVAL with a message that names the argument (the shape rules are checked before the context and the pointers).
 * batch = 0 returns MCLE_OK and launches nothing.
 * The search is a real matrix product (16 codewords x 16 links per tile, inner dimension [Re; Im] of the dim entries) on
 * v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32 followed by a column minimum taken in index order: no output depends on the grid,
 * on MCLE_OPT_GRID_OVERSUB, on the position of a link in its strip of 16 or on how a batch is split, bit for bit.  Scaling d_bigH
 * by a power of two changes nothing; multiplying a link by j changes nothing under metric 1.
 * mcle_ctx_last_kernel: "quantize_links f64|f32 m<metric>".
 *
 * mcle_run_ia_quantized: mcle_run_ia (K = 3, 2 x 2, one stream; every solver; either arithmetic) with the solver seeing only the
 * quantized channel: three launches per slice -- (1) draw big_H and quantize its 9 links (the search above), (2) redraw big_H,
 * gather the nine 2 x 2 blocks from the codebook by index, run the solver on them and record G_kl = U_k H_kl F_l on the TRUE H,
 * (3) the symbol walk of mcle_run_ia, untouched.  The draws are those of mcle_run_ia for the same (seed, realization): a perfect-CSI
 * run and a quantized run of one seed are on common random numbers.  A singular quantized system is flagged skipped as today.
 * d_sum_capacity: sum_k log2(1 + SINR_k), SINR_k = |G_kk|^2 / (sum_{l != k} |G_kl|^2 + noise_var ||U_k||^2) -- MultiUserChannelMatrix.
 * calc_SINR on the true channel (app :272-273), not the solver's own figure.  d_index (may be NULL) [count][3][3]; d_dist_sum (may
 * be NULL) [count]: the sum of the realization's nine chosen distances in link order.  qcfg: K = 3, nr = nt = 2.  As for mcle_run_ia,
 * 6 * n_symbols <= 2^31 - 1 (draw positions are 32-bit) and count <= 2^31 - 1 per call. */
enum { MCLE_QUANT_EUCLIDEAN = 0, MCLE_QUANT_CHORDAL = 1 };
typedef struct mcle_quant_cfg {
    int32_t K, nr, nt;                  /* 1 <= K <= 4, 1 <= nr, nt <= 6 : dim = nr*nt <= 36 */
    int32_t n_codewords;                /* 1 .. 4096 */
    int32_t metric;                     /* MCLE_QUANT_*: 0 calc_dist, 1 calc_angle_dist */
    int32_t reserved[3];
} mcle_quant_cfg;
int mcle_quantize_links(mcle_ctx* ctx, int dtype, const mcle_quant_cfg* cfg, const void* d_bigH, const void* d_codebook,
                        int32_t* d_index, void* d_bigHq, double* d_dist, size_t batch);
int mcle_run_ia_quantized(mcle_ctx* ctx, int dtype, const mcle_ia_cfg* cfg, const mcle_quant_cfg* qcfg, const void* d_codebook,
                          uint64_t seed, uint64_t first, uint64_t count, mcle_counters* d_counters, uint32_t* d_sym_err,
                          uint32_t* d_bit_err, double* d_sum_capacity, uint32_t* d_iterations, int32_t* d_index,
                          double* d_dist_sum);

/* ---- indoor system level: METIS test case 2, one floor (apps/metis_scenarios/simulate_metis_scenario.py, ..._scenario2.py) ---
 * The floor is rooms_per_side x rooms_per_side square rooms of side_length metres, centres as calc_room_positions_square gives
 * them (row 0 on top; the shift keeps the reference's floor division, so side_length 7.5 with 4 rooms per side has centres -11,
 * -3.5, 4, 11.5).  Access points (APs) stand in the room centres chosen by ap_decimation (get_ap_positions: 1 every room, 2 a
 * checkerboard, 4 odd rows and columns, 9 every third from 1), numbered in row-major order of their rooms.
 * A point's room is the room with the nearest centre (per axis, the lowest index on a tie).  walls(room, AP) is the Manhattan
 * distance of the room indices; the host shows per configuration that this is the reference's round(|Re| + |Im|) of
 * (room - 1.0001 AP) / side_length and refuses a configuration where it is not.  Positions, rooms and walls are f64 / integer
 * in either arithmetic; from the squared distance on everything is `dtype`.
 *     gain g[u][a] = pl(d, walls) 10^(-walls wall_loss_dB / 10),  pl the model's linear path gain with the small-distance
 *     clamp (a negative loss in dB is 0 dB, d = 0 included):
 *       MCLE_INDOOR_PL_NONE       pl = 1
 *       MCLE_INDOOR_PL_GENERAL    10 n log10(d dist_scale) + C dB   (PathLoss3GPP1 on metres: 3.76, 128.1, 1e-3; PathLossFreeSpace)
 *       MCLE_INDOOR_PL_METIS_PS7  walls = 0: 18.7 log10 d + 46.8 + 20 log10(fc_GHz / 5);
 *                                 walls > 0: 36.8 log10 d + 43.8 + 20 log10(fc_GHz / 5) + 5 (walls - 1)       (d in metres)
 *     association a*: assoc 0 the closest AP (argmin of the distance), 1 the best channel (argmax of g); the lowest index on an
 *     exact tie.
 *     SINR = tx g[u][a*] / (sum over transmitting a != a* of tx g[u][a] + noise), reported as 10 log10.
 * The interference is summed over a != a* directly, never as total minus desired.
 *
 * mcle_indoor_sinr: the heat-map operator.  d_points [n][2] (x, y in metres) -> d_sinr_dB [n] and d_assoc [n] (either may be
 * NULL).  Every AP transmits: active must be 0; n_users and the histogram fields are ignored.
 *
 * mcle_run_indoor_drops: Monte Carlo over user drops, one drop per wavefront.  Drop r (realization first + r of mcle-philox-v1)
 * places n_users users: user u at n L (u_x - 0.5) + j n L (u_y - 0.5) with u_x, u_y the uniforms 2 u and 2 u + 1 of STREAM_CHAN
 * (n = rooms_per_side, L = side_length), or at d_positions [count][U][2] when that is not NULL.  active 1 switches off every AP
 * that no user of the drop chose (simulate_metis_scenario2.py); active 0 leaves all on.
 *     capacity[u] = log2(1 + SINR) / (users of this drop on a*)                         (f64 from the dtype SINR)
 *     d_sinr_dB, d_capacity, d_assoc [count][U];  d_sum_capacity, d_sum_sinr_dB, d_min_sinr_dB [count]: over the drop's users;
 *     d_active_aps [count]: the drop's transmitting APs (all of them with active 0);
 *     d_hist [hist_bins + 2]: users by SINR in dB -- slot 0 below hist_lo_dB, slot 1 + floor((s - lo) / step) up to hist_bins,
 *     slot hist_bins + 1 at or above the top;  d_load_hist [U + 1]: slot k counts the (drop, AP) pairs with k users.
 * Both histograms ACCUMULATE into the caller's zeroed uint64 counters (exact integers).  Every output pointer may be NULL;
 * outputs are double in either arithmetic.
 * Every output of a drop is a function of (seed, drop, cfg, dtype) alone: bit for bit independent of the grid, of
 * MCLE_OPT_GRID_OVERSUB and of how [first, first + count) is split (per-drop sums are taken in a fixed lane order).
 * Envelope: rooms_per_side 1 .. 16, ap_decimation 1 / 2 / 4 / 9 with at least one AP, n_users 1 .. 256, hist_bins 0 .. 256
 * (hist_step_dB > 0 with bins), side_length > 0, wall_loss_dB >= 0, tx_power > 0, noise_power > 0 (in f32 both must be normal
 * f32 numbers, 1.18e-38 .. 3.4e38: they are rounded to f32, and a zero noise power would make a lone AP's SINR infinite), GENERAL: pl_n > 0 and
 * dist_scale > 0, PS7: fc_MHz > 0, n and count <= 2^31-1; anything else is MCLE_E_INVAL with a message that names the argument
 * (the shape rules are checked before the context and the pointers).  n = 0 / count = 0 returns MCLE_OK and launches nothing.
 * mcle_ctx_last_kernel: "indoor_sinr f64|f32 m<model> a<assoc>", "indoor_drops f64|f32 m<model> a<assoc> t<active> u<users per
 * lane: 1, 2 or 4>". */
enum { MCLE_INDOOR_PL_NONE = 0, MCLE_INDOOR_PL_GENERAL = 1, MCLE_INDOOR_PL_METIS_PS7 = 2 };
typedef struct mcle_indoor_cfg {
    int32_t rooms_per_side;   /* 1..16 */
    int32_t ap_decimation;    /* 1, 2, 4, 9; a layout with no AP is MCLE_E_INVAL */
    int32_t model;            /* MCLE_INDOOR_PL_* */
    int32_t assoc;            /* 0 closest AP (argmin distance), 1 best channel (argmax gain) */
    int32_t active;           /* 0 every AP transmits, 1 only APs some user chose (drops only) */
    int32_t n_users;          /* drops only: 1..256 */
    int32_t hist_bins;        /* 0..256 */
    int32_t reserved;
    double side_length, wall_loss_dB;
    double pl_n, pl_C, dist_scale;  /* GENERAL: 10 n log10(d * dist_scale) + C (3GPP: 3.76, 128.1, 1e-3) */
    double fc_MHz;                  /* METIS PS7 */
    double tx_power, noise_power;   /* linear */
    double hist_lo_dB, hist_step_dB;
} mcle_indoor_cfg;
int mcle_indoor_sinr(mcle_ctx* ctx, int dtype, const mcle_indoor_cfg* cfg, const double* d_points, size_t n, double* d_sinr_dB,
                     int32_t* d_assoc);
int mcle_run_indoor_drops(mcle_ctx* ctx, int dtype, const mcle_indoor_cfg* cfg, uint64_t seed, uint64_t first, uint64_t count,
                          const double* d_positions, uint64_t* d_hist, uint64_t* d_load_hist, double* d_sum_capacity,
                          double* d_sum_sinr_dB, double* d_min_sinr_dB, int32_t* d_active_aps, double* d_sinr_dB,
                          double* d_capacity, int32_t* d_assoc);

/* ---- hexagonal-cell system level: a cluster of hexagonal cells (apps/comp_BD/simulate_comp.py 'Random' users; cell/cell.py) -
 * num_cells (K, 1 .. 19) hexagonal cells of cell_radius with a base station in every centre.  The geometry is the HOST's
 * (pyphysim_amd/cell.py restates cell.Cluster): the config carries, per cell c, the positions pos_x / pos_y [pos_start[c] ..
 * pos_start[c + 1]) -- the cell's centre first, then with wrap_around (19 cells only) its two or three wrapped copies --, the
 * cluster centre and the cluster's external radius.  Positions, offsets and squared distances are f64 in either arithmetic; from
 * the logarithm of the squared distance on everything is `dtype`.
 *     distance d[p][c] = |p - centre_c|, with wrap_around the minimum over the cell's positions;
 *     gain g[p][c] = 10^(-PL_dB(d) / 10):  MCLE_HEX_PL_NONE 1;  MCLE_HEX_PL_GENERAL 10 n log10(d dist_scale) + C dB
 *         (PathLoss3GPP1 on km: 3.76, 128.1, 1; PathLossFreeSpace).  SMALL DISTANCES: a negative loss in dB is clamped to 0 dB,
 *         gain 1, d = 0 included -- the reference's handle_small_distances_bool = True; with it off the reference raises below
 *         3.9e-4 km for 3GPP1, which a Monte Carlo over 1e6 drops meets about once;
 *     interferer gain g_ext[p] = the model at external_radius - |p - cluster centre| under the same clamp (app :205-213); a
 *         point on or beyond the external circle is taken as ON the interferer (distance 0, gain 1);
 *     SINR of a point served by cell c = tx g[p][c] / (sum_{c' != c} tx g[p][c'] + ext_power g_ext[p] + noise), the
 *         interference summed directly, never as total minus desired.  n_ext only sets how often the records repeat g_ext.
 *
 * mcle_hex_gains: the operator on injected points.  d_points [n][2] (x, y) -> d_dist [n][K], d_gain [n][K + 1] (the last column
 * is the interferer), d_sinr_dB [n] (served by d_assoc), d_assoc [n]: the FIRST cell of the largest gain.  Any output may be
 * NULL; users_per_cell, min_dist_ratio and the histogram fields are ignored.
 *
 * mcle_run_hex_drops: Monte Carlo over user drops, one drop per wavefront.  Drop r (realization first + r of mcle-philox-v1)
 * places users_per_cell (U) users in every cell, user q = cell U + slot; every user is served by the cell it was dropped in.
 * Attempt t (0 <= t < 128) of user q takes the uniforms 2 (128 q + t) and 2 (128 q + t) + 1 of stream 5 (STREAM_DROP; the
 * channel stream that mcle_run_comp reads on the same (seed, realization) is not touched): the candidate centre + (2 (u_x - 1/2)
 * r, 2 (u_y - 1/2) r), every operation rounded on its own, wins if it is inside the cell (|y| < h and sqrt(3) |x| + |y| < 2 h on
 * the offset, h = sqrt(3) r / 2) and at least min_dist_ratio r from the centre.  A user that exhausts its 128 attempts
 * (probability below 1e-17) sets d_flags[r] = 1: the drop's floating outputs are NaN and it is left out of the histogram.
 * With d_positions [count][K U][2] not NULL nothing is drawn.
 *     d_flags [count] (int32); d_records [count][K U][K + n_ext]: the gains, the interferer's repeated n_ext times -- with U = 1
 *     the d_pathloss of mcle_run_comp; d_pos_out [count][K U][2]; d_sinr_dB, d_capacity [count][K U] (capacity = log2(1 +
 *     SINR), f64 from the dtype SINR); d_hist [hist_bins + 2]: users by SINR in dB as for mcle_run_indoor_drops, ACCUMULATED
 *     into the caller's zeroed uint64 counters; d_sum_capacity, d_min_sinr_dB [count]: over the drop's users.
 * Every output pointer may be NULL; outputs are double in either arithmetic.  Every output of a drop is a function of (seed,
 * drop, cfg, dtype) alone: bit for bit independent of the grid, of MCLE_OPT_GRID_OVERSUB and of how [first, first + count) is
 * split.
 * Envelope: num_cells 1 .. 19, users_per_cell >= 1 with num_cells users_per_cell <= 256, min_dist_ratio in [0, 0.7],
 * wrap_around 0 / 1 (1: 19 cells), n_ext 0 .. 8, hist_bins 0 .. 256 (hist_step_dB > 0 with bins), cell_radius > 0, GENERAL: pl_n
 * > 0 and dist_scale > 0, tx_power > 0, noise_power > 0, ext_power >= 0 (in f32 normal f32 numbers, ext_power or 0), n_pos in
 * [num_cells, 64] with pos_start from 0 to n_pos in steps of 1 (with wrap_around 1 .. 4), finite positions, external_radius > 0,
 * n and count <= 2^31-1; anything else is MCLE_E_INVAL with a message that names the argument (the rules are checked before the
 * context and the pointers).  n = 0 / count = 0 returns MCLE_OK and launches nothing.
 * mcle_ctx_last_kernel: "hex_gains f64|f32 m<model> w<wrap>", "hex_drops f64|f32 m<model> u<users per lane: 1, 2 or 4>
 * w<wrap>". */
enum { MCLE_HEX_PL_NONE = 0, MCLE_HEX_PL_GENERAL = 1 };
#define MCLE_HEX_MAX_POS 64
typedef struct mcle_hex_cfg {
    int32_t num_cells;        /* 1..19 */
    int32_t users_per_cell;   /* drops only: num_cells * users_per_cell <= 256 */
    int32_t model;            /* MCLE_HEX_PL_* */
    int32_t wrap_around;      /* 0 / 1 (19 cells only) */
    int32_t n_ext;            /* 0..8: copies of the interferer's column in the records */
    int32_t hist_bins;        /* 0..256 */
    int32_t n_pos;            /* entries of pos_x / pos_y */
    int32_t reserved;
    double cell_radius, min_dist_ratio;
    double pl_n, pl_C, dist_scale;  /* GENERAL: 10 n log10(d * dist_scale) + C (3GPP on km: 3.76, 128.1, 1) */
    double tx_power, noise_power, ext_power;   /* linear */
    double hist_lo_dB, hist_step_dB;
    double external_radius, centre_x, centre_y;
    int32_t pos_start[20];
    double pos_x[MCLE_HEX_MAX_POS], pos_y[MCLE_HEX_MAX_POS];
} mcle_hex_cfg;
int mcle_hex_gains(mcle_ctx* ctx, int dtype, const mcle_hex_cfg* cfg, const double* d_points, size_t n, double* d_dist,
                   double* d_gain, double* d_sinr_dB, int32_t* d_assoc);
int mcle_run_hex_drops(mcle_ctx* ctx, int dtype, const mcle_hex_cfg* cfg, uint64_t seed, uint64_t first, uint64_t count,
                       const double* d_positions, int32_t* d_flags, double* d_records, double* d_pos_out, double* d_sinr_dB,
                       double* d_capacity, uint64_t* d_hist, double* d_sum_capacity, double* d_min_sinr_dB);

/* ---- same-seed parity mode: NumPy's legacy global RandomState replayed on the device -------
 * Realization r receives exactly what the reference draws after np.random.seed(seed_base + r)
 * (legacy MT19937; util/misc.py:327-355 randn_c = randn real block then imag block, and
 * np.random.randint of apps/awgn_modulators/simulate_psk.py:65).  A program is a sequence of
 * segments: kind 0 = randint(0, range, n) with `range` a power of two -> int32 outputs,
 * kind 1 = randn(n) -> float64 outputs (the polar method's cached value carries over between
 * segments like NumPy's), kind 2 = rand(n) -> float64 uniforms in [0, 1).  Rows: d_int [count][n_int], d_dbl [count][n_dbl]; d_status[count] is
 * set to 1 if the word budget of a realization was exhausted (never observed; may be NULL). */
typedef struct mcle_legacy_seg {
    int32_t kind;
    int32_t n;
    uint32_t range;
    uint32_t reserved;
} mcle_legacy_seg;
int mcle_legacy_draws(mcle_ctx* ctx, const mcle_legacy_seg* segs, int n_segs, uint32_t seed_base,
                      uint64_t first, uint64_t count, int32_t* d_int, size_t n_int, double* d_dbl,
                      size_t n_dbl, uint32_t* d_status);
/* out = scale * (re + 1j*im): assembles randn_c from the two randn blocks */
int mcle_complex_from_parts(mcle_ctx* ctx, int dtype, const double* d_re, const double* d_im,
                            double scale, void* d_out, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* MCLE_H */
