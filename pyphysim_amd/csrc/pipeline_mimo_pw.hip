// pipeline_mimo_pw.hip -- config 4's link (4 x 4 Blast + OFDM, complex128) with 1 / NW OF THE TIME SAMPLES PER WAVEFRONT, NW = 2, 4, 8
// (fft_size 512, 1024, 2048): the quarter-wave kernel of pipeline_mimo_qw.hip (NW = 4 there) as a template over the number of
// wavefronts, with the decode on the matrix cores (round 6).  Same link, same draw ledger (philox.hpp), same record kernel
// (k_mimo_filters_planar) and results contract as k_run_mimo_ofdm_planar<double, N, 4, 4, ...>, whose per-realization counts it
// reproduces (reference: apps/mimo/simulate_mimo.py:68-142, mimo/mimo.py:609-660, modulators/ofdm.py:52-94, :394-466).
//
// Decomposition (pipeline_mimo_qw.hip has the long form): a workgroup of NW wavefronts is one realization, N = 256 NW.  Wavefront j
// owns the time samples n = NW m + j of ALL four antennas.  The first radix-NW DIF stage of the inverse transform,
//   x[NW m + j] = IDFT256_k' { conj(W_N)^(j k') sum_q e^(+2 pi i j q / NW) X[k' + 256 q] },
// is evaluated per wavefront for ITS j straight from the label bytes (NW table look-ups per element; recomputed, not exchanged);
// the 256-point transforms are two radix-16 register passes around one wave-private transposition; the channel is
// v_mfma_f64_4x4x4; the noise pair (2 p, 2 p + 1) is the same lane of wavefronts j and j ^ 1.  On receive the LAST radix-NW DIT stage
//   Y[k' + 256 q] = sum_j e^(-2 pi i j q / NW) W_N^(j k') Y_j[k']
// is the one exchange between the wavefronts (re planes, then im planes).
//
// What is new against pipeline_mimo_qw.hip: WHO reads the exchange.  There the thread that owns k' reads the sixteen (j, r) values
// and decodes four bins x four streams in its own registers: sixteen complex multiply-adds per bin on the VALU.  Here lane (r, g) of
// wavefront jw reads antenna r ONLY -- the NW partial transforms of its 16 / NW elements k' = g + 16 u, u in jw's share -- finishes
// the last stage for them (16 / NW butterflies of NW points) and holds Y_r at sixteen bins, while lanes (0..3, g) hold the SAME
// sixteen bins of the four receive antennas: the decode est_a = sum_r G[a][r] Y_r is the contraction over the four lanes of a column
// that the channel already is -- v_mfma_f64_4x4x4, lane (r, h) supplying G[h mod 4][r] -- and stream a's sixteen estimates land in
// lane (a, g).  Their labels are sixteen CONSECUTIVE bytes of that lane's label row ([q + NW u], u in jw's share): one 16-byte read.
// Decisions: the form fixed at compile time (walk_f64.hpp: walk_decide), four symbols at a time.
// LDS: NW planes of 8.5 KiB + tables -> 512: 27 KiB (five workgroups per CU fit, three wavefronts per SIMD = six workgroups of 128
// threads ... the register bound decides), 1024: 46 KiB (three workgroups per CU, as the quarter-wave kernel).
// Envelope: fft_size 256 NW, 4 x 4, full band, even cyclic prefix, a constellation with a certificate or the slicer.
// Round 7: the text above is the TIME-DOMAIN form (template parameter TD = true, option f64_threads = 265).  The default form leaves the
// transmit side out -- the channel is flat, so only the noise is transformed and H X joins its spectrum in front of the decode: see the
// comment at k_run_mimo_ofdm_pw.
// Round 10: the default form deals the 4 NW (antenna, time class) partial transforms BY LANE ROW (template parameter ROWS = true): lane
// row rho of wavefront w owns the pair f = NW antenna + class = 4 w + rho, so the two samples of a Philox NOISE block sit sixteen lanes
// apart in ONE wavefront and their words change rows in registers -- no LDS round trip, no barrier B1.  The map of
// the text above (wavefront = class, row = antenna) stays as ROWS = false, option f64_threads = 266: the A/B partner.
// Round 20: at 1024 and 2048 points the exchange between the wavefronts carries COMPLEX values in two halves (template parameter
// XCH = true), each lane refilling the slots it has just read: workgroup barrier B3 is not issued.  512 points and
// option f64_threads = 267 keep the re / im planes; 268 asks for the halves at every size.
#include "mimo_planar_common.hpp"
#include "walk_f64.hpp"

namespace mcle {

constexpr int kPwPlane = 4 * 272;                // doubles per wavefront plane (8 704 B): row stride 17 / 272, antenna stride 272
__host__ __device__ __forceinline__ int pw_slot(int a, int e) { return a * 272 + e + (e >> 4); }
// time index (within the wavefront's 256 samples) held by register c of lane group h after the second DIF pass
__host__ __device__ __forceinline__ int pw_mtime(int h, int c) { return (c & 3) * 64 + (c >> 2) * 16 + (h & 3) * 4 + (h >> 2); }
template <int NW> constexpr int pw_lab_stride() { return 16 * NW + 16; }     // bytes per (antenna, group) row: [q + NW u] + bank rotation
// bytes of the kernel's static LDS arrays (Box-Muller tables, label rows, two records, partial counts, totals): the launcher counts them
template <int NW> constexpr size_t pw_static_lds() {
    return (size_t)((kBmLdsDoubles + 1) & ~1) * sizeof(double) + (size_t)64 * pw_lab_stride<NW>() + 2 * (d64_rec<4, 4>() + 1) * sizeof(double2) +
           64 * sizeof(unsigned) + sizeof(WgTotals);
}

// x of the odd lane rows (16-31, 48-63) changes places with y of the even rows sixteen lanes below: v_permlane16_swap_b32
__device__ __forceinline__ void pw_row_swap(uint32_t& x, uint32_t& y) {
#if defined(__HIP_DEVICE_COMPILE__)
#if __has_builtin(__builtin_amdgcn_permlane16_swap)
    const auto s = __builtin_amdgcn_permlane16_swap(x, y, false, false);
    x = s[0];
    y = s[1];
#else
    const bool odd = (__lane_id() & 16) != 0;
    const uint32_t give = odd ? x : y, got = (uint32_t)__shfl_xor((int)give, 16);
    if (odd) x = got;
    else y = got;
#endif
#endif
}

// Output J of the first radix-NW DIF stage for the sixteen elements k' = g + 16 u of one lane, from the label bytes of its row
// (byte q + NW u = the label of bin k' + 256 q): Z_u = conj(W_N^(16 J u)) sum_q e^(2 pi i J q / NW) X_q; the lane factor
// conj(W_N^(J g)) rides on the first pass's twiddles.
template <int NW, int J, bool STUB>
__device__ __forceinline__ void pw_first_stage(const unsigned char* lab_row, const double2* s_txtab, const double2* __restrict__ g_tw,
                                               double2 (&v)[16]) {
    const uint4* lab = reinterpret_cast<const uint4*>(lab_row);
    if constexpr (NW == 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint4 L = lab[i];
            const uint32_t wds[4] = {L.x, L.y, L.z, L.w};
#pragma unroll
            for (int uu = 0; uu < 4; ++uu) {
                const int u = 4 * i + uu;
                const uint32_t w = wds[uu];
                double2 X0, X1, X2, X3;
                if constexpr (STUB) {
                    X0 = X1 = X2 = X3 = mk<double>((double)w, 1.0);
                } else {
                    X0 = s_txtab[w & 0xFFu];
                    X1 = s_txtab[(w >> 8) & 0xFFu];
                    X2 = s_txtab[(w >> 16) & 0xFFu];
                    X3 = s_txtab[w >> 24];
                }
                const double2 A = (J & 1) ? csub(X0, X2) : cadd(X0, X2);
                const double2 B = (J & 1) ? csub(X1, X3) : cadd(X1, X3);
                double2 S;
                if constexpr (J == 0) S = cadd(A, B);
                else if constexpr (J == 1) S = mk<double>(A.x - B.y, A.y + B.x);      // A + i B
                else if constexpr (J == 2) S = csub(A, B);
                else S = mk<double>(A.x + B.y, A.y - B.x);                            // A - i B
                if constexpr (J == 0) v[u] = S;
                else if (u == 0) v[u] = S;
                else v[u] = cmulc(S, g_tw[16 * J * u]);                                // uniform address: a scalar load
            }
        }
    } else if constexpr (NW == 8) {
        // sum_q w^(J q) X_q, w = e^(2 pi i / 8), as (A_0 + i^J A_2) + w^J (A_1 + i^J A_3) with A_q0 = X_q0 + (-1)^J X_(q0 + 4)
        constexpr double kH = 0.70710678118654752440;
        auto rotJ = [](double2 z) {                               // i^J z
            if constexpr ((J & 3) == 0) return z;
            else if constexpr ((J & 3) == 1) return mk<double>(-z.y, z.x);
            else if constexpr ((J & 3) == 2) return mk<double>(-z.x, -z.y);
            else return mk<double>(z.y, -z.x);
        };
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint4 L = lab[i];
            const uint32_t wds[4] = {L.x, L.y, L.z, L.w};
#pragma unroll
            for (int uu = 0; uu < 2; ++uu) {
                const int u = 2 * i + uu;
                const uint32_t w0 = wds[2 * uu], w1 = wds[2 * uu + 1];
                double2 X[8];
                if constexpr (STUB) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) X[q] = mk<double>((double)(w0 + w1), 1.0);
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        X[q] = s_txtab[(w0 >> (8 * q)) & 0xFFu];
                        X[q + 4] = s_txtab[(w1 >> (8 * q)) & 0xFFu];
                    }
                }
                double2 A[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) A[q] = (J & 1) ? csub(X[q], X[q + 4]) : cadd(X[q], X[q + 4]);
                const double2 B0 = cadd(A[0], rotJ(A[2])), B1 = cadd(A[1], rotJ(A[3]));
                double2 S;
                if constexpr (J == 0) S = cadd(B0, B1);
                else if constexpr (J == 2) S = mk<double>(B0.x - B1.y, B0.y + B1.x);              // + i B1
                else if constexpr (J == 4) S = csub(B0, B1);
                else if constexpr (J == 6) S = mk<double>(B0.x + B1.y, B0.y - B1.x);              // - i B1
                else {
                    // w^J = (c + i s) / sqrt 2: J = 1: (1, 1), 3: (-1, 1), 5: (-1, -1), 7: (1, -1)
                    constexpr double c = (J == 1 || J == 7) ? kH : -kH, sn = (J == 1 || J == 3) ? kH : -kH;
                    S = mk<double>(B0.x + (c * B1.x - sn * B1.y), B0.y + (sn * B1.x + c * B1.y));
                }
                if constexpr (J == 0) v[u] = S;
                else if (u == 0) v[u] = S;
                else v[u] = cmulc(S, g_tw[16 * J * u]);
            }
        }
    } else {
        static_assert(NW == 2, "first stage");
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const uint4 L = lab[i];
            const uint32_t wds[4] = {L.x, L.y, L.z, L.w};
#pragma unroll
            for (int uu = 0; uu < 8; ++uu) {
                const int u = 8 * i + uu;
                const uint32_t w = wds[uu >> 1] >> (16 * (uu & 1));
                double2 X0, X1;
                if constexpr (STUB) {
                    X0 = X1 = mk<double>((double)(w & 0xFFFFu), 1.0);
                } else {
                    X0 = s_txtab[w & 0xFFu];
                    X1 = s_txtab[(w >> 8) & 0xFFu];
                }
                const double2 S = J ? csub(X0, X1) : cadd(X0, X1);
                if constexpr (J == 0) v[u] = S;
                else if (u == 0) v[u] = S;
                else v[u] = cmulc(S, g_tw[16 * J * u]);
            }
        }
    }
}

// TD = false (the default form): THE SIGNAL IS ADDED AFTER THE RECEIVE TRANSFORM.  The channel is flat -- one H per realization -- so
// by linearity of the DFT  fft(H T + sigma n) = H fft(T) + fft(sigma n)  and fft(T) is the symbols themselves times tx_scale N: the
// transmit transform, its first radix-NW stage and its transposition carry X through ifft and fft back to itself and are not issued.
// Only the noise (drawn in the time domain by the same ledger, same lane / register / sample map pw_mtime) goes through the receive
// passes, the exchange and the last stage; lane (r, g) of wavefront jw then holds the NOISE spectrum of receive antenna r in register
// q + NW uu, and lane (a, g) holds the labels of stream a at exactly those bins (byte q + NW uu of the decode's 16-byte read): one
// look-up per register and  Y_r = sum_a H[r][a] X_a (tx_scale N) + noise  on v_mfma_f64_4x4x4 with the channel's own lane maps (A =
// H[h mod 4][a], B = the lane's symbol, C = the noise spectrum).  DESIGN.md 5.14 has the scale and why no count moves.
// TD = true (option f64_threads = 265): the time-domain form of round 6 -- transmit transform, channel on the samples -- kept as the
// A/B partner and second witness.
// ABL (MCLE_EXPERIMENTS builds only, option f64_variant: WRONG results by construction): 32 = no label draws / look-ups,
// 64 = no transmit passes (TD only: the default form has none, the bit switches nothing off there), 128 = no noise draws,
// 256 = no channel products (TD) / no signal contraction (default form), 512 = no receive passes, 1024 = no decode
// ROWS = true (the default form's default since round 10): OWNERSHIP BY LANE ROW.  The receive passes and the transposition work per
// lane row and do not care which (antenna, class) pair a row carries, so the 4 NW pairs, flattened f = NW antenna + class, are dealt
// f = 4 w + rho to lane row rho = lane >> 4 of wavefront w (NW = 4: wavefront = antenna, row = class).  Even and odd classes are then
// even and odd rows of one wavefront: every lane draws eight NOISE blocks -- an even row those of registers cc < 8, its partner lane
// + 16 those of registers 8 + cc -- and two row swaps per block leave (w0, w1) = the words of register cc and (w2, w3) = those of
// register 8 + cc in EVERY lane: static register indices, no select, no LDS.  With the words gone nothing is published before B2 (the
// labels of S0a are first read behind B4): barrier B1 is not issued.  Wavefront w leaves the partial spectrum of its row rho in slice
// f of the planes (272 doubles each, + 16 for an odd antenna: the rows r, r + 1 of one reading half-wave land on the two halves of
// the bank row); the reader of antenna r takes class jj from slice NW r + jj.  Every floating-point operation and its operands are
// those of ROWS = false (option f64_threads = 266) -- only the wavefront and the lane where it runs moved.
// XCH = true (what the default form by lane row runs at 1024 and 2048 points since round 20): THE EXCHANGE IN COMPLEX HALVES.  The sixteen
// elements of a lane go through LDS as complex values (16-byte stores and loads) in two halves by uu instead of as re and im planes:
// phase A carries uu < UU / 2 of every reader, phase B the rest.  A slice (272 doubles = 136 slots of 16 bytes) holds 128 values per
// phase: the writer (wavefront w, row rho) puts element k' = g + 16 (UU jw + uu) into slot g + 16 ((UU / 2) jw + uu) of slice 4 w + rho,
// and behind B2 the reader (wavefront jw, row r) takes class jj from slice NW r + jj.  Every phase-A slot is read by exactly ONE lane,
// and that lane stores its own eight phase-B values into the eight slots it has just read -- the value for (reader wavefront jw',
// uu') into the slot it read for (jj = jw', uu' - UU / 2).  A wavefront's LDS operations complete in issue order, so the store stands
// behind the load of the same slot and nobody else touches the slot in between: BARRIER B3 IS NOT ISSUED.  Behind B4 the reader finds
// (antenna r, class jj), which the pair f = NW r + jj = 4 w' + rho' computed, in slice NW rho' + jw at g + 16 ((UU / 2) w' + uu - UU / 2).
// No shift for odd antennas: the rows r, r + 1 of one 16-lane group of a 16-byte read lie a multiple of 256 bytes apart in both
// phases, sixteen consecutive slots each (tests/test_pw_exchange_layout.py replays all of it, bank conflicts included).
// BARRIER B5 behind the draw (round 20, item 2; NOT in the default build: it measured 0.1 ms per 2^20 realizations SLOWER than B5 at
// the top, profiles/r20/pw_exchange_ab.log): with XCH, -DMCLE_PW_LATE_B5 moves B5 from the top of the symbol to the first store into
// the planes (the transposition behind pass 2') -- labels, records and the draw own nothing another wavefront still reads (DESIGN.md
// 5.28 has the argument per LDS object), so decode, S0a and the whole draw run without a barrier between them.
// XCH = false (option f64_threads = 267, tag suffix "/x") is the exchange by re / im planes with B3: the witness.  ROWS = false, TD
// and the ABL builds keep it as well.
template <int NW, int DEC, int WPS, bool TD = false, int ABL = 0, bool ROWS = !TD, bool XCH = ROWS && !TD>
__global__ __launch_bounds__(64 * NW, WPS) void k_run_mimo_ofdm_pw(MimoParams pp, ModemParams<double> mp, uint64_t seed, uint64_t first,
                                                                   uint64_t count, const double2* __restrict__ g_tw,
                                                                   const double2* __restrict__ g_recs, mcle_counters* counters,
                                                                   uint32_t* __restrict__ sym_out, uint32_t* __restrict__ bit_out) {
    using T = double;
    constexpr int N = 256 * NW, NT = 4, NR = 4, kRec = d64_rec<NT, NR>(), TB = 64 * NW, UU = 16 / NW;
    constexpr int kLabStride = pw_lab_stride<NW>();
    static_assert(NW == 2 || NW == 4 || NW == 8, "wavefronts per realization");
    static_assert(!(TD && ROWS), "the time-domain form keeps the map wavefront = class");
    static_assert(!XCH || (ROWS && ABL == 0), "the exchange in complex halves belongs to the default form by lane row");
    constexpr bool kAhead = ROWS && ABL == 0;
#ifdef MCLE_PW_LATE_B5
    constexpr bool kLateB5 = XCH && kAhead;
#else
    constexpr bool kLateB5 = false;
#endif
    constexpr int kLogNW = NW == 2 ? 1 : NW == 4 ? 2 : 3;
    extern __shared__ __attribute__((aligned(16))) char pw_smem[];
    // Round 8: everything of a FIXED size is a static array -- the Box-Muller tables, the label rows, the records, the partial counts, the
    // totals -- so its address is a compile-time constant and a look-up is its index plus an immediate offset.  Behind the dynamic
    // block's base (and, before, behind the two constellation tables, whose length is a launch parameter) every table read of the
    // noise draw paid a vector add of a run-time base.  The dynamic block keeps the planes and the two tables.
    constexpr int kBm = (kBmLdsDoubles + 1) & ~1;
    __shared__ __attribute__((aligned(16))) double s_bm[kBm];                          // Box-Muller tables
    __shared__ __attribute__((aligned(16))) unsigned char s_lab[64 * kLabStride];       // [4][16][kLabStride] labels
    __shared__ __attribute__((aligned(16))) cx<T> s_rec[2 * (kRec + 1)];                // [2][kRec + 1]
    __shared__ unsigned s_part[64];                                                     // [2][16][2]
    __shared__ WgTotals totals;
    static_assert(sizeof(s_bm) + sizeof(s_lab) + sizeof(s_rec) + sizeof(s_part) + sizeof(totals) == pw_static_lds<NW>(), "launcher's LDS sum");
    T* s_R = reinterpret_cast<T*>(pw_smem);                                  // [NW wavefronts][kPwPlane]: scratch plane of wavefront j
    cx<T>* s_table = reinterpret_cast<cx<T>*>(s_R + NW * kPwPlane);           // [tab_len] constellation
    cx<T>* s_txtab = s_table + ((mp.M + 1) & ~1);                             // [tab_len] constellation x tx scale (TD) / x tx scale N

    const int tid = threadIdx.x, lane = tid & 63;
    const int j = __builtin_amdgcn_readfirstlane(tid >> 6);                 // this wavefront's time class n mod NW (scalar)
    const int pj = j & 1;
    const int cp = pp.cp;
    const int per_sym = N * NT;
    const uint64_t row = (uint64_t)pp.n_ofdm_sym * (N + cp);
    const T sigma = (T)sqrt(pp.noise_var);
    const T tx_scale = (T)(1.0 / sqrt((double)NT) / sqrt((double)(N + cp)));
    // the receive passes are un-normalized and the record's G carries rx_scale = sqrt(N + cp) / N: a symbol that went through the
    // un-normalized inverse and forward transforms comes back times N
    const T tab_scale = TD ? tx_scale : tx_scale * (T)N;
    const uint32_t mask = (uint32_t)(mp.M - 1);
    for (int m = tid; m < mp.M; m += TB) {
        const cx<T> c = mp.g_table[m];
        s_table[m] = c;
        s_txtab[m] = cscale(c, tab_scale);
    }
    if constexpr (ROWS) bm_tables_to_lds_pairs(s_bm, tid, TB);        // (same size: the pair tables first, each pair one 16-byte read)
    else bm_tables_to_lds(s_bm, tid, TB);
    if (tid == 0) wg_zero(totals);

    T* s_mine = s_R + j * kPwPlane;
    uint2* s_words_mine = reinterpret_cast<uint2*>(s_mine);                // [16 slots][64 lanes] word pairs of MY samples
    // (the pass count of a workgroup: a launch has at most 2^20 realizations, 32 bits hold it -- one lane instead of two)
    using Pass = std::conditional_t<kAhead, uint32_t, uint64_t>;
    Pass it = 0;
    uint64_t rl_prev = 0;
    cx<T> rec_next = mk<T>(0, 0);
    if (tid < kRec && blockIdx.x < count) rec_next = g_recs[(uint64_t)blockIdx.x * kRec + tid];
    // Round 22 (default form by lane row): THE HEAD OF THE REALIZATION LOOP.  The kernel holds more scalars than it has scalar
    // registers, and what does not fit lives in the lanes of one vector register: every reload is a v_readlane_b32, every update a
    // v_writelane_b32, on the issue slots the kernel is bound by.  The step of the loop is read ONCE as a value (it was a pointer
    // into the launch arguments, two lanes, and a scalar load with its wait twice per realization), and what only thread 0 needs
    // one realization later -- where the previous realization's two counts go -- is formed inside account_prev()'s branch.
    // (every other form reads gridDim.x where it did: their code is the witness)
    unsigned step = 0;
    if constexpr (kAhead) {
        step = gridDim.x;
        asm volatile("" : "+s"(step));
    }
    auto grid_step = [&]() -> unsigned {
        if constexpr (kAhead) return step;
        else return gridDim.x;
    };
    __syncthreads();
    for (uint64_t rl = blockIdx.x; rl < count; rl += grid_step(), ++it) {
        const Rng rng(seed, first + rl);
        const int buf = (int)(it & 1);
        if (tid < kRec) {                                                   // (first read after the next workgroup barrier)
            s_rec[buf * (kRec + 1) + tid] = rec_next;
            if (rl + grid_step() < count) rec_next = g_recs[(rl + grid_step()) * kRec + tid];
        }
        const cx<T>* s_H = s_rec + buf * (kRec + 1);                        // [NR][NT]
        const cx<T>* s_G = s_H + NT * NR;                                   // [NT][NR]
        unsigned se = 0, be = 0;
        for (int os = 0; os < pp.n_ofdm_sym; ++os) {
            // B5: the previous symbol's exchange planes and labels have been read (kLateB5: in front of the first store into the planes)
            if constexpr (!kLateB5) {
                if (it > 0 || os > 0) __syncthreads();
            }
            // The loop comes back here with scalar loads of the decode on the books, and a scalar load returns out of order: the first
            // LDS wait behind it can only be lgkmcnt(0), which in the pipelined draw would wait for block 1's table reads three
            // instructions behind their issue.  Retire them here, behind the barrier, where nothing is in flight: the draw's first wait
            // is then a counted one like the others (s_waitcnt lgkmcnt(0) alone: vmcnt and expcnt fields at their maxima).
            if constexpr (ROWS && !(ABL & 128)) __builtin_amdgcn_s_waitcnt(0xC07F);
            // ---- S0a: this thread's DATA block: subcarriers d = 4 tid .. 4 tid + 3, four antennas each -> label bytes, laid out
            //      [antenna][group g = k' mod 16][q + NW u] for bin k = k' + 256 q, k' = g + 16 u (full band: k = d ^ (N / 2)) ----
            {
                const int t = opaque(tid);
                Words4 dw;
                if constexpr (ABL & 32) dw.w[0] = dw.w[1] = dw.w[2] = dw.w[3] = (uint32_t)t * 0x01010101u;
                else dw = rng.block(STREAM_DATA, (uint32_t)(((uint64_t)os * per_sym) >> 4) + (uint32_t)t);
                const int q = (t >> 6) ^ (NW / 2), u = (t & 63) >> 2;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const uint32_t w = dw.w[s] & (mask * 0x01010101u);
                    const int g = 4 * (t & 3) + s;
                    unsigned char* dst = s_lab + g * kLabStride + NW * u + q;
#pragma unroll
                    for (int a = 0; a < 4; ++a) dst[a * 16 * kLabStride] = (unsigned char)(w >> (8 * a));
                }
            }
            // ---- S0b: the NOISE blocks of half of this lane's sixteen sample pairs: words 0, 1 are the even sample's (wavefront j & ~1),
            //      words 2, 3 the odd one's (j | 1), both through the scratch planes (read back before the channel).  Which plane is
            //      mine is wave-uniform: the two destinations are chosen once, no word pair goes through a select ----
            if constexpr (!ROWS) {
                const int ln = opaque(lane);
                const int r = ln >> 4, h = ln & 15;
                // register c = 8 pj + cc holds sample time n = NW pw_mtime(h, c) + j, pw_mtime(h, c) = pw_mtime(h, cc) + 32 pj; the pair's
                // even sample has the flat index i0 = r row + os (N + cp) + cp + NW mtime + (j & ~1): block i0 / 2 = b0 + (NW / 2) pw_mtime(0, cc)
                const uint64_t i00 = (uint64_t)r * row + (uint64_t)os * (N + cp) + cp + (j & ~1) + 32 * NW * pj + NW * (uint64_t)pw_mtime(h, 0);
                const uint32_t b0 = (uint32_t)(i00 >> 1);
                uint2* w_even = reinterpret_cast<uint2*>(s_R + (j & ~1) * kPwPlane) + (8 * pj) * 64 + ln;
                uint2* w_odd = reinterpret_cast<uint2*>(s_R + (j | 1) * kPwPlane) + (8 * pj) * 64 + ln;
#pragma unroll
                for (int cc = 0; cc < 8; ++cc) {
                    Words4 b;
                    if constexpr (ABL & 128) b.w[0] = b.w[1] = b.w[2] = b.w[3] = b0 + cc;
                    else b = rng.block(STREAM_NOISE, b0 + (uint32_t)(NW / 2) * (uint32_t)pw_mtime(0, cc));
                    w_even[cc * 64] = make_uint2(b.w[0], b.w[1]);
                    w_odd[cc * 64] = make_uint2(b.w[2], b.w[3]);
                }
            }
            // every wave is past the previous realization: account it (ROWS: behind B2, the first barrier of the symbol)
            auto account_prev = [&]() {
                if (tid == 0 && os == 0 && it > 0) {
                    const unsigned* qq = s_part + (buf ^ 1) * 32;
                    unsigned ts = 0, tb = 0;
#pragma unroll
                    for (int i = 0; i < NW; ++i) {
                        ts += qq[2 * i];
                        tb += qq[2 * i + 1];
                    }
                    // (kAhead: the previous realization's index from this one's INSIDE the branch -- formed at the loop head, the two
                    //  output addresses were computed by every wavefront, parked in four lanes and read back here by thread 0 alone)
                    uint64_t rp = rl_prev;
                    if constexpr (kAhead) {
                        uint64_t here = rl;
                        asm volatile("" : "+s"(here));
                        rp = here - step;
                    }
                    wg_account(totals, ts, tb, s_rec[(buf ^ 1) * (kRec + 1) + 2 * NT * NR].x != 0.0, rp, sym_out, bit_out);
                }
            };
            if constexpr (!ROWS) {
                __syncthreads();                              // B1: labels and word pairs in place
                account_prev();
            }
            cx<T> v[16];
            // ---- S1: lane (a, g): the first-stage output of this wavefront's time class for k' = g + 16 u; compiled per class ----
            if constexpr (TD) {
                const int ln = opaque(lane);
                const unsigned char* lab = s_lab + ln * kLabStride;                // (a * 16 + g) = lane
                if constexpr (NW == 4) {
                    switch (j) {
                        case 0: pw_first_stage<4, 0, (ABL & 32) != 0>(lab, s_txtab, g_tw, v); break;
                        case 1: pw_first_stage<4, 1, (ABL & 32) != 0>(lab, s_txtab, g_tw, v); break;
                        case 2: pw_first_stage<4, 2, (ABL & 32) != 0>(lab, s_txtab, g_tw, v); break;
                        default: pw_first_stage<4, 3, (ABL & 32) != 0>(lab, s_txtab, g_tw, v); break;
                    }
                } else if constexpr (NW == 8) {
                    switch (j) {
                        case 0: pw_first_stage<8, 0, (ABL & 32) != 0>(lab, s_txtab, g_tw, v); break;
                        case 1: pw_first_stage<8, 1, (ABL & 32) != 0>(lab, s_txtab, g_tw, v); break;
                        case 2: pw_first_stage<8, 2, (ABL & 32) != 0>(lab, s_txtab, g_tw, v); break;
                        case 3: pw_first_stage<8, 3, (ABL & 32) != 0>(lab, s_txtab, g_tw, v); break;
                        case 4: pw_first_stage<8, 4, (ABL & 32) != 0>(lab, s_txtab, g_tw, v); break;
                        case 5: pw_first_stage<8, 5, (ABL & 32) != 0>(lab, s_txtab, g_tw, v); break;
                        case 6: pw_first_stage<8, 6, (ABL & 32) != 0>(lab, s_txtab, g_tw, v); break;
                        default: pw_first_stage<8, 7, (ABL & 32) != 0>(lab, s_txtab, g_tw, v); break;
                    }
                } else {
                    if (j == 0) pw_first_stage<2, 0, (ABL & 32) != 0>(lab, s_txtab, g_tw, v);
                    else pw_first_stage<2, 1, (ABL & 32) != 0>(lab, s_txtab, g_tw, v);
                }
            }
            // ---- transmit transform, pass 1 (DIF spans 64, 16 of the 256-point transforms; registers to registers) ----
            if constexpr (TD && !(ABL & 64)) {
                const int g = opaque(lane) & 15;
                R16Tw64<T> tw;
#pragma unroll
                for (int m = 1; m <= 3; ++m) {
                    tw.a1[m - 1] = g_tw[g * (NW * m + j)];                       // W_256^(g m) x the lane factor W_N^(j g)
                    tw.a2[m - 1] = g_tw[4 * NW * g * m];
                }
                const cx<T> f0 = g_tw[g * j];
                r16_pass<T, true, false, 0, false, true, true>(nullptr, nullptr, 0, tw, nullptr, 0, v, v);
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = cmulc(v[q], f0);             // row m' = 0 takes the lane factor by itself
            }
            // ---- the word pairs of my sixteen noise samples (before the scratch plane is reused) ----
            uint2 nw[16];
            if constexpr (!ROWS) {
                const int ln = opaque(lane);
#pragma unroll
                for (int c = 0; c < 16; ++c) nw[c] = s_words_mine[c * 64 + ln];
            }
            // ---- transposition (a, g | u) -> (a, h | c): element g + 16 u = 16 h + c, re plane then im plane ----
            if constexpr (TD) {
                const int ln = opaque(lane);
                const int a = ln >> 4, g = ln & 15;
                const int wbase = pw_slot(a, g), rbase = pw_slot(a, 16 * g);       // element g + 16 u: wbase + 17 u; 16 g + c: rbase + c
                T xr[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) s_mine[wbase + 17 * u] = v[u].x;
                walk_wave_order();
#pragma unroll
                for (int c = 0; c < 16; ++c) xr[c] = s_mine[rbase + c];
                walk_wave_order();
#pragma unroll
                for (int u = 0; u < 16; ++u) s_mine[wbase + 17 * u] = v[u].y;
                walk_wave_order();
#pragma unroll
                for (int c = 0; c < 16; ++c) v[c] = mk<T>(xr[c], s_mine[rbase + c]);
            }
            // ---- pass 2 (spans 4, 1: sixteen consecutive elements, constant roots only) ----
            if constexpr (TD && !(ABL & 64)) {
                R16Tw64<T> none;
                r16_pass<T, true, false, 0, false, true, true, false, true>(nullptr, nullptr, 0, none, nullptr, 0, v, v);
            }
            // ---- default form: the noise alone, lane (r, h), register c = sample NW pw_mtime(h, c) + j of receive antenna r ----
            if constexpr (!TD && !ROWS) {
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    if constexpr (ABL & 128) v[c] = mk<T>((T)nw[c].x, sigma);
                    else v[c] = cn_words(nw[c].x, nw[c].y, sigma, s_bm);
                }
            }
            // ---- ROWS: lane (rho, h) of wavefront j, register c = sample NW pw_mtime(h, c) + class of the pair f = 4 j + rho.  The
            //      block of registers (cc, 8 + cc) of an even row is drawn by the row itself (cc) and by the row above (8 + cc:
            //      pw_mtime(h, 8 + cc) = pw_mtime(h, cc) + 32); its flat sample index is i0 = antenna row + os (N + cp) + cp +
            //      NW mtime + (class & ~1), block i0 / 2 as in S0b ----
            if constexpr (ROWS) {
                const int ln = opaque(lane);
                const int rho = ln >> 4, h = ln & 15;
                const int f = 4 * j + rho, ant = f >> kLogNW, cls = f & (NW - 1);
                const uint64_t i00 = (uint64_t)ant * row + (uint64_t)os * (N + cp) + cp + (cls & ~1) + 32 * NW * (rho & 1) + NW * (uint64_t)pw_mtime(h, 0);
                const uint32_t b0 = (uint32_t)(i00 >> 1);
                if constexpr (ABL & 128) {
#pragma unroll
                    for (int cc = 0; cc < 8; ++cc) {
                        Words4 b;
                        b.w[0] = b.w[1] = b.w[2] = b.w[3] = b0 + cc;
                        pw_row_swap(b.w[0], b.w[2]);
                        pw_row_swap(b.w[1], b.w[3]);
                        v[cc] = mk<T>((T)b.w[0], sigma);
                        v[8 + cc] = mk<T>((T)b.w[2], sigma);
                    }
                } else {
                    // Round 17: THE DRAW IS PIPELINED ONE BLOCK DEEP.  A sample's three table reads take their addresses from Philox words
                    // and its arithmetic starts with their values: compiled sample after sample, every read was waited on in full about
                    // five instructions behind its issue, forty times per realization, and the wavefront had nothing of its own to
                    // cover it.  Block cc + 1 is FETCHED -- Philox, the two row swaps, the integer parts and the six reads of its two
                    // samples (cn_fetch_lds_pairs) -- before block cc is FINISHED (cn_finish: the arithmetic of cn_from_words_lds_pairs,
                    // word for word), and the scheduling barriers hold that order: a read is now a block's arithmetic ahead of the
                    // counted wait that covers it.  Same words, same reads, same values, same registers v[cc], v[8 + cc].
                    BmFetched ft[8][2];
                    auto fetch = [&](int cc) {
                        Words4 b = rng.block(STREAM_NOISE, b0 + (uint32_t)(NW / 2) * (uint32_t)pw_mtime(0, cc));
                        pw_row_swap(b.w[0], b.w[2]);
                        pw_row_swap(b.w[1], b.w[3]);
                        ft[cc][0] = cn_fetch_lds_pairs(b.w[0], b.w[1], s_bm);
                        ft[cc][1] = cn_fetch_lds_pairs(b.w[2], b.w[3], s_bm);
                    };
                    fetch(0);
#pragma unroll
                    for (int cc = 0; cc < 8; ++cc) {
                        if (cc + 1 < 8) fetch(cc + 1);
                        __builtin_amdgcn_sched_barrier(0);
                        v[cc] = cn_finish(ft[cc][0], sigma);
                        v[8 + cc] = cn_finish(ft[cc][1], sigma);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
            // ---- channel: R_r = sum_a H[r][a] T_a + noise on v_mfma_f64_4x4x4 (pipeline_mimo_qw.hip: the lane maps) ----
            if constexpr (TD) {
                const int ln = opaque(lane);
                const cx<T> hA = s_H[(ln & 3) * NT + (ln >> 4)];                   // H[h mod 4][a]
                const T hre = hA.x, him = hA.y, nhim = -hA.y;
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    cx<T> z;
                    if constexpr (ABL & 128) z = mk<T>((T)nw[c].x, sigma);
                    else z = cn_words(nw[c].x, nw[c].y, sigma, s_bm);
                    if constexpr (ABL & 256) {
                        v[c] = cadd(v[c], z);
                    } else {
                        T yr = __builtin_amdgcn_mfma_f64_4x4x4f64(hre, v[c].x, z.x, 0, 0, 0);
                        T yi = __builtin_amdgcn_mfma_f64_4x4x4f64(him, v[c].x, z.y, 0, 0, 0);
                        yr = __builtin_amdgcn_mfma_f64_4x4x4f64(nhim, v[c].y, yr, 0, 0, 0);
                        yi = __builtin_amdgcn_mfma_f64_4x4x4f64(hre, v[c].y, yi, 0, 0, 0);
                        v[c] = mk<T>(yr, yi);
                    }
                }
            }
            // ---- receive transform: pass 2' (DIT spans 1, 4), transposition back, pass 1' (spans 16, 64) ----
            // Round 22 (default form by lane row): the six twiddles of pass 1' go out HERE, behind the draw and in front of pass 2' --
            // their addresses depend on the lane alone, the fetched samples of the draw are dead, and behind the transposition three
            // of them were waited on five to eight instructions behind their issue.  (In front of the transposition's first store
            // the whole transposition lies between issue and wait, but it is LDS traffic: eight VALU instructions.)  The same loads,
            // the same values; the scheduling barrier keeps pass 2' behind them.
            R16Tw64<T> tw1;                                                       // the twiddles of pass 1'
            if constexpr (kAhead) {
                const int g = opaque(lane) & 15;
#pragma unroll
                for (int m = 1; m <= 3; ++m) {
                    tw1.a1[m - 1] = g_tw[NW * g * m];
                    tw1.a2[m - 1] = g_tw[4 * NW * g * m];
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (!(ABL & 512)) {
                R16Tw64<T> none;
                r16_pass<T, false, true, 0, false, true, true, false, true>(nullptr, nullptr, 0, none, nullptr, 0, v, v);
            }
            {
                const int ln = opaque(lane);
                const int a = ln >> 4, g = ln & 15;
                const int wbase = pw_slot(a, g), rbase = pw_slot(a, 16 * g);
                T xr[16];
                // B5 (kLateB5): this is the symbol's first store into a plane, and the other wavefronts' phase-B loads of the previous
                // symbol read this one -- S0a, the draw and pass 2' above touch nothing that the previous symbol still reads
                // (the sixteen samples are pinned in front of the branch: left alone the compiler sinks every cn_finish of the draw below the
                //  conditional barrier, keeps all sixteen fetched samples alive up to it and spills a hundred registers)
                if constexpr (kLateB5) {
#pragma unroll
                    for (int c = 0; c < 16; ++c) asm volatile("" : "+v"(v[c].x), "+v"(v[c].y));
                    if (it > 0 || os > 0) __syncthreads();
                }
#pragma unroll
                for (int c = 0; c < 16; ++c) s_mine[rbase + c] = v[c].x;
                walk_wave_order();
#pragma unroll
                for (int u = 0; u < 16; ++u) xr[u] = s_mine[wbase + 17 * u];
                walk_wave_order();
#pragma unroll
                for (int c = 0; c < 16; ++c) s_mine[rbase + c] = v[c].y;
                walk_wave_order();
#pragma unroll
                for (int u = 0; u < 16; ++u) v[u] = mk<T>(xr[u], s_mine[wbase + 17 * u]);
            }
            if constexpr (!(ABL & 512)) {
                if constexpr (!kAhead) {
                    const int g = opaque(lane) & 15;
#pragma unroll
                    for (int m = 1; m <= 3; ++m) {
                        tw1.a1[m - 1] = g_tw[NW * g * m];
                        tw1.a2[m - 1] = g_tw[4 * NW * g * m];
                    }
                }
                r16_pass<T, false, true, 0, false, true, true>(nullptr, nullptr, 0, tw1, nullptr, 0, v, v);
            }
            // ---- the exchange: Y_j[k'] of receive antenna r (lane (r, g), register u: k' = g + 16 u) -> plane j at r 272 + k', re then
            //      im; lane (r, g) of wavefront jw reads the NW partial transforms of ITS k' = g + 16 (UU jw + uu), antenna r only ----
            T er[NW][UU], ei[NW][UU];
            cx<T> ez[NW][UU];                                                     // (XCH) the same values as complex numbers
            // Round 17 (default form by lane row): what the code behind B4 reads and the exchange does not write -- the lane's label
            // row, H[h mod 4][a], G[h mod 4][r], the last stage's twiddles of uu = 0 -- is read BEFORE the wait at B4, so its latency
            // runs while the wavefront stands at the barrier; the twiddles of uu + 1 are then issued ahead of the butterflies of uu.
            // The same loads, the same values, another place.
            constexpr uint32_t kTwBytes = (uint32_t)sizeof(cx<T>);                // one twiddle table entry; 16 entries from uu to uu + 1
            uint32_t kp0 = 0;
            // W_N^(m kp), kp = kp0 + 16 uu: table m is ONE lane offset 16 m kp0 bytes behind the (scalar) table pointer and uu only moves
            // the load's immediate, 16 sizeof(entry) m uu = 256 m uu < 4 096 bytes -- left to itself the compiler saw g + 16 (...) as an `or` and rebuilt
            // every one of the addresses in 64 bits (round 15; the same loads, the same values)
            static_assert(16 * kTwBytes * (NW - 1) * (UU - 1) < 4096, "the load's immediate offset");
            auto tw_at = [&](int m, int uu) {
                const char* lane_base = reinterpret_cast<const char*>(g_tw) + (size_t)(kTwBytes * (uint32_t)m * kp0);
                return *reinterpret_cast<const cx<T>*>(lane_base + 16 * (int)kTwBytes * m * uu);
            };
            cx<T> twb[2][NW - 1];                                                 // (kAhead) twiddles of uu in twb[uu & 1]
            uint4 lab_ahead = make_uint4(0, 0, 0, 0);
            cx<T> hA_ahead = mk<T>(0, 0), gA_ahead = mk<T>(0, 0);
            if constexpr (XCH) {
                const int ln = opaque(lane);
                const int r = ln >> 4, g = ln & 15;
                constexpr int UH = UU / 2, kSl = 272 / 2;                           // uu per phase; 16-byte slots per slice
                cx<T>* s_X = reinterpret_cast<cx<T>*>(s_R);
                const int wA = (4 * j + r) * kSl + g;                              // phase A store: slice 4 j + r, slot g + 16 (UH jw + uu)
                const int rA = NW * r * kSl + g + 16 * UH * j;                     // phase A load (+ jj slices, + 16 uu) = phase B store
                // phase B load: (antenna r, class jj) was computed by the pair f = NW r + jj = 4 w' + rho' and lies in slice NW rho' + j
                // at g + 16 (UH w' + uu - UH).  NW = 2: w' = r >> 1, rho' = 2 (r & 1) + jj; NW = 4, 8: w' = (NW / 4) r + (jj >> 2), rho' = jj & 3
                const int rB = NW == 2 ? (4 * (r & 1) + j) * kSl + g + 16 * UH * (r >> 1) : j * kSl + g + 16 * UH * (NW / 4) * r;
                r16_wave_sync();                               // (my own reads of the transposition are done)
                // THE ROUNDINGS OF PASS 1' ARE KEPT BY KEEPING ITS BASIC BLOCKS.  -ffp-contract=fast fuses a product and a sum only inside one
                // basic block.  In the re / im exchange the real parts were consumed in front of the branch of account_prev() and the
                // imaginary parts behind it: the compiler sank the last imaginary sums of the pass below that branch, and two of them
                // -- y h - x h of the roots (1 -/+ i) / sqrt 2 -- stayed a v_mul_f64 and a v_add_f64 there.  With all sixteen values
                // consumed in one block they become v_fma_f64: 2 of 1 553 static f64 instructions, another last bit in the noise
                // spectrum.  So the real parts are pinned here, the previous realization is accounted (one branch, thread 0), and the
                // imaginary parts are pinned behind it: kernel_census.py counts the parent's f64 instructions opcode for opcode.
                // account_prev() in front of B2 is safe: it runs at os = 0, it > 0 only, where this symbol's B5 -- at the top or in
                // front of the transposition -- has been passed, i.e. every wavefront has left the previous realization and its
                // s_part entries; s_part[buf ^ 1] and the flag of s_rec[buf ^ 1] are next written a realization later.
#pragma unroll
                for (int u = 0; u < 16; ++u) asm volatile("" : "+v"(v[u].x));
                account_prev();
#pragma unroll
                for (int u = 0; u < 16; ++u) asm volatile("" : "+v"(v[u].y));
#pragma unroll
                for (int jw = 0; jw < NW; ++jw)
#pragma unroll
                    for (int uu = 0; uu < UH; ++uu) s_X[wA + 16 * (UH * jw + uu)] = v[UU * jw + uu];
                __syncthreads();                               // B2
#pragma unroll
                for (int jj = 0; jj < NW; ++jj)
#pragma unroll
                    for (int uu = 0; uu < UH; ++uu) ez[jj][uu] = s_X[rA + jj * kSl + 16 * uu];
                // no B3: each slot is refilled by the lane that has just read it, behind that read in the wavefront's LDS queue
#pragma unroll
                for (int jw = 0; jw < NW; ++jw)
#pragma unroll
                    for (int uu = UH; uu < UU; ++uu) s_X[rA + jw * kSl + 16 * (uu - UH)] = v[UU * jw + uu];
                kp0 = (uint32_t)opaque((ln & 15) + 16 * UU * j);
#pragma unroll
                for (int m = 1; m < NW; ++m) twb[0][m - 1] = tw_at(m, 0);
                lab_ahead = *reinterpret_cast<const uint4*>(s_lab + ln * kLabStride + 16 * j);
                hA_ahead = s_H[(ln & 3) * NT + (ln >> 4)];
                gA_ahead = s_G[(ln & 3) * NR + (ln >> 4)];
                __syncthreads();                               // B4
#pragma unroll
                for (int jj = 0; jj < NW; ++jj) {
                    const int off = NW == 2 ? 2 * jj * kSl : (jj & 3) * NW * kSl + 16 * UH * (jj >> 2);
#pragma unroll
                    for (int uu = UH; uu < UU; ++uu) ez[jj][uu] = s_X[rB + off + 16 * (uu - UH)];
                }
            } else {
                const int ln = opaque(lane);
                const int r = ln >> 4, g = ln & 15;
                // ROWS: my row r carries the pair f = 4 j + r -> slice f = row r of my plane, + 16 for an odd antenna; antenna r's
                // class jj is slice NW r + jj
                constexpr int kClass = ROWS ? 272 : kPwPlane;  // doubles from class jj to class jj + 1 of one antenna
                const int wpos = r * 272 + g + (ROWS ? 16 * (((4 * j + r) >> kLogNW) & 1) : 0);
                const int rpos = (ROWS ? NW * r * 272 + 16 * (r & 1) : r * 272) + g + 16 * UU * j;
                r16_wave_sync();                               // (my own reads of the transposition are done)
#pragma unroll
                for (int u = 0; u < 16; ++u) s_mine[wpos + 16 * u] = v[u].x;
                __syncthreads();                               // B2
                if constexpr (ROWS) account_prev();
#pragma unroll
                for (int jj = 0; jj < NW; ++jj)
#pragma unroll
                    for (int uu = 0; uu < UU; ++uu) er[jj][uu] = s_R[jj * kClass + rpos + 16 * uu];
                __syncthreads();                               // B3
#pragma unroll
                for (int u = 0; u < 16; ++u) s_mine[wpos + 16 * u] = v[u].y;
                if constexpr (kAhead) {
                    kp0 = (uint32_t)opaque((ln & 15) + 16 * UU * j);
#pragma unroll
                    for (int m = 1; m < NW; ++m) twb[0][m - 1] = tw_at(m, 0);
                    lab_ahead = *reinterpret_cast<const uint4*>(s_lab + ln * kLabStride + 16 * j);
                    hA_ahead = s_H[(ln & 3) * NT + (ln >> 4)];
                    gA_ahead = s_G[(ln & 3) * NR + (ln >> 4)];
                }
                __syncthreads();                               // B4
#pragma unroll
                for (int jj = 0; jj < NW; ++jj)
#pragma unroll
                    for (int uu = 0; uu < UU; ++uu) ei[jj][uu] = s_R[jj * kClass + rpos + 16 * uu];
            }
            // ---- last radix-NW stage for my UU elements (register q + NW uu = bin k' + 256 q), [default form: the signal,] decode on
            //      the matrix cores, decisions ----
            if constexpr (!(ABL & 1024)) {
                const int ln = opaque(lane);
                if constexpr (!kAhead) kp0 = (uint32_t)opaque((ln & 15) + 16 * UU * j);
                // kAhead: the twiddles of uu were loaded one step ahead (uu = 0: before B4), those of uu + 1 go out before the butterflies of uu
                auto ex = [&](int jj, int uu) {
                    if constexpr (XCH) return ez[jj][uu];
                    else return mk<T>(er[jj][uu], ei[jj][uu]);
                };
                auto tw_of = [&](int m, int uu) {
                    if constexpr (kAhead) return twb[uu & 1][m - 1];
                    else return tw_at(m, uu);
                };
#pragma unroll
                for (int uu = 0; uu < UU; ++uu) {
                    if constexpr (kAhead) {
                        if (uu + 1 < UU) {
#pragma unroll
                            for (int m = 1; m < NW; ++m) twb[(uu + 1) & 1][m - 1] = tw_at(m, uu + 1);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    if constexpr (NW == 4) {
                        const cx<T> w1 = tw_of(1, uu), w2 = tw_of(2, uu), w3 = tw_of(3, uu);
                        const cx<T> u0 = ex(0, uu);
                        const cx<T> u1 = cmul(ex(1, uu), w1);
                        const cx<T> u2 = cmul(ex(2, uu), w2);
                        const cx<T> u3 = cmul(ex(3, uu), w3);
                        CxOps<T>::template bfly4<false>(u0, u1, u2, u3, v[4 * uu], v[4 * uu + 1], v[4 * uu + 2], v[4 * uu + 3]);
                    } else if constexpr (NW == 8) {
                        // Y_q = E_q + w'^q O_q, Y_(q + 4) = E_q - w'^q O_q, E / O = the 4-point forward transforms of the even / odd
                        // partial transforms, w' = e^(-2 pi i / 8)
                        cx<T> x[8];
                        x[0] = ex(0, uu);
#pragma unroll
                        for (int jj = 1; jj < 8; ++jj) x[jj] = cmul(ex(jj, uu), tw_of(jj, uu));
                        cx<T> E[4], O[4];
                        CxOps<T>::template bfly4<false>(x[0], x[2], x[4], x[6], E[0], E[1], E[2], E[3]);
                        CxOps<T>::template bfly4<false>(x[1], x[3], x[5], x[7], O[0], O[1], O[2], O[3]);
                        constexpr T kH = (T)0.70710678118654752440;
                        const cx<T> t0 = O[0];
                        const cx<T> t1 = mk<T>(kH * (O[1].x + O[1].y), kH * (O[1].y - O[1].x));      // (1 - i) / sqrt 2
                        const cx<T> t2 = mk<T>(O[2].y, -O[2].x);                                     // -i
                        const cx<T> t3 = mk<T>(kH * (O[3].y - O[3].x), -kH * (O[3].x + O[3].y));     // (-1 - i) / sqrt 2
                        v[8 * uu + 0] = cadd(E[0], t0); v[8 * uu + 4] = csub(E[0], t0);
                        v[8 * uu + 1] = cadd(E[1], t1); v[8 * uu + 5] = csub(E[1], t1);
                        v[8 * uu + 2] = cadd(E[2], t2); v[8 * uu + 6] = csub(E[2], t2);
                        v[8 * uu + 3] = cadd(E[3], t3); v[8 * uu + 7] = csub(E[3], t3);
                    } else {
                        const cx<T> u0 = ex(0, uu);
                        const cx<T> u1 = cmul(ex(1, uu), tw_of(1, uu));
                        v[2 * uu] = cadd(u0, u1);
                        v[2 * uu + 1] = csub(u0, u1);
                    }
                }
            }
            {
                const int ln = opaque(lane);
                uint4 L;                                                                               // labels of my sixteen bins, stream a
                if constexpr (kAhead) L = lab_ahead;
                else L = *reinterpret_cast<const uint4*>(s_lab + ln * kLabStride + 16 * j);
                const uint32_t wds[4] = {L.x, L.y, L.z, L.w};
                // default form: Y_r = sum_a H[r][a] X_a + noise spectrum -- byte q + NW uu of L is stream a's label at the bin of register
                // q + NW uu, lane (a, g) supplies H[h mod 4][a] and its symbol, lane (r, g) the noise and takes Y_r
                if constexpr (!TD && !(ABL & 256)) {
                    cx<T> hA;                                                      // H[h mod 4][a]
                    if constexpr (kAhead) hA = hA_ahead;
                    else hA = s_H[(ln & 3) * NT + (ln >> 4)];
                    const T hre = hA.x, him = hA.y, nhim = -hA.y;
                    // by groups of four (round 15): four look-ups into four registers, then the sixteen products, first products first
                    // -- the table reads stay ahead of the products that take them instead of one read, one wait, four products
                    // (round 17: the look-ups of group i + 1 ahead of the products of group i cost a second set of sixteen registers here,
                    // where the kernel's pressure peaks -- four spilled at the 168 bound: not in the build)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        cx<T> X[4];
#pragma unroll
                        for (int jj = 0; jj < 4; ++jj) {
                            const uint32_t lb = (wds[i] >> (8 * jj)) & 0xFFu;
                            if constexpr (ABL & 32) X[jj] = mk<T>((T)lb, 1.0);
                            else X[jj] = s_txtab[lb];
                        }
                        T yr[4], yi[4];
#pragma unroll
                        for (int jj = 0; jj < 4; ++jj) {
                            yr[jj] = __builtin_amdgcn_mfma_f64_4x4x4f64(hre, X[jj].x, v[4 * i + jj].x, 0, 0, 0);
                            yi[jj] = __builtin_amdgcn_mfma_f64_4x4x4f64(him, X[jj].x, v[4 * i + jj].y, 0, 0, 0);
                        }
#pragma unroll
                        for (int jj = 0; jj < 4; ++jj) {
                            yr[jj] = __builtin_amdgcn_mfma_f64_4x4x4f64(nhim, X[jj].y, yr[jj], 0, 0, 0);
                            yi[jj] = __builtin_amdgcn_mfma_f64_4x4x4f64(hre, X[jj].y, yi[jj], 0, 0, 0);
                            v[4 * i + jj] = mk<T>(yr[jj], yi[jj]);
                        }
                    }
                }
                if constexpr (!(ABL & 1024)) {
                cx<T> gA;                                                          // G[h mod 4][r]
                if constexpr (kAhead) gA = gA_ahead;
                else gA = s_G[(ln & 3) * NR + (ln >> 4)];
                const T gre = gA.x, gim = gA.y, ngim = -gA.y;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    cx<T> e[4];
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        const int u = 4 * i + jj;
                        T xr = __builtin_amdgcn_mfma_f64_4x4x4f64(gre, v[u].x, 0.0, 0, 0, 0);
                        T xi = __builtin_amdgcn_mfma_f64_4x4x4f64(gim, v[u].x, 0.0, 0, 0, 0);
                        xr = __builtin_amdgcn_mfma_f64_4x4x4f64(ngim, v[u].y, xr, 0, 0, 0);
                        xi = __builtin_amdgcn_mfma_f64_4x4x4f64(gre, v[u].y, xi, 0, 0, 0);
                        e[jj] = mk<T>(xr, xi);
                    }
                    if constexpr (DEC == WDEC_SLICER || DEC == WDEC_QAM_CERT) {
                        // the level-domain count takes the four sent labels as the word they already are (S0a masked every byte):
                        // no byte is extracted for the decisions
                        walk_qam_count4<DEC == WDEC_QAM_CERT>(mp, s_table, e, wds[i], se, be);
                    } else {
                        int tx[4];
#pragma unroll
                        for (int jj = 0; jj < 4; ++jj) tx[jj] = (int)((wds[i] >> (8 * jj)) & 0xFFu);
                        walk_decide<DEC, 4>(mp, s_table, nullptr, e, tx, se, be);
                    }
                }
                } else {
                    T keep = er[0][0] + ei[NW - 1][UU - 1];
                    if constexpr (!TD) {
#pragma unroll
                        for (int u = 0; u < 16; ++u) keep += v[u].x + v[u].y;
                    }
                    se += (unsigned)(keep == 0.5) + (wds[0] == 0x12345u);
                }
            }
        }
        // Round 22 (default form by lane row): the two totals by six v_add_u32 with DPP modifiers and one v_readlane_b32 each
        // (walk_wave_total) -- wave_sum_u32 is twelve ds_bpermute_b32 in six dependent steps, each waited on in full, in all NW
        // wavefronts at once right in front of B5.  32-bit unsigned sums either way: the same words, wrap-around included.
        if constexpr (kAhead) {
            se = walk_wave_total(se);
            be = walk_wave_total(be);
        } else {
            se = wave_sum_u32(se);
            be = wave_sum_u32(be);
        }
        if (lane == 0) {
            s_part[buf * 32 + 2 * j] = se;
            s_part[buf * 32 + 2 * j + 1] = be;
        }
        rl_prev = rl;
    }
    __syncthreads();
    if (tid == 0) {
        if (it > 0) {
            const int buf = (int)((it - 1) & 1);
            const unsigned* qq = s_part + buf * 32;
            unsigned ts = 0, tb = 0;
#pragma unroll
            for (int i = 0; i < NW; ++i) {
                ts += qq[2 * i];
                tb += qq[2 * i + 1];
            }
            // (kAhead: the index of the last realization from the pass count -- rl_prev is then not carried through the loop)
            if constexpr (kAhead) rl_prev = blockIdx.x + (uint64_t)(it - 1) * step;
            wg_account(totals, ts, tb, s_rec[buf * (kRec + 1) + 2 * NT * NR].x != 0.0, rl_prev, sym_out, bit_out);
        }
        wg_flush(totals, counters, (unsigned long long)per_sym * pp.n_ofdm_sym, (unsigned long long)per_sym * pp.n_ofdm_sym * mp.bits);
    }
}

template <int NW, int WPS, bool TD, int ABL, bool ROWS, bool XCH>
static int launch_mimo_ofdm_pw(mcle_ctx* ctx, const C4Plan& plan, const mcle_mimo_ofdm_cfg* cfg, uint64_t seed, uint64_t first,
                               uint64_t count, mcle_counters* d_counters, uint32_t* d_sym, uint32_t* d_bit) {
    using T = double;
    constexpr int N = 256 * NW, NT = 4, NR = 4;
    int rc;
    void* tw = nullptr;
    if ((rc = ctx->get_twiddles(N, MCLE_F64, &tw))) return rc;
    MimoParams pp{cfg->cp_size, cfg->num_used, cfg->n_ofdm_sym, cfg->mmse, cfg->noise_var};
    ModemParams<T> mp = pipe_modem<T>(ctx, cfg->demod_method);
    const int dec = walk_dec_kind(ctx, mp);          // (the plan's form; here for the on-axis constants it leaves in mp)
    mp.grid.G = 0;
    const size_t tab_len = ((size_t)mp.M + 1) & ~(size_t)1;
    const size_t dyn = (size_t)NW * kPwPlane * sizeof(T) + 2 * tab_len * sizeof(cx<T>);      // planes + the two constellation tables
    const size_t lds = dyn + pw_static_lds<NW>();                                             // + the kernel's static arrays
    MCLE_REQUIRE(lds + 512 <= (size_t)160 * 1024, "part-wave MIMO-OFDM kernel: %zu B of LDS do not fit", lds);
    auto kern = k_run_mimo_ofdm_pw<NW, WDEC_SLICER, WPS, TD, ABL, ROWS, XCH>;
    switch (dec) {
        case WDEC_QAM_CERT: kern = k_run_mimo_ofdm_pw<NW, WDEC_QAM_CERT, WPS, TD, ABL, ROWS, XCH>; break;
        case WDEC_QUAD_CERT: kern = k_run_mimo_ofdm_pw<NW, WDEC_QUAD_CERT, WPS, TD, ABL, ROWS, XCH>; break;
        case WDEC_AXIS4_CERT: kern = k_run_mimo_ofdm_pw<NW, WDEC_AXIS4_CERT, WPS, TD, ABL, ROWS, XCH>; break;
        default: break;
    }
    MCLE_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
    int per_cu = (int)((size_t)160 * 1024 / (lds + 512));
    if (per_cu < 1) per_cu = 1;
    const int by_waves = WPS * 4 / NW;                         // wavefronts per SIMD x four SIMDs / wavefronts per workgroup
    if (per_cu > by_waves) per_cu = by_waves;
    const uint64_t resident = (uint64_t)ctx->n_cu * per_cu;
    static_assert(XCH ? ROWS && ABL == 0 : true, "the exchange in complex halves: default form by lane row only");
    set_c4_kernel(ctx, plan);
    const uint64_t kSlice = 1ull << 20;          // realizations per record kernel + link kernel pair (553 MB of records; 2^18: three more tails per bench step, -0.6 %)
    return launch_sliced_planar<T, N, NT, NR>(ctx, pp, seed, first, count, kSlice, d_sym, d_bit,
                                              [&](void* recs, uint64_t at, uint64_t n, uint32_t* sym, uint32_t* bit) {
        // (workgroups per resident slot: up to 32 at 1024 points -- 31.36 against 31.53 ms per 2^20 realizations at 16, 31.40 at 48)
        const unsigned grid = (unsigned)oversubscribed_grid(ctx, resident, n, 8, NW == 4 ? 32 : 16);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * NW), dyn, ctx->stream, pp, mp, seed, at, n, (const cx<T>*)tw, (const cx<T>*)recs,
                           d_counters, sym, bit);
    });
}

// The part-wave instantiations <NW, wavefronts per SIMD, time-domain form, ablation, ownership by lane row, exchange in complex
// halves>; which of them serves a call: c4_select.hpp.  Per size: the map of rounds 6 - 9 (a wavefront owns a time class: noise words
// through LDS, barrier B1), ownership by lane row with the exchange in complex halves and with the exchange by re / im planes
// (barrier B3: the witness of round 20 -- DESIGN.md 5.28), the time-domain form; at 512 / 1024 points the default form's exchange
// bounded for two wavefronts per SIMD as well.
int launch_mimo_ofdm_pw(mcle_ctx* ctx, const C4Plan& p, const mcle_mimo_ofdm_cfg* cfg, uint64_t seed, uint64_t first, uint64_t count,
                        mcle_counters* d_counters, uint32_t* d_sym, uint32_t* d_bit) {
#define MCLE_PW(NW_, WPS_, TD_, ABL_, ROWS_, XCH_)                                                                              \
    if (p.n == 256 * NW_ && p.wps == WPS_ && p.td == TD_ && p.abl == ABL_ && p.rows == ROWS_ && p.halves == XCH_)               \
        return launch_mimo_ofdm_pw<NW_, WPS_, TD_, ABL_, ROWS_, XCH_>(ctx, p, cfg, seed, first, count, d_counters, d_sym, d_bit);
#define MCLE_PW_SIZE(NW_, WPS_)                                                                                                 \
    MCLE_PW(NW_, WPS_, false, 0, false, false) MCLE_PW(NW_, WPS_, false, 0, true, true) MCLE_PW(NW_, WPS_, false, 0, true, false) \
    MCLE_PW(NW_, WPS_, true, 0, false, false)
    MCLE_PW_SIZE(2, 3) MCLE_PW(2, 2, false, 0, true, false)
    MCLE_PW_SIZE(4, 3) MCLE_PW(4, 2, false, 0, true, true)
    MCLE_PW_SIZE(8, 2)
#ifdef MCLE_EXPERIMENTS     // section ablations of the time-domain form and of the default form with the exchange by planes
#define MCLE_PW_ABL(V_)                                                                                                         \
    MCLE_PW(2, 3, true, V_, false, false) MCLE_PW(2, 3, false, V_, true, false) MCLE_PW(4, 3, true, V_, false, false)           \
    MCLE_PW(4, 3, false, V_, true, false)
    MCLE_PW_ABL(32) MCLE_PW_ABL(64) MCLE_PW_ABL(128) MCLE_PW_ABL(256) MCLE_PW_ABL(512) MCLE_PW_ABL(1024) MCLE_PW_ABL(2016)
#undef MCLE_PW_ABL
#endif
#undef MCLE_PW_SIZE
#undef MCLE_PW
    MCLE_REQUIRE(false, "internal: no part-wave MIMO-OFDM kernel <%d> w%d time %d rows %d halves %d ablation %d", p.n / 256, p.wps, (int)p.td,
                 (int)p.rows, (int)p.halves, p.abl);
}

}  // namespace mcle
