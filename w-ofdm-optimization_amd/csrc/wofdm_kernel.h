// Host <-> kernel contract of the frame kernel (internal to libwofdm_hip.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define WOFDM_LT 21   // taps the FIR is unrolled for (channels are zero-padded to it)

struct wofdm_kdump {          // device pointers, all may be null
    uint8_t *labels_tx;
    float2  *X, *tx, *conv, *rx, *Y, *Xhat;
    uint8_t *labels_rx;
    float   *gain;
    float2  *unit_noise;
    float2  *sink;            // where the per-lane stage dumps of lanes without a sample go: the
                              // instrumented kernels store unconditionally instead of branching
};

// LDS carve: fixed-size regions first (compile-time offsets), the frame buffer last.
//   tw    float2[N]          twiddles exp(-2 pi i m / N)    (N = 256, 512: 6 KB -- the matrix-pipe layouts 10 / 11 / 12 keep
//                            six of the ten operand rows of the transforms there, [6][64] 16-byte rows)
//   g     float2[N]          pilot equaliser X0/Y0
//   sums  float [2][32]      per-wave signal / noise power partials, double-buffered by frame parity
//   flags int   [64]         [w] = last loop iteration whose phase A wave w has finished,
//                            [16] = last iteration whose pilot equaliser G is published, [20] = a wave gave up waiting,
//                            [17 .. 19], [21 .. 23], [28 .. 31] = the hand-out of the launch's items (WS_* in wofdm_kernel.hip),
//                            [32 + w] = (Tx-mask variants) last iteration whose masked symbol wave w has written to its row,
//                            [48 + w] = (Tx-mask variants on the matrix pipe, layouts 9 / 15) last iteration whose row wave w has
//                            turned into its two f16 planes (the successor's first tile reads the row's last samples)
//   wtx   float [N + CPCS]   Tx window / N      (needs cp + cs <= CPCS_MAX = 128; 64 at N = 1024,
//                            where the frame buffer leaves no room for more anyway)
//   wrx   float [N + 64]     Rx window          (needs tail_rx <= 64)
//   lut   float2[64]         QAM constellation by label
//   fbuf  float2[fbuf_len]   WOFDM_LT-1 zeros | frame (T) | zeros
//   tail  float2[S][tail_tx] fall tails, behind the frame buffer (then the Tx-mask tables, if any)
// (NOTW: layouts 13 / 14 / 16 -- N = 64, 128 with the transforms on the matrix pipe -- keep no twiddle table: their operand rows come
// from L2.  Those 512 bytes decide at N = 64 whether a workgroup takes twelve or thirteen of the LDS's 128 allocation units --
// ten or nine workgroups per CU: wofdm_lds_workgroups_per_cu)
template <int N, bool NOTW = false> struct wofdm_lds {
    static constexpr int TAIL_MAX = 16, CPCS_MAX = N >= 1024 ? 64 : 128, TAILRX_MAX = 64;
    static constexpr int off_tw = 0;
    static constexpr int TW_BYTES = NOTW ? 0 : (N == 256 || N == 512 ? 6 * 64 * 16 : 8 * N);
    static constexpr int off_g = off_tw + TW_BYTES;
    static constexpr int off_sums = off_g + 8 * N;
    static constexpr int off_flags = off_sums + 4 * 64;
    static constexpr int off_wtx = off_flags + 4 * 64;
    static constexpr int off_wrx = off_wtx + 4 * (N + CPCS_MAX);
    static constexpr int off_lut = off_wrx + 4 * (N + TAILRX_MAX);
    static constexpr int off_fbuf = off_lut + 8 * 64;
};

// geometry array read by the kernel through a laundered pointer (see GEO_PHASE)
enum { WOFDM_G_S, WOFDM_G_MU, WOFDM_G_RHO, WOFDM_G_BETA, WOFDM_G_DELTA, WOFDM_G_GAMMA, WOFDM_G_KAPPA,
       WOFDM_G_L, WOFDM_G_P, WOFDM_G_B, WOFDM_G_T, WOFDM_G_NL, WOFDM_G_NSNR, WOFDM_G_NCH, WOFDM_G_FBUF,
       WOFDM_G_NACT,      // loaded subcarriers (WOFDM_VAR_ALLOC)
       WOFDM_G_SPWR,      // layout 16: symbols a wave takes (wofdm_small_spwr; the other layouts hold theirs at compile time)
       WOFDM_G_COUNT };

struct wofdm_kparams {
    uint32_t n_cells;       // cells covered by this launch, starting at first_cell
    uint32_t first_cell;
    uint32_t inject_base_cell;   // injected arrays AND the counter array are indexed from this cell
    unsigned lds_bytes;
    uint64_t frames_per_cell, frame_offset;
    // (cell, frame) items of the launch, cell-major (wofdm_work_split): workgroup b starts with a run of head_q items, one more
    // for the first head_r workgroups; the items [tail0, total) go out in chunks of `chunk` through the work counter
    uint64_t head_q, head_r, tail0, total;
    uint32_t chunk;               // 0: no tail
    unsigned long long *work;     // the plan's work counter: items of the tail handed out so far (zero at the launch)
    uint32_t seed_lo, seed_hi;
    unsigned long long *counts;   // [cells][4], entry 0 = cell inject_base_cell
    // layouts 10 / 11 / 12 (both transforms on the matrix pipe): operand table [10 + 2 (N/256 - 1)][64] x 16 bytes
    // (wofdm_abi.hip) and the power of two per (snr, channel) that centres the received samples in the f16 range
    const uint4 *dftc;
    const float *rx_scale;
    const uint8_t *labels;  // inject: [cells][frames][S][N]
    const float2  *unit_noise;    // inject: [cells][frames][NL]
    float2 *noise_scratch;        // generate, N >= WOFDM_NOISE_SCRATCH_MIN_N: [grid][16][RB][64]
    unsigned *status;             // device word, bit 0 set if a wave gave up waiting on a flag
    // Scaling of the on-air signal inside the kernel.  The Tx window table holds w_tx * tx_scale
    // (1/N of the IDFT, and in the matrix-pipe FIR layouts a power of two that centres the samples
    // in the f16 range); the channel's Toeplitz operands carry their own power of two.  Everything
    // behind the FIR is homogeneous in that scale (the noise gain is derived from the measured
    // powers, the equaliser divides by the pilot), so only the stage dumps undo it.
    float tx_scale, dump_unscale_tx, dump_unscale_rx;
    wofdm_kdump dump;
#ifdef WOFDM_DELAY
    // developer build (tools/delay_probe.py): the waves of delay_waves sleep delay_len x 4 us at point delay_point
    uint32_t delay_point, delay_waves, delay_len;
#endif
#ifdef WOFDM_AUDIT
    // developer build (tools/audit_suite.py): per (workgroup, frame, wave) record of 8 words -- bit errors,
    // symbol errors, noise gain, Ps, Pn, HW_ID, XCC_ID, clock -- for the first audit_items frames of a workgroup
    uint32_t *audit;
    uint32_t audit_items;
#endif
};

// How a launch's (cell, frame) items are shared out among its workgroups (wofdm_work_split).
//   equal split:  workgroup b runs head_q consecutive items, one more if b < head_r (total / grid and total % grid): all there is
//                 to a launch that is not `dynamic`, or has no more items than workgroups;
//   dynamic:      a static head of head_q = alpha_256 / 256 of total / grid items per workgroup, and behind the heads a tail,
//                 [tail0, total), that the workgroups take in chunks of `chunk` items, first come first served
//                 (wofdm_frames_kernel: take_chunk).
// launch() makes a launch dynamic where that pays: more than one workgroup per CU -- those do not run at one rate, DESIGN.md
// section 4; one workgroup per CU has nothing to even out and N = 512 lost 5 % to the chunks' barriers -- and at least
// WOFDM_SPLIT_MIN_ITEMS items per workgroup: a grab costs a workgroup about as much as a fifth of a frame, and a tail of a few
// chunks evens out nothing (launches of 80 ... 125 items per workgroup lost 3 ... 8 %, those of 977 and 1 953 gained 7 % and
// 5 %; nothing in between has been measured: profiles/work_split.txt).
// The instantiations that hold the hand-out's code, and so can be given a tail: the layouts of the plain and allocation variants
// that run with several workgroups per CU (10, 11: N = 256; 13, 14, 16: N = 64, 128), and layout 12 at N = 512 (one workgroup per
// CU: a tail only under the developer override).  Every other kernel is compiled as it was with equal shares.
static constexpr bool wofdm_layout_dynamic(int layout, int n_fft)
{
    return layout == 10 || layout == 11 || layout == 13 || layout == 14 || layout == 16 || (layout == 12 && n_fft == 512);
}
#define WOFDM_SPLIT_ALPHA_256 192     // 3/4 static; the chunked quarter absorbs the spread of the workgroups' rates
#define WOFDM_SPLIT_CHUNK 8           // (both: interleaved A/Bs at C2, profiles/work_split.txt)
#define WOFDM_SPLIT_MIN_ITEMS 512
struct wofdm_split { uint64_t head_q, head_r, tail0; uint32_t chunk; };    // chunk 0: no tail
static inline wofdm_split wofdm_work_split(uint64_t total, uint64_t grid, bool dynamic, uint32_t alpha_256, uint32_t chunk)
{
    const uint64_t q = total / grid;
    if (!dynamic || total <= grid) return {q, total % grid, total, 0u};
    // (q * alpha in two parts: q may take all 64 bits' worth of frames_per_cell * cells / grid)
    const uint64_t head = (q >> 8) * alpha_256 + (((q & 255u) * alpha_256) >> 8);
    return {head, 0u, head * grid, chunk};
}

// DFT lengths from which the generated unit noise is parked in HBM scratch between the FIR and
// the noise-scaling phase instead of registers
#ifndef WOFDM_NOISE_SCRATCH_MIN_N
#define WOFDM_NOISE_SCRATCH_MIN_N 1024
#endif
// largest cp + cs the Tx window table of the kernel holds (wofdm_lds<N>::CPCS_MAX)
static inline int wofdm_cpcs_max(int n_fft) { return n_fft >= 1024 ? 64 : 128; }
static inline int wofdm_kslot(int k) { return k == 6 ? 8 : k; }
static constexpr int wofdm_fir8_tiles(int n_fft) { return n_fft >= 1024 ? 9 : (n_fft >= 512 ? 5 : 3); }

// ---- Layouts of the frame kernel ----
// The template parameter LAY of wofdm_frames_kernel, also the plan's kernel id (wofdm_plan_kernel_id).  Everything that depends
// on it is read from wofdm_layout_info: the host's sizing here, the kernel's prologue, its __launch_bounds__ and the set of
// instantiations (wofdm_layout_built).  Which layout a geometry gets is wofdm_pick_layout / wofdm_pick_layout_masked.
//    1, 2   one / two symbols per wave, FIR and transforms on the VALU
//    4, 5   four symbols per wave (quarter-wave layout, N = 256), VALU; 5 has 20 FIR outputs per lane instead of 18 (B <= 320)
//    6, 7   4 / 5 with the FIR on the matrix pipe (9 / 10 tiles of 128 samples per wave, two samples per lane and tile)
//    8      one symbol per wave with the FIR on the matrix pipe (N >= 512; wofdm_fir8_tiles tiles per wave)
//    9      8's frame format for the Tx-mask variants (any N <= 512): the mask stage works on the rows as fp32, phase B turns them
//           into the f16 planes in place
//    10, 11 6 / 7 with both 256-point transforms on the matrix pipe as well (lane l holds elements l + 64 j of each of the wave's
//           four symbols)
//    12     8 with both transforms on the matrix pipe as well (N = 512, 1024: 16 . 16 . N/256, the last stage in registers)
//    13, 14 N = 64, 128 with the FIR and both transforms on the matrix pipe: 16 / 8 symbols per wave (one MFMA stage over the
//           stride-N/16 index, the radix-N/16 stage in registers), 10 / 11 FIR tiles per wave
//    15     9 at N = 256 for the fast-convolution Tx mask with every transform on the matrix pipe: the symbol's own two as in
//           layout 12 (one set), the mask's two 1024-point ones as four sets each with no exchange in between (no mask scratch
//           in LDS)
//    16     13 with a RUN-TIME number of symbols per wave (even, <= 1024 / N, wofdm_small_spwr) and a partly filled last wave:
//           the N = 64, 128 geometries layouts 13 / 14 do not take -- S not a multiple of 16 / 8, strides beyond their tiles
//           (N = 64 at CP 32: two waves of eight symbols) -- which ran layout 2 before (round 4)
enum { WOFDM_FIR_VALU, WOFDM_FIR_QUARTER, WOFDM_FIR_ONE };          // VALU / matrix pipe, a wave's symbols as one row / one symbol per wave
enum { WOFDM_DFT_VALU, WOFDM_DFT_MDFT, WOFDM_DFT_BIG, WOFDM_DFT_SMALL };  // VALU / matrix pipe: 256-point (mdft_fwd), mdft_big, one stage
struct wofdm_layout {
    int spw;            // symbol slots per wave, fixed at compile time (layout 16: the most; its run-time count is wofdm_spwr); 0: no layout
    int fir, dft;       // WOFDM_FIR_*, WOFDM_DFT_*
    bool partial;       // run-time number of symbols per wave (gm[WOFDM_G_SPWR])
    bool masked;        // built for the Tx-mask variants only
    int nt;             // FIR tiles of 128 samples per wave (matrix-pipe FIR)
    int rb;             // FIR outputs per lane (fir_geo)
    int wg, min_waves;  // __launch_bounds__: workgroup size, waves per SIMD (4: one 16-wave workgroup per CU -> 128 VGPRs per lane)
    int n_min, n_max;   // DFT lengths it is built for
    unsigned vars;      // variants it is built for (bit WOFDM_VAR_*; wofdm_layout_built)
};
#define WOFDM_LAYOUT_COUNT 17   // ids 0 .. 16
static constexpr wofdm_layout wofdm_layout_info(int id, int n_fft)
{
    const int f8 = wofdm_fir8_tiles(n_fft), sm = 1024 / n_fft;
    const unsigned PA = 3u, MASKS = 12u;   // plain + allocation; the two Tx-mask variants
    switch (id) {
    //               spw  fir                dft              part   mask   nt  rb                   wg     minw  N          vars
    case 1:  return {1,  WOFDM_FIR_VALU,    WOFDM_DFT_VALU,  false, false, 0,  n_fft / 64 + 1,      1024,  4,    64, 1024,  PA | MASKS};
    case 2:  return {2,  WOFDM_FIR_VALU,    WOFDM_DFT_VALU,  false, false, 0,  2 * (n_fft / 64) + 2, 512,  4,    64, 256,   PA};
    case 4:  return {4,  WOFDM_FIR_VALU,    WOFDM_DFT_VALU,  false, false, 0,  4 * (n_fft / 64) + 2, 256,  3,    256, 256,  PA};
    case 5:  return {4,  WOFDM_FIR_VALU,    WOFDM_DFT_VALU,  false, false, 0,  20,                  256,   3,    256, 256,  PA};
    case 6:  return {4,  WOFDM_FIR_QUARTER, WOFDM_DFT_VALU,  false, false, 9,  18,                  256,   3,    256, 256,  PA};
    case 7:  return {4,  WOFDM_FIR_QUARTER, WOFDM_DFT_VALU,  false, false, 10, 20,                  256,   3,    256, 256,  PA};
    case 8:  return {1,  WOFDM_FIR_ONE,     WOFDM_DFT_VALU,  false, false, f8, 2 * f8,              1024,  4,    512, 1024, PA};
    case 9:  return {1,  WOFDM_FIR_ONE,     WOFDM_DFT_VALU,  false, true,  f8, 2 * f8,              1024,  4,    64, 1024,  MASKS};
    case 10: return {4,  WOFDM_FIR_QUARTER, WOFDM_DFT_MDFT,  false, false, 9,  18,                  256,   3,    256, 256,  PA};
    case 11: return {4,  WOFDM_FIR_QUARTER, WOFDM_DFT_MDFT,  false, false, 10, 20,                  256,   3,    256, 256,  PA};
    case 12: return {1,  WOFDM_FIR_ONE,     WOFDM_DFT_BIG,   false, false, f8, 2 * f8,              1024,  4,    512, 1024, PA};
    case 13: return {sm, WOFDM_FIR_QUARTER, WOFDM_DFT_SMALL, false, false, 10, 20,                  n_fft, 3,    64, 128,   PA};
    case 14: return {sm, WOFDM_FIR_QUARTER, WOFDM_DFT_SMALL, false, false, 11, 22,                  n_fft, 3,    64, 128,   PA};
    case 15: return {1,  WOFDM_FIR_ONE,     WOFDM_DFT_BIG,   false, true,  f8, 2 * f8,              1024,  4,    256, 256,  8u};
    case 16: return {sm, WOFDM_FIR_QUARTER, WOFDM_DFT_SMALL, true,  false, 10, 20,                  256,   3,    64, 128,   PA};
    }
    return {};
}
#define WOFDM_FIR8_VT 48      // words per plane of layout 8's virtual row behind the last symbol
#define WOFDM_FIRM_PRE 24     // zero samples in front of the frame in the f16 planes (taps - 1 <= 24, 16-byte rows)
static constexpr int wofdm_rb(int n_fft, int layout = 1) { return wofdm_layout_info(layout, n_fft).rb; }
// Layout 16: the symbols a wave takes -- the frame spread evenly over the fewest waves (at most four) whose share, rounded up to
// an even count (a wave's rows are split between the two f16 planes), fits the 1024 / N symbol slots and the ten tiles of a
// wave; 0: none fits.  The last wave takes what is left (S - (W - 1) spwr symbols, any count >= 1).
static constexpr int wofdm_small_spwr(int n_fft, int S, int B)
{
    const int slots = 1024 / n_fft;
    for (int W = 1; W <= 4; ++W) {
        const int spwr = ((S + W - 1) / W + 1) & ~1;
        if (spwr <= slots && spwr * B <= 128 * 10 && (W - 1) * spwr < S) return spwr;
    }
    return 0;
}
// symbols per wave as the kernel of `layout` runs this geometry, and the waves of its workgroup
static constexpr int wofdm_spwr(int layout, int n_fft, int S, int B)
{
    const wofdm_layout li = wofdm_layout_info(layout, n_fft);
    return li.partial ? wofdm_small_spwr(n_fft, S, B) : li.spw;
}
static constexpr int wofdm_waves(int layout, int n_fft, int S, int B)
{
    const int r = wofdm_spwr(layout, n_fft, S, B);
    return r > 0 ? (S + r - 1) / r : 0;
}
// Layout of the plain and allocation variants: four symbols per wave at N = 256 (quarter-wave layouts, S a multiple of 4,
// four symbols within the FIR outputs of a wave), the matrix-pipe layouts 13 / 14 / 16 at N = 64, 128 and 12 / 8 at N >= 512
// where they fit, else two symbols per wave where the register budget allows it (N <= 256) and S is even, else one.
static constexpr int wofdm_pick_layout(int n_fft, int S, int B, bool plain = false, bool firm = true, bool mdft = true)
{
    // (the matrix-pipe kernels take a stride of at least n_fft for granted: their tiles below SPW n_fft
    // samples carry no validity tests)
    firm = firm && B >= n_fft;
    if (plain && mdft && firm && n_fft <= 128 && S % (1024 / n_fft) == 0) {
        if ((1024 / n_fft) * B <= 128 * wofdm_layout_info(13, n_fft).nt) return 13;
        if ((1024 / n_fft) * B <= 128 * wofdm_layout_info(14, n_fft).nt) return 14;
    }
    if (plain && mdft && firm && n_fft <= 128 && wofdm_small_spwr(n_fft, S, B) > 0) return 16;
    if (plain && n_fft == 256 && S % 4 == 0) {
        if (firm && 4 * B <= 128 * wofdm_layout_info(6, n_fft).nt) return mdft ? 10 : 6;
        if (firm && 4 * B <= 128 * wofdm_layout_info(7, n_fft).nt) return mdft ? 11 : 7;
        if (4 * B <= 64 * wofdm_rb(n_fft, 4)) return 4;
        if (4 * B <= 64 * wofdm_rb(n_fft, 5)) return 5;       // 288 < B <= 320: 20 outputs per lane
    }
    // one symbol per wave, matrix-pipe FIR: every stride (a 16-byte operand row that straddles the end of a symbol is cut word by
    // word, fir_load; with an odd stride the rows of the odd symbols start on an odd sample of the frame: their noise pairs take
    // two Philox blocks, their last pair holds one sample -- round 4; the LDS takes 16-byte accesses at any 4-byte alignment)
    if (firm && plain && n_fft >= 512 && (B % 2 == 0 || mdft) && B <= 128 * wofdm_fir8_tiles(n_fft)) return mdft ? 12 : 8;
    return (n_fft <= 256 && S % 2 == 0 && 2 * B <= 64 * wofdm_rb(n_fft, 2)) ? 2 : 1;
}

// layout of the Tx-mask variants: 9 where the matrix-pipe FIR fits (B >= n_fft, B within its tiles; every stride since round 4 --
// the rows of these layouts keep the stride itself as their pitch, so odd strides put planes on 4- and 8-byte boundaries, which
// the LDS takes at a price: CPW N = 256 masked 2.63e8 symbols/s against 2.85e8 at an even stride, 1.99e8 in layout 1), else 1
static inline int wofdm_pick_layout_masked(int n_fft, int B, bool firm)
{
    return (firm && B >= n_fft && B <= 128 * wofdm_fir8_tiles(n_fft)) ? 9 : 1;
}

// float2 elements of noise scratch per workgroup (0: not used for this DFT length)
static inline size_t wofdm_noise_scratch_len(int n_fft, int layout)
{
    return n_fft >= WOFDM_NOISE_SCRATCH_MIN_N ? (size_t)16 * 64 * wofdm_rb(n_fft, layout) : 0;
}

// float2 elements of the frame buffer.  Matrix-pipe layouts: the same bytes hold two planes of
// packed-f16 words (hi and lo halves of every sample), each `len` words long: 24 zeros, the frame,
// and zeros up to the end of the tile that covers the trailing samples behind the last wave.
static constexpr int wofdm_fbuf_len(int N, int T, int layout, int S = 0, int B = 0)
{
    const wofdm_layout li = wofdm_layout_info(layout, N);
    // (behind the last wave's first sample: its tiles and one more of zeros; layout 16: the last wave starts at (W - 1) spwr B)
    if (li.dft == WOFDM_DFT_SMALL)
        return (WOFDM_FIRM_PRE + (wofdm_waves(layout, N, S, B) - 1) * wofdm_spwr(layout, N, S, B) * B + 128 * (li.nt + 1) + 3) / 4 * 4;
    if (li.fir == WOFDM_FIR_ONE) {
        // words per plane between the LDS rows of two symbols: the stride itself in the Tx-mask layouts (9, 15: the row holds the
        // masked symbol as fp32 first), rounded up to whole 16-byte operand rows in layouts 8 / 12 -- every row and both of its
        // planes then start on 16 bytes whatever the stride (round 4: strides of 2 mod 4 ran on 8-byte-aligned planes before, odd
        // ones not at all)
        const int row_stride = li.masked ? B : (B + 3) & ~3;
        return (8 + 2 * S * row_stride + 2 * WOFDM_FIR8_VT) / 2;
    }
    if (li.fir == WOFDM_FIR_QUARTER)
        return (WOFDM_FIRM_PRE + (S - 4) * B + 128 * (li.nt + 1) + 3) / 4 * 4;
    return ((WOFDM_LT - 1) + T + (WOFDM_LT - 1) + li.rb + 8 + 1) / 2 * 2;
}
// The LDS of a CU is handed out in units of 1 280 bytes (160 KiB / 128) on this GPU -- measured, round 4: with 15 808 bytes per
// one-wave workgroup (thirteen units) a CU holds NINE workgroups, not the ten the occupancy API reports (158 080 bytes do fit
// 160 KiB), and a grid of ten per CU ran as two rounds -- nine, then one -- at the rate of five (profiles/r04_occ_small.txt);
// every other kernel's residency agrees with the same unit (three workgroups of 52 640 bytes = 3 x 42 units do fit).  The plan's
// grid counts workgroups by it.
#define WOFDM_LDS_GRANULE 1280
static inline int wofdm_lds_workgroups_per_cu(unsigned lds_bytes)
{
    const unsigned units = (lds_bytes + WOFDM_LDS_GRANULE - 1) / WOFDM_LDS_GRANULE;
    return units ? (int)(160u * 1024u / WOFDM_LDS_GRANULE / units) : 32;
}
static inline unsigned wofdm_lds_bytes(int N, int T, int layout, int S, int B)
{
    const int fixed = (wofdm_layout_info(layout, N).dft == WOFDM_DFT_SMALL ? 0 : (N == 256 || N == 512 ? 6 * 64 * 16 : 8 * N)) + 8 * N + 4 * 64 + 4 * 64 + 4 * (N + wofdm_cpcs_max(N)) + 4 * (N + 64) + 8 * 64;
    const int beta = T - S * B;
    // (layout 15, behind the fall tails: 16 bytes of alignment, a row of 344 samples per wave for the mask stage's spill, and 64 spare
    // bytes at the very end -- the target of the mask stage's stores that have no output)
    return (unsigned)(fixed + 8 * wofdm_fbuf_len(N, T, layout, S, B) + 8 * S * beta + (layout == 15 ? 16 + S * 344 * 8 + 64 : 0));
}

// ---- Built geometries ----
// The frame kernel reads its structure lengths from a device array, again in every phase (GEO_PHASE in wofdm_kernel.hip): they are
// run-time values to it.  For the geometries of this table the generate-mode, production, plain kernels of N = 256 are built a
// second time with the row's lengths as compile-time constants (template parameter GEO of wofdm_frames_kernel = the row's id =
// its index + 1; id 0 = geometry at run time, every other kernel).  n_snr, n_channels and everything per cell stay run-time values.
// Rows: the seven structures (variants.py: wtx, wrx, WOLA, CPW, CPwtx, CPwrx, CP) at N = 256, CP 32, the reference's tails, 16
// symbols per frame, 21 taps, noise_before_truncate = 1.  A row whose kernel fails the build's static checks, spills to scratch, takes
// more than 168 VGPRs or loses the third workgroup per CU is taken out of the table and runs generic (profiles/kernel_table_geo.json).
// (The "// <id> <name>" comment of each row is read as data: tools/kernel_table.py and the tests take the rows' structure names from it.
// Taking a row out renumbers the rows below it: renumber their comments and regenerate profiles/kernel_table_geo.json.)
struct wofdm_geo_row { int n_fft, S, mu, rho, beta, delta, gamma, kappa, L, P, B, T, NL; };
#define WOFDM_GEO_COUNT 7
static constexpr wofdm_geo_row wofdm_geo_table[WOFDM_GEO_COUNT] = {
    //N   S   mu  rho beta delta gamma kappa L   P    B    T     NL
    {256, 16, 32, 8,  8,   0,    32,   0,    21, 296, 288, 4616, 4636},   // 1 wtx
    {256, 16, 32, 5,  0,   10,   27,   0,    21, 293, 293, 4688, 4708},   // 2 wrx
    {256, 16, 32, 8,  8,   10,   22,   5,    21, 296, 288, 4616, 4636},   // 3 WOLA
    {256, 16, 32, 13, 8,   10,   27,   0,    21, 301, 293, 4696, 4716},   // 4 CPW
    {256, 16, 32, 0,  8,   0,    24,   8,    21, 288, 280, 4488, 4508},   // 5 CPwtx
    {256, 16, 32, 0,  0,   10,   22,   5,    21, 288, 288, 4608, 4628},   // 6 CPwrx
    {256, 16, 32, 0,  0,   0,    32,   0,    21, 288, 288, 4608, 4628},   // 7 CP
};
static constexpr wofdm_geo_row wofdm_geo_row_of(int id) { return id >= 1 && id <= WOFDM_GEO_COUNT ? wofdm_geo_table[id - 1] : wofdm_geo_row{}; }
// the layout a row's kernel is built as (what wofdm_pick_layout gives the geometry under the default options)
static constexpr int wofdm_geo_layout(int id)
{
    return id >= 1 && id <= WOFDM_GEO_COUNT ? wofdm_pick_layout(wofdm_geo_table[id - 1].n_fft, wofdm_geo_table[id - 1].S, wofdm_geo_table[id - 1].B, true) : 0;
}
// id of a geometry: every field equal to a row's, else 0
static constexpr int wofdm_geo_id(const wofdm_geo_row &g)
{
    for (int i = 0; i < WOFDM_GEO_COUNT; ++i) {
        const wofdm_geo_row &r = wofdm_geo_table[i];
        if (r.n_fft == g.n_fft && r.S == g.S && r.mu == g.mu && r.rho == g.rho && r.beta == g.beta && r.delta == g.delta
            && r.gamma == g.gamma && r.kappa == g.kappa && r.L == g.L && r.P == g.P && r.B == g.B && r.T == g.T && r.NL == g.NL)
            return i + 1;
    }
    return 0;
}

// kernel registry (wofdm_kernel.hip)
// constants travel as separate noalias arguments so that uniform reads become scalar loads:
// w_tx[pairs][P], w_rx[pairs][N+delta], h[n_ch][WOFDM_LT] zero padded, noise_lin[n_snr]
// fira[n_ch][4][64] (uint4): the channel's Toeplitz operands of the matrix-pipe FIR, in MFMA A layout
typedef void (*wofdm_kernel_fn)(wofdm_kparams, const float *, const float *, const float2 *,
                                const float *, const int *, const uint32_t *, const float2 *,
                                const uint4 *);
enum { WOFDM_MODE_GEN = 0, WOFDM_MODE_INJECT = 1, WOFDM_MODE_DUMP_GEN = 2, WOFDM_MODE_DUMP_INJECT = 3 };
// kernel variants: every subcarrier loaded / a subcarrier allocation mask / allocation + per-symbol
// spectral Tx mask (one symbol per wave, n_fft <= WOFDM_TXMASK_MAX_N: the mask table needs LDS)
// (direct form, g_tmask = impulse response) / the same as fast convolution (g_tmask = spectrum; n_fft
// <= WOFDM_TXFFT_MAX_N and 3P-2 <= WOFDM_TXFFT_LEN)
enum { WOFDM_VAR_PLAIN = 0, WOFDM_VAR_ALLOC = 1, WOFDM_VAR_TXMASK = 2, WOFDM_VAR_TXFFT = 3, WOFDM_VAR_COUNT };
#define WOFDM_TXMASK_MAX_N 512
#define WOFDM_TXFFT_MAX_N 256
#define WOFDM_TXFFT_LEN 1024
#define WOFDM_TXFFT_SLOTS 8
// the (layout, N, variant) combinations the library instantiates (wofdm_kernel.hip, pick_layout)
static constexpr bool wofdm_layout_built(int layout, int n_fft, int var)
{
    const wofdm_layout li = wofdm_layout_info(layout, n_fft);
    return li.spw > 0 && n_fft >= li.n_min && n_fft <= li.n_max && ((li.vars >> var) & 1u)
           && (var != WOFDM_VAR_TXMASK || n_fft <= WOFDM_TXMASK_MAX_N) && (var != WOFDM_VAR_TXFFT || n_fft <= WOFDM_TXFFT_MAX_N);
}
// LDS behind the frame buffer in the FFT form: twiddles + scratch rows
static inline unsigned wofdm_txfft_lds_bytes(void)
{
    return 8u * (unsigned)(WOFDM_TXFFT_LEN * (1 + WOFDM_TXFFT_SLOTS));
}
// bytes of LDS the (complex) Tx mask table takes behind the frame buffer (mask_geo in
// wofdm_kernel.hip)
static inline unsigned wofdm_txmask_lds_bytes(int n_fft)
{
    const int cpcs = wofdm_cpcs_max(n_fft);
    const int lmax = 2 * (n_fft + cpcs) - 1, no = (lmax + 63) / 64, mb = 4;
    return 8u * (unsigned)((n_fft + cpcs + 2 * mb) + 64 * no + mb);
}
// one translation unit per (DFT length, bits per subcarrier): wofdm_kernel.hip with
// -DWOFDM_TU_N=<N> -DWOFDM_TU_K=<k>
wofdm_kernel_fn wofdm_select_kernel_n64_k2(int layout, int mode, int var);
wofdm_kernel_fn wofdm_select_kernel_n64_k4(int layout, int mode, int var);
wofdm_kernel_fn wofdm_select_kernel_n64_k6(int layout, int mode, int var);
wofdm_kernel_fn wofdm_select_kernel_n128_k2(int layout, int mode, int var);
wofdm_kernel_fn wofdm_select_kernel_n128_k4(int layout, int mode, int var);
wofdm_kernel_fn wofdm_select_kernel_n128_k6(int layout, int mode, int var);
wofdm_kernel_fn wofdm_select_kernel_n256_k2(int layout, int mode, int var);
wofdm_kernel_fn wofdm_select_kernel_n256_k4(int layout, int mode, int var);
wofdm_kernel_fn wofdm_select_kernel_n256_k6(int layout, int mode, int var);
wofdm_kernel_fn wofdm_select_kernel_n512_k2(int layout, int mode, int var);
wofdm_kernel_fn wofdm_select_kernel_n512_k4(int layout, int mode, int var);
wofdm_kernel_fn wofdm_select_kernel_n512_k6(int layout, int mode, int var);
wofdm_kernel_fn wofdm_select_kernel_n1024_k2(int layout, int mode, int var);
wofdm_kernel_fn wofdm_select_kernel_n1024_k4(int layout, int mode, int var);
wofdm_kernel_fn wofdm_select_kernel_n1024_k6(int layout, int mode, int var);
static inline wofdm_kernel_fn wofdm_select_kernel(int n_fft, int bits_per_sc, int layout, int mode, int var)
{
    if (n_fft == 64 && bits_per_sc == 2) return wofdm_select_kernel_n64_k2(layout, mode, var);
    if (n_fft == 64 && bits_per_sc == 4) return wofdm_select_kernel_n64_k4(layout, mode, var);
    if (n_fft == 64 && bits_per_sc == 6) return wofdm_select_kernel_n64_k6(layout, mode, var);
    if (n_fft == 128 && bits_per_sc == 2) return wofdm_select_kernel_n128_k2(layout, mode, var);
    if (n_fft == 128 && bits_per_sc == 4) return wofdm_select_kernel_n128_k4(layout, mode, var);
    if (n_fft == 128 && bits_per_sc == 6) return wofdm_select_kernel_n128_k6(layout, mode, var);
    if (n_fft == 256 && bits_per_sc == 2) return wofdm_select_kernel_n256_k2(layout, mode, var);
    if (n_fft == 256 && bits_per_sc == 4) return wofdm_select_kernel_n256_k4(layout, mode, var);
    if (n_fft == 256 && bits_per_sc == 6) return wofdm_select_kernel_n256_k6(layout, mode, var);
    if (n_fft == 512 && bits_per_sc == 2) return wofdm_select_kernel_n512_k2(layout, mode, var);
    if (n_fft == 512 && bits_per_sc == 4) return wofdm_select_kernel_n512_k4(layout, mode, var);
    if (n_fft == 512 && bits_per_sc == 6) return wofdm_select_kernel_n512_k6(layout, mode, var);
    if (n_fft == 1024 && bits_per_sc == 2) return wofdm_select_kernel_n1024_k2(layout, mode, var);
    if (n_fft == 1024 && bits_per_sc == 4) return wofdm_select_kernel_n1024_k4(layout, mode, var);
    if (n_fft == 1024 && bits_per_sc == 6) return wofdm_select_kernel_n1024_k6(layout, mode, var);
    return nullptr;
}
// the kernels of the built geometries (wofdm_geo_table): wofdm_frames_kernel<256, k, wofdm_geo_layout(geo), false, false, 0, geo>,
// in translation units of their own (wofdm_kernel.hip with -DWOFDM_TU_GEO -DWOFDM_TU_N=256 -DWOFDM_TU_K=<k>: a kernel's register
// allocation answers to what is compiled beside it, and the generic kernels are to come out as they are); nullptr: none built
wofdm_kernel_fn wofdm_select_kernel_geo_n256_k2(int geo);
wofdm_kernel_fn wofdm_select_kernel_geo_n256_k4(int geo);
wofdm_kernel_fn wofdm_select_kernel_geo_n256_k6(int geo);
static inline wofdm_kernel_fn wofdm_select_kernel_geo(int n_fft, int bits_per_sc, int geo)
{
    if (n_fft == 256 && bits_per_sc == 2) return wofdm_select_kernel_geo_n256_k2(geo);
    if (n_fft == 256 && bits_per_sc == 4) return wofdm_select_kernel_geo_n256_k4(geo);
    if (n_fft == 256 && bits_per_sc == 6) return wofdm_select_kernel_geo_n256_k6(geo);
    return nullptr;
}
// which build of wofdm_kernel.hip a unit is (WOFDM_UNIT_BUILD there; 0 = the product's): the generic unit of (N, k) and the unit of
// its built geometries.  configure() takes a built geometry's kernel only where the two agree -- a library with one generic unit
// swapped for another build (tests/native: the fault-injected one) then runs that unit's kernels, as it means to.
// (Why here and not in that library's Makefile: it links the product's wofdm_kernel_n*_k*.o by wildcard, the *_geo.o units with them,
// and the rule must hold for any such library -- a developer variant too -- without each of them knowing which units to swap in pairs.)
int wofdm_kernel_unit_build_n256_k2(void);
int wofdm_kernel_unit_build_n256_k4(void);
int wofdm_kernel_unit_build_n256_k6(void);
int wofdm_kernel_geo_unit_build_n256_k2(void);
int wofdm_kernel_geo_unit_build_n256_k4(void);
int wofdm_kernel_geo_unit_build_n256_k6(void);
static inline bool wofdm_geo_unit_matches(int n_fft, int bits_per_sc)
{
    if (n_fft == 256 && bits_per_sc == 2) return wofdm_kernel_unit_build_n256_k2() == wofdm_kernel_geo_unit_build_n256_k2();
    if (n_fft == 256 && bits_per_sc == 4) return wofdm_kernel_unit_build_n256_k4() == wofdm_kernel_geo_unit_build_n256_k4();
    if (n_fft == 256 && bits_per_sc == 6) return wofdm_kernel_unit_build_n256_k6() == wofdm_kernel_geo_unit_build_n256_k6();
    return false;
}
hipError_t wofdm_philox_kat_launch(const uint32_t *ctr_key_dev, uint32_t *out_dev, hipStream_t s);

// ---- The auxiliary kernels (wofdm_aux.hip, one translation unit per DFT length: -DWOFDM_TU_N=<N>) ----

// Tx waveform + averaged periodogram for a batch of jobs (wofdm_tx_psd_batch), every N.  A job's waveform sits at
// x + x_off (len samples); its periodogram is summed by the work items item0 ... item0 + n_items - 1 (one workgroup
// each, consecutive slices), whose partial spectra a second pass adds in that order.
struct wofdm_bjob {
    int32_t block, cp, cs, overlap;   // symbol block of X, CP, CS, overlapping tail samples
    int32_t w_off, len;               // offset of the job's Tx window in w_tx; waveform length overlap + S (P - overlap)
    int32_t item0, n_items;
    int64_t x_off;
};
struct wofdm_bitem {
    int32_t job, slice0, n_slices, pad;
};
// transforms of 1024 points (FL = 8 N > 1024: R = FL / 1024 decimated sub-sequences of a slice, one wave each) or of FL
// points (R = 1); 8 waves per workgroup = 8 / R slices at a time, 4 rounds per work item
__host__ __device__ constexpr int wofdm_psd_batch_r(int n_fft) { return 8 * n_fft > 1024 ? 8 * n_fft / 1024 : 1; }
__host__ __device__ constexpr int wofdm_psd_batch_slices(int n_fft) { return 4 * (8 / wofdm_psd_batch_r(n_fft)); }

// Masked jobs of wofdm_tx_psd_batch_masked: the spectral Tx mask as fast convolution over 8 n_fft points (3 P - 2 of them
// in use), so P <= (8 n_fft + 2) / 3 -- every cp + cs <= n_fft / 2 and more.  A masked job keeps the whole filtered symbols
// y_s[2 P - 1] at Y + y_off before the gather that forms its waveform; its mask spectrum is spec[spec][8 n_fft].
struct wofdm_mjob {
    int32_t job, spec;                // index into the job table; index of the mask's fast-convolution spectrum
    int64_t y_off;
};
__host__ __device__ constexpr int wofdm_txmask_batch_pmax(int n_fft) { return (8 * n_fft + 2) / 3; }

// Tx PAPR (wofdm_tx_papr): one chunk of n_jobs consecutive (pair, frame) items, item = pair * frames + f, from item0 on.  A job
// is one frame: its symbol grid X[job][S][n_fft], its waveform x[job][T] (T = beta + S B) and, masked, its filtered symbols
// Y[job][S][2P - 1]; the job tables are written on the device by the generation kernel.  A period is (item, symbol).
#define WOFDM_PAPR_MAX_JOBS 65535          // a chunk's jobs are the y dimension of the waveform kernels' grids
#define WOFDM_PAPR_MAX_BINS 8192           // the workgroup-local histogram is 4 n_bins bytes of LDS
struct wofdm_pparams {
    int32_t S, k, P, cp, cs, beta, n_jobs, n_bins;
    float lo_db, step_db;
    uint32_t seed_lo, seed_hi;
    uint64_t item0, frames, frame_offset;
    uint32_t wdiv;                    // cells per window pair: the item's "pair" is its CELL of the label stream, its window that
                                      // of pair / wdiv (wofdm_tx_papr: 1; wofdm_rx_profile: n_snr n_channels)
    uint32_t stream;                  // label stream of philox.h the grids are drawn from: 0 = WOFDM_STREAM_BITS (the frames of
                                      // a plan), WOFDM_STREAM_ACI for the neighbour of wofdm_rx_profile_aci (with its own amask)
    const float *wtx;                 // [pairs][P]
    const uint8_t *amask;             // [n_fft] 0 / 1, or null = every bin loaded
    const float2 *spec;               // [8 n_fft] fast-convolution spectrum of the Tx mask, or null = no mask
    wofdm_bjob *jobs;                 // [n_jobs]
    wofdm_mjob *mjobs;                // [n_jobs] (masked)
    float2 *X, *x, *Y;
    unsigned long long *hist;         // [pairs][n_bins], accumulated into
    uint32_t *max_bits;               // [pairs] bit pattern of the largest PAPR so far (non-negative floats order as integers)
    float2 *periods;                  // [pairs * frames * S] {peak, energy}, or null
};

// Receive profile (wofdm_rx_profile): the chunk of wofdm_pparams with items = (cell, frame), item = cell * frames + f -- the
// Tx chain leaves X[job][S][n_fft] and x[job][T] --, one workgroup per item, then the ordered sums of the chunk onto the totals.
struct wofdm_rparams {
    int32_t S, k, B, T, NL, delta, gam, kap, n_ch, n_snr, n_jobs;
    uint32_t seed_lo, seed_hi;
    uint64_t item0, frames, frame_offset;
    const float2 *X, *x;              // the chunk's symbol grids and waveforms
    const float *wrx;                 // [pairs][n_fft + delta]
    const float2 *h;                  // [n_ch][WOFDM_LT], zero padded
    const float *nlin;                // [n_snr] 10^(-snr / 10)
    const uint8_t *amask;             // [n_fft] 0 / 1, or null = every bin loaded
    float *part_pow;                  // [n_jobs][n_fft] sum |Xhat - X|^2 of the item
    uint32_t *part_cnt;               // [n_jobs][n_fft] bit errors | symbol errors << 16 of the item
    unsigned long long *errs;         // [cells][n_fft][2], accumulated into
    double *pow;                      // [cells][n_fft], accumulated into
};
// The adjacent-band neighbour of wofdm_rx_profile_aci, a second argument of the receive kernel's ACI arm (the plain kernel and
// its parameters stay as they are): its waveforms xi[job][Ti], Ti = T + B (S + 1 symbols), its channels, its amplitude; the
// victim's on-air sample t carries a_lvl xi[t + ioff], ioff = B - aci_delay in [1, B].
struct wofdm_aparams {
    const float2 *xi;
    const float2 *hi;                 // [n_ch][WOFDM_LT], zero padded
    int32_t Ti, ioff;
    float a_lvl;
};
// The receiver offsets of wofdm_rx_profile_sync, a second argument of wofdm_rxprof_sync_kernel: the Tx chain and pass 1 of an
// item run once, pass 2 once per point with the receive windows moved by theta samples and every sample under them rotated by
// base[point][s] e^{2 pi i eps m / n_fft} (m: index under the window).  base is prepared on the host in double precision:
// exp(2 pi i frac(eps (s B + gam + theta) / n_fft)) for a free-running oscillator, 1 for a tracked one.  With it the partials
// and totals of wofdm_rparams carry a leading point axis: part_pow, part_cnt [n_jobs][n_points][n_fft]; errs, pow
// [n_points][cells][n_fft].
#define WOFDM_SYNC_POINTS 64               // WOFDM_SYNC_MAX_POINTS of include/wofdm.h
struct wofdm_spoint {
    int32_t theta;                    // |theta| < B
    float eps;                        // subcarrier spacings
};
struct wofdm_sparams {
    int32_t n_points;
    uint64_t cells;
    const wofdm_spoint *pts;          // [n_points]
    const float2 *base;               // [n_points][S]
    float *sym_pow;                   // [n_jobs][n_points][S] sum over the loaded bins of |Xhat - X|^2 of symbol s (s = 0: 0)
    uint32_t *sym_cnt;                // [n_jobs][n_points][S] bit errors | symbol errors << 16 of symbol s
    unsigned long long *sym_errs;     // [n_points][cells][S - 1][2], accumulated into
    double *sym_tot;                  // [n_points][cells][S - 1], accumulated into
};
// The moving channel of wofdm_rx_profile_doppler, a third argument of wofdm_rxprof_doppler_kernel: per track and channel the
// tap vectors at the on-air indices 0, knot_step, 2 knot_step, ... (the knots); the tap l at on-air index a is
// K[q][l] + f (K[q + 1][l] - K[q][l]), q = min(a / knot_step, n_knots - 2), f = (a - q knot_step) / knot_step, taken at the
// OUTPUT sample of the convolution.  The tracks take the place of wofdm_sparams' points (n_points = n_tracks; pts and base
// are not read): partials and totals carry a leading track axis, and wofdm_rxprof_sync_reduce_kernel adds them up.
#define WOFDM_DOPPLER_TRACKS 16            // WOFDM_DOPPLER_MAX_TRACKS of include/wofdm.h
#define WOFDM_DOPPLER_KNOTS 64             // WOFDM_DOPPLER_MAX_KNOTS of include/wofdm.h
struct wofdm_dparams {
    const float2 *knots;              // [n_tracks][n_ch][n_knots][WOFDM_LT], zero padded
    int32_t n_knots, knot_step;       // (n_knots - 1) knot_step >= T + n_taps - 2: the knots cover the frame
};
// The oscillator phase noise of wofdm_rx_profile_pn, a third argument of wofdm_rxprof_pn_kernel.  wofdm_pn_walk_kernel leaves
// the unit walk of every item of the chunk in walk, u[a] = xi[0] + ... + xi[a] over the on-air indices a < S B a receiver at
// timing 0 reads (xi: stream 3 of philox.h), once per frame whatever the number of points; the point scales it: the sample
// at a is rotated by e^{i sigma u[a]}, or by e^{i sigma (u[a] - mean of u under the symbol's window)} where the common
// phase error is tracked.  The points take the place of wofdm_sparams' points (pts and base of it are not read).
#define WOFDM_PN_POINTS 16                 // WOFDM_PN_MAX_POINTS of include/wofdm.h
struct wofdm_pnpoint {
    double turn;                      // sigma / (2 pi) = sqrt(beta / (2 pi n_fft)) (host, double, from beta as stored)
    int32_t tracked, pad;
};
struct wofdm_pnparams {
    const wofdm_pnpoint *pts;         // [n_points]
    double *walk;                     // [n_jobs][S B]
};

// the launchers of one DFT length
struct wofdm_aux_fns {
    // closed-form ICI/ISI power kernels
    hipError_t (*interf)(int jobs, int P, int B, int mu, int delta, int gam, int kap, int n_ch, const float *wtx,
                         const float *wrx, const float2 *h, float *power, hipStream_t s);
    // Closed-form ICI/ISI power of the half-band, masked system (wofdm_interference_masked): the masked on-air pulses of every
    // loaded bin once per window pair into cols[pairs][n_fft][JP] (J = B + P - 1 samples each, JP >= J the row pitch), then one
    // workgroup per (pair, channel) job.  g: the mask's circular impulse response [2P - 1], or null = no mask; amask: [n_fft]
    // 0 / 1, or null = every bin loaded; wanted may be null.
    hipError_t (*interf_masked)(int pairs, int n_ch, int P, int B, int mu, int delta, int gam, int kap, int JP, const float *wtx,
                                const float *wrx, const float2 *h, const float2 *g, const uint8_t *amask, float2 *cols,
                                float *power, float *wanted, hipStream_t s);
    // Tx waveform + averaged periodogram (row f4), N <= 256 (transform length 8 N <= 2048); null above
    hipError_t (*psd)(int P, int mu, int rho, int overlap, int no_symbols, const float *wtx, const float2 *X, float2 *x, int len,
                      float *psd, hipStream_t s);
    hipError_t (*psd_batch)(int n_jobs, int no_symbols, int n_items, const wofdm_bjob *jobs, const wofdm_bitem *items,
                            const float *wtx, const float2 *X, float2 *x, float *partial, float *psd, hipStream_t s);
    // plain_jobs: the n_plain unmasked jobs (waveform by wofdm_txwave_batch_kernel, as psd_batch); mjobs: the n_masked masked
    // ones; max_len: longest masked waveform.  Periodogram and reduction over the whole table `jobs`.
    hipError_t (*psd_batch_masked)(int n_jobs, int no_symbols, int n_items, const wofdm_bjob *jobs, const wofdm_bitem *items,
                                   int n_plain, const wofdm_bjob *plain_jobs, int n_masked, const wofdm_mjob *mjobs, int max_len,
                                   const float2 *spec, float2 *Y, const float *wtx, const float2 *X, float2 *x, float *partial,
                                   float *psd, hipStream_t s);
    // Tx PAPR of one chunk of frames (wofdm_pparams): symbol grids from the Philox label streams, the waveforms by the kernels of
    // psd_batch / psd_batch_masked with one job per frame, then {peak, energy} of every symbol period and its histogram bin.
    hipError_t (*papr)(const wofdm_pparams *p, hipStream_t s);
    // Receive profile of one chunk of (cell, frame) items: the Tx chain of papr (p->wdiv = cells per window pair), one
    // workgroup per item for its per-bin error counts and error power, and the sums of the chunk in frame order.
    hipError_t (*rx_profile)(const wofdm_pparams *p, const wofdm_rparams *r, hipStream_t s);
    // The same beside an adjacent-band neighbour (wofdm_rx_profile_aci): a second pass through the Tx chain with pa (S + 1
    // symbols of the label stream pa->stream on the allocation pa->amask, tables and buffers of its own), and the ACI arm of the
    // receive kernel, which adds the neighbour's waveform a->xi through a->hi to every received sample of pass 2.
    hipError_t (*rx_profile_aci)(const wofdm_pparams *p, const wofdm_pparams *pa, const wofdm_rparams *r, const wofdm_aparams *a,
                                 hipStream_t s);
    // The same under receiver timing and carrier offsets (wofdm_rx_profile_sync): the Tx chain once, wofdm_rxprof_sync_kernel
    // (pass 1 once per item, pass 2 once per point of sp), and the ordered sums per point, per bin and per data symbol.
    hipError_t (*rx_profile_sync)(const wofdm_pparams *p, const wofdm_rparams *r, const wofdm_sparams *sp, hipStream_t s);
    // The same over channels that move within the frame (wofdm_rx_profile_doppler): the Tx chain once,
    // wofdm_rxprof_doppler_kernel (pass 1 and pass 2 once per track of dp, sp->n_points tracks), and rx_profile_sync's sums.
    hipError_t (*rx_profile_doppler)(const wofdm_pparams *p, const wofdm_rparams *r, const wofdm_sparams *sp,
                                     const wofdm_dparams *dp, hipStream_t s);
    // The same under oscillator phase noise (wofdm_rx_profile_pn): the Tx chain once, wofdm_pn_walk_kernel (the items' unit
    // walks, once), wofdm_rxprof_pn_kernel (pass 1 once per item, pass 2 once per point of pn), and rx_profile_sync's sums.
    hipError_t (*rx_profile_pn)(const wofdm_pparams *p, const wofdm_rparams *r, const wofdm_sparams *sp, const wofdm_pnparams *pn,
                                hipStream_t s);
};
const wofdm_aux_fns *wofdm_aux_n64(void);
const wofdm_aux_fns *wofdm_aux_n128(void);
const wofdm_aux_fns *wofdm_aux_n256(void);
const wofdm_aux_fns *wofdm_aux_n512(void);
const wofdm_aux_fns *wofdm_aux_n1024(void);
static inline const wofdm_aux_fns *wofdm_aux(int n_fft)
{
    switch (n_fft) {
    case 64: return wofdm_aux_n64();
    case 128: return wofdm_aux_n128();
    case 256: return wofdm_aux_n256();
    case 512: return wofdm_aux_n512();
    case 1024: return wofdm_aux_n1024();
    }
    return nullptr;
}
