// wofdm_link.h -- the five impairments combined (wofdm_rx_profile_link): the parameters of the receive body's seventh arm
// (wofdm_aux.hip), and the same arm with soft decisions (wofdm_rx_profile_soft); the chunk of a receive-profile call and its
// launcher, one table per DFT length beside wofdm_aux_fns and wofdm_pa_fns.  A header of its own:
// wofdm_kernel.h is part of the frame kernels' source hash (profiles/hbm_traffic.json), and nothing here touches them
// (GNUmakefile tells make which objects depend on this file, for the same reason).
#pragma once
#include "wofdm_pa.h"
#include "philox.h"

#define WOFDM_LINK_POINTS 16               // WOFDM_LINK_MAX_POINTS of include/wofdm.h

// What a point of wofdm_rx_profile_link adds to the points of the arms it switches on: those stay where their arms read them --
// the receiver offsets in wofdm_sparams (pts, base), the oscillator in wofdm_pnparams (pts), the amplifier in wofdm_paparams (pts,
// y: the point's waveform) --, all with the link call's n_points points.
struct wofdm_lpoint {
    int32_t track;                    // row of wofdm_dparams' knots: a track of the call, or the static one behind them
    int32_t aci_on;                   // the neighbour is on the air for this point
    int32_t ioff;                     // B - aci_delay in [1, B]
    float a_lvl;                      // 10^(aci_level_db / 20)
};
// A seventh argument of wofdm_rxprof_link_kernel.  wofdm_dparams' knots hold n_tracks + 1 tracks: behind the call's own the
// static channel h at every knot, which is what a point without a track reads (with equal knots the tap is the knot, bit for
// bit); wofdm_aparams' ioff and a_lvl are not read, its xi only where a point has aci_on.
struct wofdm_lparams {
    const wofdm_lpoint *pts;          // [n_points]
};

// The soft outputs of wofdm_rx_profile_soft, an eighth argument of wofdm_rxprof_soft_kernel (the link arm with the demapper
// switched on).  For the decision of loaded bin n, data symbol s >= 1: nu = |G[n]|^2 v W2, v = g^2 Pn / NL the per-sample noise
// variance pass 1 put on the air for the point, W2 = w2[pair]; Lambda_i the max-log bit metrics over nu; and per scale j
// pen_j = sum_i log2(1 + 2^(-(1 - 2 b_i) cs[j] Lambda_i)), cs[j] = c_j log2(e) formed on the host.  The wave of symbol s writes
// pen_j of its bins to bit_part (0 on unloaded bins), coalesced, and leaves their sum over the loaded bins -- a lane's bins
// ascending, then papr_wave_reduce -- in sym_part; wofdm_rxprof_soft_frame_kernel adds a frame's symbols, ascending in single
// precision, into the first symbol's element, and wofdm_rxprof_soft_reduce_kernel the frames onto the fp64 totals, ascending.
#define WOFDM_SOFT_SCALES 16               // WOFDM_SOFT_MAX_SCALES of include/wofdm.h
struct wofdm_softparams {
    int32_t n_scales;
    float cs[WOFDM_SOFT_SCALES];      // c_j log2(e)
    const float *w2;                  // [pairs] sum of the Rx window's squares (host, double, stored in single)
    float *bit_part;                  // [n_jobs][n_points][S - 1][n_scales][n_fft]; [..][0][..][..] becomes the frame's sum
    float *sym_part;                  // [n_jobs][n_points][n_scales][S] (s = 0 is not written and not read)
    double *bit_tot;                  // [n_points][cells][n_scales][n_fft], accumulated into
    double *sym_tot;                  // [n_points][cells][n_scales][S - 1], accumulated into
};

// The tracking receiver of wofdm_rx_profile_tracking, a ninth argument of wofdm_rxprof_tracking_kernel (the link arm with the
// demapper and the TRACK flag): the comb of pilot bins and per point the two mechanisms.  A point with neither runs the soft
// kernel's statements; one with either equalises with Hhat_s = H0 + t (HL conj(rho) - H0), t = s / (S - 1), and the phase q_s
// (include/wofdm.h has the definition).  Pilot bins, and the last symbol of a point with post, count nothing.
struct wofdm_tpoint {
    int32_t cpe;                      // the per-symbol common phase from the comb
    int32_t post;                     // symbol S - 1 is a second known symbol
};
struct wofdm_trackparams {
    const uint8_t *pilots;            // [n_fft], or null: no comb
    const wofdm_tpoint *pts;          // [n_points]
};

// The coded link of wofdm_rx_profile_coded, a tenth argument of wofdm_rxprof_coded_kernel (the tracking kernel with the CODED
// flag) and the argument of wofdm_viterbi_kernel.  The receive kernel leaves, per bin of every data symbol, the k soft bits d =
// clamp(rint(llr_scale z_i), -127, 127) (include/wofdm.h) as one 8-byte store, padded with zeros; 0 where no decision is taken.
// The decoder reads a codeword's coded-stream index c at byte gather[c] of the codeword's block (cw_stride bytes apart): for the
// profile gather[c] = 8 n + i of position perm[c] = r k + i (n the r-th data bin), for wofdm_viterbi_decode perm[c] itself.
#define WOFDM_CODE_CODES 4                 // WOFDM_CODE_MAX of include/wofdm.h
struct wofdm_codeparams {
    float llr_scale;
    int8_t *soft;                     // [n_jobs][n_points][S - 1][n_fft][8]; the decoder alone: [n_cw][cw_stride]
    const int32_t *gather;            // [n_c]
    int32_t n_c, n_codes;
    int32_t rate[WOFDM_CODE_CODES], steps[WOFDM_CODE_CODES];   // steps: wofdm_code_steps(rate, n_c) >= 7
    int64_t cw_stride;                // bytes between the blocks of two codewords
    // the profile (bits null): codeword w is (job, point, data symbol), counted into errs unless pts[point].post and the last symbol
    unsigned long long *errs;         // [n_points][cells][n_codes][S - 1][2] {info-bit errors, codeword errors}, integer atomics
    const wofdm_tpoint *pts;          // [n_points]
    int32_t n_points, S1;             // S1 = S - 1
    uint64_t item0, frames, cells;
    // wofdm_viterbi_decode (errs null): the decoded bits and the final metrics of code 0
    uint8_t *bits;                    // [n_cw][steps[0]]
    int32_t *metric;                  // [n_cw], or null
    uint32_t n_cw;
};

// The streaming decoder wofdm_viterbi_long_kernel (wofdm_rx_profile_coded_frame, wofdm_viterbi_decode_long): the code, metric and
// rules of wofdm_viterbi_kernel, the survivor history in device memory instead of LDS -- hist holds the decisions in blocks of
// 64 steps: bit i of word [wave][block][s] is the decision into state s at step 64 block + i of the launch's wave-th codeword,
// 512 bytes per block, ceil(steps / 64) blocks per codeword.  One launch decodes ONE code; codeword w reads coded-stream index c at byte
// gather[c] of its block soft + w cw_stride.  A variant v is a codeword length: the profile has one per number of data symbols
// S_d in use -- variant 1 belongs to the points with post, variant 0 to the others --, the decoder alone only variant 0.
#define WOFDM_CODE_LONG_STEPS 1048576      // WOFDM_CODE_LONG_MAX_STEPS of include/wofdm.h
struct wofdm_longparams {
    const int8_t *soft;               // the profile: [n_jobs][n_points][S - 1][n_fft][8]; the decoder alone: [n_cw][n_c]
    unsigned long long *hist;         // [n_cw][hist_blocks][64]
    const int32_t *gather[2];         // [n_c[v]]; the profile: (S_d, perm, sym_rot and the data bins folded) 8 (N j + n) + i
    int32_t n_c[2], steps[2];         // steps[v] = wofdm_code_steps(rate, n_c[v]) in 7 ... WOFDM_CODE_LONG_STEPS, or 0: no codeword
    int32_t rate, hist_blocks;        // hist_blocks >= ceil(steps[v] / 64)
    int64_t cw_stride;
    uint32_t n_cw;                    // the launch's codewords; the profile: n_jobs n_points, codeword w = (job, point)
    // the profile (bits null): counted into errs[point][cell][n_codes][2] at code
    unsigned long long *errs;         // {info-bit errors, codeword errors}, integer atomics
    const wofdm_tpoint *pts;          // [n_points]
    int32_t n_points, code, n_codes;
    uint64_t item0, frames, cells;
    // wofdm_viterbi_decode_long (errs null)
    uint8_t *bits;                    // [n_cw][steps[0]]
    int32_t *metric;                  // [n_cw], or null
};

// The layered min-sum decoder wofdm_ldpc_kernel (wofdm_rx_profile_ldpc, wofdm_ldpc_decode) of the quasi-cyclic (J, L) code of
// include/wofdm.h.  One launch decodes ONE code, one workgroup per codeword; a codeword reads variable x < n at byte
// gather[v][wi n + x] of its block soft + w cw_stride, wi its index within the frame (the decoder alone: 0).  A variant v is a
// word length as in wofdm_longparams; the profile's grid is (n_jobs n_points, the largest W in use), and a workgroup whose wi is not
// below its variant's W leaves at once.  LDS: a header of WOFDM_LDPC_LDS_HEAD bytes (the counters, the J L shifts), Q as int16
// [L Z] rounded up to four bytes, R as int8 [edge][Z], edge = the layer's edges in column order, the layers one behind the other.
#define WOFDM_LDPC_BITS 16384              // WOFDM_LDPC_MAX_BITS of include/wofdm.h
#define WOFDM_LDPC_LDS_HEAD 304            // 4 int32 counters, 6 x 24 int16 shifts
#define WOFDM_LDPC_LDS_MAX 163584          // the 160 KiB of a gfx950 workgroup less the kernel's 256 static bytes (the OR's)
struct wofdm_ldpcparams {
    const int8_t *soft;               // the profile: [n_jobs][n_points][S - 1][n_fft][8]; the decoder alone: [n_cw][n]
    const int32_t *gather[2];         // [W[v] n[v]] at least
    int32_t n[2], W[2], Z[2];         // the word's positions, the words per frame (0: the variant is unused), the lift
    int32_t J, L, max_iter;
    int64_t cw_stride;
    uint32_t n_cw;                    // grid x; the profile: n_jobs n_points, block w = (job, point)
    // the profile (bits null): counted into errs[point][cell][n_codes][4] at code
    unsigned long long *errs;         // {info-bit errors, codeword errors, unconverged codewords, iterations}, integer atomics
    const wofdm_tpoint *pts;          // [n_points]
    int32_t n_points, code, n_codes;
    uint64_t item0, frames, cells;
    // wofdm_ldpc_decode (errs null)
    uint8_t *bits;                    // [n_cw][n[0]]
    int32_t *iters;                   // [n_cw]
    uint8_t *conv;                    // [n_cw]
};
// The decoder's LDS in bytes, host, launcher and kernels alike: Q's and R's, each rounded up to four bytes; the kernels carve by
// the same two functions.  (int suffices: before it sizes anything every caller has checked J <= 6 and L <= 24, and either Z <=
// 32767 -- ldpc_ok -- or n <= WOFDM_LDPC_BITS, of which Z is the lift.)
__host__ __device__ static inline int32_t wofdm_ldpc_q_bytes(int32_t n0) { return (2 * n0 + 3) & ~3; }        // n0 = L Z
__host__ __device__ static inline int32_t wofdm_ldpc_r_bytes(int32_t J, int32_t L, int32_t Z)
{
    return ((J * L - J * (J - 1) / 2) * Z + 3) & ~3;
}
static inline uint64_t wofdm_ldpc_lds(int32_t J, int32_t L, int32_t Z)
{
    return WOFDM_LDPC_LDS_HEAD + (uint64_t)wofdm_ldpc_q_bytes(L * Z) + (uint64_t)wofdm_ldpc_r_bytes(J, L, Z);
}

// The information stream of the coset view (wofdm_rx_profile_coset, wofdm_coset_info), a fifth Philox stream beside the four of
// philox.h -- defined here, philox.h being part of the frame kernels' source hash, which never draw it: block b of (seed, cell,
// frame) is philox4x32_10 of counter (b, frame lo, frame hi, 4 << 28 | cell) under key (seed lo, seed hi), and bit i of the
// frame's stream is bit i mod 32 of word (i mod 128) div 32 of block i div 128.  Neither the point nor the code enters it.
#define WOFDM_STREAM_INFO 4u
// word q (32 bits) of the stream; the word is picked by selects, never by an index (a block stays in registers)
__host__ __device__ __forceinline__ uint32_t wofdm_info_word(uint32_t seed_lo, uint32_t seed_hi, uint32_t cell, uint64_t frame, uint32_t q)
{
    const philox_out o = philox4x32_10(q >> 2, (uint32_t)frame, (uint32_t)(frame >> 32), (WOFDM_STREAM_INFO << 28) | cell, seed_lo, seed_hi);
    const uint32_t lo = (q & 1u) != 0 ? o.w[1] : o.w[0], hi = (q & 1u) != 0 ? o.w[3] : o.w[2];
    return (q & 2u) != 0 ? hi : lo;
}

// What the coset instantiations of the two decoders (wofdm_viterbi_coset_kernel, wofdm_ldpc_coset_kernel) take beside the
// decoder's own parameters: the call's key and first frame.  Workgroup w = (job, point) draws the stream of cell (item0 + job) /
// frames, frame frame_offset + (item0 + job) mod frames.
struct wofdm_cosetparams {
    uint32_t seed_lo, seed_hi;
    uint64_t frame_offset;
};
// the coset LDPC instantiation's LDS in bytes: the decoder's, and behind it the transmitted word as bits, one per variable < L Z
static inline uint64_t wofdm_ldpc_coset_lds(int32_t J, int32_t L, int32_t Z)
{
    return wofdm_ldpc_lds(J, L, Z) + 4ull * (((uint64_t)L * (uint64_t)Z + 31ull) / 32ull);
}

// Retransmissions with soft combining (wofdm_rx_profile_harq, wofdm_ldpc_harq_decode): what wofdm_ldpc_harq_kernel takes beside
// wofdm_ldpcparams and wofdm_cosetparams.  A group is `rounds` consecutive rows of soft bits that carry the same word; row r of
// workgroup w's group is block (w / n_points) rounds n_points + r n_points + w mod n_points of lp.soft in the profile (the
// chunk's frames [job][point], a group's frames one behind the other) and block w rounds + r in the decoder alone, cw_stride
// bytes apart.  The profile's grid x is (n_jobs / rounds) n_points: n_jobs, item0 and frames are multiples of rounds, so that
// no group straddles a chunk or a cell; the word is drawn from the group's first frame.  LDS: wofdm_ldpc_coset_lds.
#define WOFDM_HARQ_ROUNDS 8                // WOFDM_HARQ_MAX_ROUNDS of include/wofdm.h
#define WOFDM_HARQ_NF 13                   // WOFDM_HARQ_FIELDS of include/wofdm.h: lp.errs is [n_points][cells][n_codes][13]
struct wofdm_harqparams {
    int32_t rounds, combine;          // 1 ... WOFDM_HARQ_ROUNDS; 1: the sum of the rows so far (Chase), 0: the row alone
    int32_t *round;                   // wofdm_ldpc_harq_decode: [n_cw] the 1-based stop round, or null
};

// The stand-alone encoders (wofdm_conv_encode, wofdm_ldpc_encode): bits as bytes, one block per codeword
struct wofdm_convencparams {
    const uint8_t *info;              // [n_cw][steps - 6]
    uint8_t *coded;                   // [n_cw][n_c]
    int32_t rate, n_c, steps;         // steps = wofdm_code_steps(rate, n_c) in 7 ... WOFDM_CODE_LONG_STEPS
    uint32_t n_cw;
};
struct wofdm_ldpcencparams {
    const uint8_t *info;              // [n_cw][n - J Z]
    uint8_t *word;                    // [n_cw][n]
    int32_t J, L, n, Z;
    uint32_t n_cw;
};

// The coded link's unit (wofdm_code.hip, compiled once: none of its kernels knows the DFT length).  What the receive profile's
// chunk launcher in the per-N units calls behind the soft bits -- each *_enqueue checks its parameters first (hipErrorInvalidValue,
// nothing launched), `profile` saying which of the two uses of the struct they describe --
bool wofdm_viterbi_ok(const wofdm_codeparams &cd, bool profile);
void wofdm_viterbi_enqueue(const wofdm_codeparams &cd, hipStream_t s);       // wofdm_viterbi_kernel: grid (n_cw, n_codes), cd checked
hipError_t wofdm_viterbi_long_enqueue(const wofdm_longparams &lp, bool profile, hipStream_t s);           // one wave per codeword
hipError_t wofdm_viterbi_coset_enqueue(const wofdm_longparams &lp, const wofdm_cosetparams &cs, hipStream_t s);
hipError_t wofdm_ldpc_enqueue(const wofdm_ldpcparams &lp, bool profile, hipStream_t s);                   // one workgroup per codeword
hipError_t wofdm_ldpc_coset_enqueue(const wofdm_ldpcparams &lp, const wofdm_cosetparams &cs, hipStream_t s);
hipError_t wofdm_ldpc_harq_enqueue(const wofdm_ldpcparams &lp, const wofdm_cosetparams &cs, const wofdm_harqparams &hq, bool profile,
                                   hipStream_t s);
// -- and what the C ABI calls on data of the caller's (errs null, bits set): wofdm_viterbi_decode, wofdm_viterbi_decode_long,
// wofdm_ldpc_decode, wofdm_ldpc_harq_decode, wofdm_conv_encode, wofdm_ldpc_encode
hipError_t wofdm_viterbi_launch(const wofdm_codeparams *cd, hipStream_t s);
hipError_t wofdm_viterbi_long_launch(const wofdm_longparams *lp, hipStream_t s);
hipError_t wofdm_ldpc_launch(const wofdm_ldpcparams *lp, hipStream_t s);
hipError_t wofdm_ldpc_harq_launch(const wofdm_ldpcparams *lp, const wofdm_harqparams *hq, hipStream_t s);
hipError_t wofdm_conv_encode_launch(const wofdm_convencparams *ep, hipStream_t s);
hipError_t wofdm_ldpc_encode_launch(const wofdm_ldpcencparams *ep, hipStream_t s);

// The arms of the receive body (rxprof_body of wofdm_aux.hip, which says what each adds)
enum { RXP_PLAIN, RXP_ACI, RXP_SYNC, RXP_DOPPLER, RXP_PA, RXP_PN, RXP_LINK };

// One chunk of a receive-profile call, whichever of the twelve: the victim's Tx chain, the receive kernel's parameters, and the
// stages' parameter structs as the kernels take them.  The arm says which stages the chunk runs -- a stage's struct is read
// only where its arm or RXP_LINK is on --; the link arm runs every stage, its points switch them, and only its neighbour
// (no point has aci_on: nb_on = false), its demapper (wofdm_rx_profile_soft: soft_on) and, with the demapper, its tracking receiver
// (wofdm_rx_profile_tracking: track_on) are the call's to leave out.
struct wofdm_rxchunk {
    int32_t arm;                      // RXP_*
    bool nb_on, soft_on, track_on;    // RXP_ACI: nb_on is true; track_on needs soft_on
    bool code_on;                     // (wofdm_rx_profile_coded) needs track_on: the soft-bit stores and the decoder behind them
    bool frame_on;                    // (wofdm_rx_profile_coded_frame) needs code_on: wofdm_viterbi_long_kernel over the frame's
                                      // data symbols, one launch per code of cd, in the place of the per-symbol decoder
    wofdm_pparams tx, nb;             // the victim's Tx chain; the neighbour's (S + 1 symbols, its own stream, allocation, buffers)
    wofdm_rparams r;
    wofdm_aparams a;                  // RXP_LINK: ioff and a_lvl are the points'
    wofdm_sparams sp;
    wofdm_dparams dp;
    wofdm_paparams pa;
    wofdm_pnparams pn;
    wofdm_lparams lk;
    wofdm_softparams soft;
    wofdm_trackparams tk;
    wofdm_codeparams cd;              // frame_on: llr_scale, soft, n_codes and rate; errs and steps are not read
    wofdm_longparams fr;              // frame_on: hist, gather, n_c, hist_blocks, errs; the launcher fills in the rest
    int32_t fr_steps[WOFDM_CODE_CODES][2];   // frame_on: steps per code and variant
    int32_t n_tracks;                 // RXP_LINK: the tracks of dp's knots, the static one included
    int32_t max_theta;                // RXP_LINK: the largest timing offset of the points, or 0 (the knots cover the samples it reaches)
    bool ldpc_on;                     // (wofdm_rx_profile_ldpc) needs code_on, never with frame_on: wofdm_ldpc_kernel over the frame's
                                      // data symbols, one launch per code, in the place of the per-symbol decoder; of cd as frame_on
    wofdm_ldpcparams ld;              // ldpc_on: gather, n, W, errs; the launcher fills in the rest
    int32_t ld_code[WOFDM_CODE_CODES][3];    // ldpc_on: J, L, max_iter per code
    int32_t ld_Z[WOFDM_CODE_CODES][2];       // ldpc_on: the lift per code and variant
    bool coset_on;                    // (wofdm_rx_profile_coset) needs code_on, never with frame_on or ldpc_on: the coset instantiations of
                                      // both decoders behind one receive kernel, cs_nv launches over fr (rates in cd.rate, fr_steps) and
                                      // cs_nl over ld (ld_code, ld_Z); either count may be 0, cd.n_codes is not read
    int32_t cs_nv, cs_nl;
    wofdm_cosetparams cs;
    int32_t hq_rounds, hq_combine;    // (wofdm_rx_profile_harq) hq_rounds > 0 needs coset_on with cs_nv = 0: wofdm_ldpc_harq_kernel in
                                      // the place of the coset LDPC launches, ld.errs with WOFDM_HARQ_NF fields; r.n_jobs, r.item0
                                      // and r.frames are multiples of hq_rounds
};

struct wofdm_link_fns {
    // One chunk of any receive profile, on stream s: the Tx chain, the neighbour's, the amplifier's waveforms and power sums,
    // the items' unit walks, the arm's receive kernel, the ordered sums (per point where the arm has points), the power sums in
    // frame order, the demapper's ordered sums -- each where its stage is on, in this order.
    hipError_t (*rx_profile_chunk)(const wofdm_rxchunk *c, hipStream_t s);
};
const wofdm_link_fns *wofdm_aux_link_n64(void);
const wofdm_link_fns *wofdm_aux_link_n128(void);
const wofdm_link_fns *wofdm_aux_link_n256(void);
const wofdm_link_fns *wofdm_aux_link_n512(void);
const wofdm_link_fns *wofdm_aux_link_n1024(void);
static inline const wofdm_link_fns *wofdm_aux_link(int n_fft)
{
    switch (n_fft) {
    case 64: return wofdm_aux_link_n64();
    case 128: return wofdm_aux_link_n128();
    case 256: return wofdm_aux_link_n256();
    case 512: return wofdm_aux_link_n512();
    case 1024: return wofdm_aux_link_n1024();
    }
    return nullptr;
}
