// wofdm_link.h -- the five impairments combined (wofdm_rx_profile_link): the parameters of the receive body's seventh arm
// (wofdm_aux.hip) and its launcher, one table per DFT length beside wofdm_aux_fns and wofdm_pa_fns; and the same arm with soft
// decisions (wofdm_rx_profile_soft).  A header of its own:
// wofdm_kernel.h is part of the frame kernels' source hash (profiles/hbm_traffic.json), and nothing here touches them
// (GNUmakefile tells make which objects depend on this file, for the same reason).
#pragma once
#include "wofdm_pa.h"

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

struct wofdm_link_fns {
    // wofdm_rx_profile_link, one chunk: the Tx chain once, the neighbour's (nb != null: a point has aci_on) once, the points'
    // amplified waveforms and power sums, the items' unit walks, wofdm_rxprof_link_kernel (both passes once per point),
    // rx_profile_sync's ordered sums and the power sums in frame order.  n_tracks: the tracks of dp's knots, the static one
    // included; max_theta: the largest timing offset of the points, or 0 (the knots cover the samples it reaches).
    hipError_t (*rx_profile_link)(const wofdm_pparams *p, const wofdm_pparams *nb, const wofdm_rparams *r, const wofdm_aparams *a,
                                  const wofdm_sparams *sp, const wofdm_dparams *dp, const wofdm_paparams *pa,
                                  const wofdm_pnparams *pn, const wofdm_lparams *lk, int n_tracks, int max_theta, hipStream_t s);
    // wofdm_rx_profile_soft, one chunk: rx_profile_link with wofdm_rxprof_soft_kernel in the link kernel's place, and behind the
    // ordered sums wofdm_rxprof_soft_reduce_kernel's
    hipError_t (*rx_profile_soft)(const wofdm_pparams *p, const wofdm_pparams *nb, const wofdm_rparams *r, const wofdm_aparams *a,
                                  const wofdm_sparams *sp, const wofdm_dparams *dp, const wofdm_paparams *pa,
                                  const wofdm_pnparams *pn, const wofdm_lparams *lk, const wofdm_softparams *so, int n_tracks,
                                  int max_theta, hipStream_t s);
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
