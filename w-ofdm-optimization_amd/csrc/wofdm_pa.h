// wofdm_pa.h -- the memoryless power amplifier behind the Tx chain (wofdm_rx_profile_pa, wofdm_tx_psd_batch_pa): the
// parameters of its kernels (wofdm_aux.hip) and the PSD's launcher, one table per DFT length beside wofdm_aux_fns (the receive
// profile's chunk is launched through wofdm_link.h).  A header of its own: wofdm_kernel.h is part of the frame kernels' source
// hash (profiles/hbm_traffic.json), and nothing here touches them (GNUmakefile tells make which objects depend on this file,
// for the same reason).
#pragma once
#include "wofdm_kernel.h"

#define WOFDM_PA_POINTS 16                 // WOFDM_PA_MAX_POINTS of include/wofdm.h
#define WOFDM_PA_M_LINEAR 0                // WOFDM_PA_LINEAR, WOFDM_PA_RAPP, WOFDM_PA_CLIP of include/wofdm.h
#define WOFDM_PA_M_RAPP 1
#define WOFDM_PA_M_CLIP 2

// One amplifier as pa_amplify() reads it: y = g x, rho = |x| / a_sat; Rapp g = (1 + rho^(2p))^(-1/(2p)), soft limiter
// g = min(1, 1 / rho), linear y = x without arithmetic.
struct wofdm_papoint {
    int32_t model;
    float two_p, inv_two_p;           // 2 p and 1 / (2 p) of the Rapp model (host, from smooth in double)
    int32_t pad;
};

// The amplifier of wofdm_rx_profile_pa, a third argument of wofdm_rxprof_pa_kernel beside wofdm_rparams and wofdm_sparams (the
// points take the place of wofdm_sparams' points; pts and base of it are not read).  wofdm_pa_wave_kernel leaves the amplified
// waveform of (job, point) in y -- a linear point's is x itself and is not written -- and the job's two power sums in pwr.
struct wofdm_paparams {
    int32_t n_points, pairs;
    const wofdm_papoint *pts;         // [n_points]
    const float *asat;                // [n_points][pairs] saturation amplitude (host, double, stored in single precision)
    float2 *y;                        // [n_jobs][n_points][T]
    float *pwr;                       // [n_jobs][n_points][2] {sum |x|^2, sum |y|^2} over the T samples of the job's frame
    double *pwr_tot;                  // [n_points][cells][2], accumulated into (frame order)
};

// The amplifier of one job of wofdm_tx_psd_batch_pa: model < 0 = none; a_sat^2 = mean |x|^2 of the job's waveform times scale
struct wofdm_pajob {
    int32_t model;
    float two_p, inv_two_p;
    int32_t pad;
    double scale;                     // 10^(ibo_db / 10)
};

struct wofdm_pa_fns {
    // wofdm_tx_psd_batch_pa: psd_batch_masked of wofdm_aux_fns (n_masked = 0: every job in plain_jobs) with, between the
    // waveform kernels and the periodogram, the jobs' mean powers (power[n_jobs][2] = {sum |x|^2, sum |y|^2}, device) and the
    // amplifier on the jobs that have one.
    hipError_t (*psd_batch_pa)(int n_jobs, int no_symbols, int n_items, const wofdm_bjob *jobs, const wofdm_bitem *items,
                               int n_plain, const wofdm_bjob *plain_jobs, int n_masked, const wofdm_mjob *mjobs, int max_len,
                               const float2 *spec, float2 *Y, const float *wtx, const float2 *X, float2 *x, float *partial,
                               float *psd, const wofdm_pajob *pa, float *power, hipStream_t s);
};
const wofdm_pa_fns *wofdm_aux_pa_n64(void);
const wofdm_pa_fns *wofdm_aux_pa_n128(void);
const wofdm_pa_fns *wofdm_aux_pa_n256(void);
const wofdm_pa_fns *wofdm_aux_pa_n512(void);
const wofdm_pa_fns *wofdm_aux_pa_n1024(void);
static inline const wofdm_pa_fns *wofdm_aux_pa(int n_fft)
{
    switch (n_fft) {
    case 64: return wofdm_aux_pa_n64();
    case 128: return wofdm_aux_pa_n128();
    case 256: return wofdm_aux_pa_n256();
    case 512: return wofdm_aux_pa_n512();
    case 1024: return wofdm_aux_pa_n1024();
    }
    return nullptr;
}
