/*
 * wofdm.h -- C ABI of libwofdm_hip.so, the MI355X (gfx950) implementation of
 * the w-OFDM Monte-Carlo BER hot path.
 *
 * The reference has no FFI: the hot path is a MATLAB local function and a
 * Python method.  The entry points below are what a binding for that path
 * replaces:
 *
 *   wofdm_run              <- ber = run_simulation(ensemble, symbolsPerTx, bitsPerSubcarrier,
 *                                numSubcar, cpLength, csLength, windowTx, channel, snr, tailTx,
 *                                tailRx, windowRx, prefixRemovalLength, circularShiftLength)
 *                             matlab/main_BER_calculation.m:230-274, batched over the
 *                             (window pair x SNR x channel) loop nest of lines 64-201;
 *                          <- wOFDMSystem.run_simulation(channel_models, window_tx, window_rx,
 *                                ensemble, snr_arr, no_symbols)
 *                             python/ofdm_utils/wofdm_simulation.py:432-481 (loop nest 168-242)
 *   wofdm_plan_*           <- the same, split into "upload constants once" + "launch a frame
 *                             range", so a driver can shard frames over GPUs and keep the
 *                             constants resident in HBM
 *   wofdm_*_injected       <- the same frame pipeline with the random draws
 *                             (main_BER_calculation.m:246,290 / wofdm_simulation.py:136,183)
 *                             supplied by the caller -- parity / HBM-streaming mode
 *
 * Conventions: plain pointers and sizes only.  `*_dev` pointers are device (HBM) addresses
 * on the plan's GPU, all others are host addresses.  All pointers are caller-owned and not
 * retained after the call returns (plans copy what they need).  Every function returns
 * WOFDM_OK (0) or a negative WOFDM_E_* code; wofdm_last_error() gives the message of the
 * last failure on the calling thread.  There is no CPU fallback: without a usable gfx950
 * device every compute entry point fails with WOFDM_E_HIP.
 *
 * A *cell* is one (window pair, SNR, channel) triple, cell = (pair*n_snr + snr)*n_channels
 * + channel.  counts[cell][4] = {bit errors, bits, symbol errors, symbols} over the data
 * symbols 1..S-1 of every frame (symbol 0 is the pilot, main_BER_calculation.m:250,266-268);
 * counters are ACCUMULATED into, never reset by a launch.
 */
#ifndef WOFDM_H
#define WOFDM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WOFDM_ABI_VERSION 1

#define WOFDM_OK            0
#define WOFDM_E_INVALID    -1   /* NULL pointer / inconsistent lengths                  */
#define WOFDM_E_UNSUPPORTED -2  /* N, k, S, taps or tails outside the built kernels     */
#define WOFDM_E_HIP        -3   /* HIP runtime error (no device, launch failure, ...)   */
#define WOFDM_E_NOMEM      -4

#define WOFDM_MAX_TAPS     21   /* taps of the reference's 200 ns Veh-A lines           */
#define WOFDM_MAX_SYMS     16   /* symbolsPerTx (matlab/window_optimization.m:39-47)    */

typedef struct wofdm_cfg {
    int32_t  n_fft;            /* N: 64, 128, 256, 512, 1024                                */
    int32_t  bits_per_sc;      /* k: 2, 4, 6 (QPSK, 16-QAM, 64-QAM, MATLAB Gray labels)     */
    int32_t  syms_per_frame;   /* S: 2..16, symbol 0 = pilot                                */
    int32_t  cp, cs;           /* mu, rho                                                   */
    int32_t  tail_tx, tail_rx; /* beta, delta (delta even)                                  */
    int32_t  prefix_rm;        /* gamma; N + delta + gamma == N + mu + rho - beta required  */
    int32_t  circ_shift;       /* kappa                                                     */
    int32_t  n_taps;           /* L <= WOFDM_MAX_TAPS                                       */
    int32_t  n_channels, n_snr, n_window_pairs;
    int32_t  noise_before_truncate; /* 1: MATLAB order (m:260-261); 0: Python (py:208-215)  */
    uint64_t frames_per_cell;  /* frames [frame_offset, frame_offset+frames_per_cell)       */
    uint64_t frame_offset;     /*   of every cell (global frame index keys the RNG)         */
    uint64_t seed;
    /* All 64 bits of seed and of the global frame index frame_offset + f key the random streams (csrc/philox.h: key =
     * (seed lo, seed hi), counter = (block, frame lo, frame hi, stream << 28 | cell)): two seeds, or two frame ranges, that
     * differ in any bit are independent experiments, and frame_offset + frames_per_cell may cross 2^32.  The cell index
     * shares its counter word with the stream id, so n_channels * n_snr * n_window_pairs must stay below 2^28
     * (WOFDM_E_UNSUPPORTED otherwise). */
} wofdm_cfg;

/* Optional stage dump of ONE frame (host float buffers, complex = interleaved re,im;
 * any pointer may be NULL).  Same stages as the oracle's dump. */
typedef struct wofdm_dump {
    uint8_t *labels_tx;  /* [S][N]                                      */
    float   *X;          /* [S][N][2]                                   */
    float   *tx;         /* [beta + S*B][2]                             */
    float   *conv;       /* [T + L - 1][2]                              */
    float   *rx;         /* [S*B][2]                                    */
    float   *Y;          /* [S][N][2]  (the kernels leave circular_shift, m:313-333, to the equaliser, which
                          * divides the resulting per-subcarrier phase out; the dump puts that phase,
                          * e^{+2 pi i (kappa + delta/2) n / N}, back on the host, so this IS the reference's Y) */
    float   *Xhat;       /* [S-1][N][2]                                 */
    uint8_t *labels_rx;  /* [S-1][N]                                    */
    float   *gain;       /* [1]                                         */
    float   *unit_noise; /* [noise_len][2] the unit normals the kernel used */
} wofdm_dump;

typedef struct wofdm_plan wofdm_plan;

int         wofdm_version(void);
int         wofdm_device_count(void);            /* < 0 on HIP failure                    */
const char *wofdm_last_error(void);
int         wofdm_noise_len(const wofdm_cfg *cfg);/* unit-noise samples per frame         */

/* Upload windows [pairs][P] / [pairs][N+delta], channels [n_channels][L][2] and SNR points
 * [n_snr] (dB) to `device` and select the kernel.  frames_per_cell / frame_offset of cfg are
 * ignored here (given per launch).  A frame whose LDS image exceeds 160 KiB is WOFDM_E_UNSUPPORTED
 * (n_fft = 1024 with 16 symbols near cp + cs = 48).  Just below that limit the kernel class can change
 * with the stride: the matrix-pipe kernels with one symbol per wave pad their LDS rows to multiples of
 * four samples, and where only the padding overflows the plan runs the one-symbol VALU kernel instead
 * (same results, lower rate; wofdm_plan_kernel_id reports layout 1). */
int wofdm_plan_create(wofdm_plan **plan, const wofdm_cfg *cfg, int device,
                      const float *w_tx, const float *w_rx, const float *h,
                      const float *snr_db);
int wofdm_plan_destroy(wofdm_plan *plan);

/* Asynchronous launch on `stream` (a hipStream_t, NULL = default stream): simulate frames
 * [frame_offset, frame_offset+frames_per_cell) of every cell with the on-device Philox4x32-10
 * streams and add into counts_dev[cells][4] (uint64, device memory of the plan's GPU).
 * EXCLUSIVE USE OF THE DEVICE while a launch is in flight.  The default kernels (transforms on the matrix
 * pipe, every N) issue MFMAs in a rhythm that, on MI355X, was MEASURED to corrupt op_sel-swizzled packed fp32
 * arithmetic (v_pk_*_f32 with an op_sel source swizzle) of OTHER waves on the same SIMD (DESIGN.md section 4,
 * hazards 1 and 4: microbenchmarks of this repository, asserted in its GPU tests; no vendor erratum is known to
 * us -- unconfirmed outside these measurements).  They contain no such instruction themselves.  What the library
 * does: every launch waits (on the device, through an event) for the previous launch this process made on that
 * GPU, whatever plan or stream; the synchronous entry points that run other kernels (wofdm_interference,
 * wofdm_tx_psd, wofdm_tx_psd_batch) hold the same gate.  What the CALLER must ensure: no kernel of its own (other libraries, other
 * streams) and no other process runs on the device while a frame launch is in flight -- one process per GPU,
 * synchronise before handing the GPU to other work (bench.py, distributed.py do).  Where that cannot be
 * guaranteed (a shared GPU), select the VALU transforms, wofdm_plan_set_option(plan, WOFDM_OPT_DFT_VALU, 1): those
 * kernels issue only single, cache-line-aligned six-MFMA chains, the shape measured to be harmless. */
int wofdm_plan_launch(wofdm_plan *plan, uint64_t frame_offset, uint64_t frames_per_cell,
                      uint64_t *counts_dev, void *stream);

/* Same, bracketed by HIP events on `stream`; blocks until the kernel finished and returns
 * its duration in milliseconds. */
int wofdm_plan_launch_timed(wofdm_plan *plan, uint64_t frame_offset, uint64_t frames_per_cell,
                            uint64_t *counts_dev, void *stream, float *kernel_ms);

/* Injected randomness, device buffers: labels_dev[cells][frames][S][N] (uint8),
 * unit_noise_dev[cells][frames][noise_len][2] (float, N(0,1) per component). */
int wofdm_plan_launch_injected(wofdm_plan *plan, uint64_t frames_per_cell,
                               const uint8_t *labels_dev, const float *unit_noise_dev,
                               uint64_t *counts_dev, void *stream);

/* Run ONE frame of `cell` on the GPU and copy its intermediate stages to host buffers.
 * labels / unit_noise: host arrays to inject, or NULL to use the Philox streams of
 * (seed, cell, frame).  counts[4] (host) accumulated into. */
int wofdm_plan_dump_frame(wofdm_plan *plan, uint32_t cell, uint64_t frame,
                          const uint8_t *labels, const float *unit_noise,
                          uint64_t *counts, wofdm_dump *out);

/* Subcarrier allocation: active[n_fft] (host), non-zero = bin n carries data.  Unloaded bins
 * transmit zero and are left out of the channel estimate and of all four counters, which then
 * count (S-1) * n_active subcarriers per frame.  NULL restores "every bin loaded".  Replaces the
 * zero-padding `symbolsInOFDM = [zeros(S,offset) transmittedSymbols zeros(S,offset)]` + ifftshift of
 * matlab/main_channel_mask.m:387-390 and the `offset+1:end-offset` selections of 367-369 (there:
 * bins [0,N/4) and [3N/4,N)); also the guard-band `subcar_alloc_mat` of
 * python/ofdm_utils/timefreq_simulation.py:223-233.  The data-bit stream keeps one slot per bin.
 * Synchronises the device; do not call while launches of this plan are in flight elsewhere. */
int wofdm_plan_set_allocation(wofdm_plan *plan, const uint8_t *active);

/* Per-symbol spectral Tx mask: mask[2P-1] (host), DFT-domain gains in natural bin order, P =
 * n_fft+cp+cs.  Every windowed symbol is zero-padded to 2P-1 samples, its DFT multiplied by the
 * mask and transformed back; the first P samples replace the symbol, the remaining P-1 are added
 * to the first P-1 samples of the NEXT symbol's row before the overlap-add (the last symbol's
 * spill is dropped).  Replaces `dft_rc_filt` (matlab/main_channel_mask.m:398-417; its mask is
 * `ifftshift(gen_raised_cosine(floor((2P-1)/2), rollOff, 2P-1))`, 402-405, 443-458).  Needs
 * n_fft <= 512 (the mask's impulse response is staged in LDS), else WOFDM_E_UNSUPPORTED.  NULL
 * removes the mask.  Synchronises the device. */
int wofdm_plan_set_tx_mask(wofdm_plan *plan, const float *mask);

/* Health of the plan's finished launches (call after synchronising the stream; copies one
 * word back): WOFDM_OK, or WOFDM_E_HIP if a kernel reported that a wave gave up waiting for its
 * workgroup -- the counters of that plan are then not to be used.  The synchronous entry points
 * (wofdm_run, wofdm_run_injected, wofdm_plan_launch_timed) check it themselves. */
int wofdm_plan_status(wofdm_plan *plan);

/* Kernel resource facts of the plan: {waves per workgroup, LDS bytes per workgroup,
 * workgroups launched, workgroups resident per CU (occupancy API, capped by the LDS allocation units: DESIGN.md section 3), CUs}. */
int wofdm_plan_info(wofdm_plan *plan, int32_t info[5]);

/* Which instantiation of the frame kernel the plan launches: {layout id, variant}.  Layout: 1, 2 =
 * one / two symbols per wave with the FIR on the VALU; 4, 5 = four symbols per wave (N = 256), FIR on
 * the VALU; 6, 7 = the same with the FIR on the matrix pipe; 9 = one symbol per wave with the FIR on the matrix pipe (Tx-mask
 * variants); 10, 11 = 6, 7 with both 256-point transforms on
 * the matrix pipe as well; 8 = one symbol per wave (N >= 512), FIR on the matrix pipe; 12 = 8 with both transforms on the
 * matrix pipe; 13, 14 = N = 64 / 128, sixteen / eight symbols per wave, FIR and transforms on the matrix pipe; 16 = 13 with a run-time
 * number of symbols per wave and a partly filled last wave (no_symbols not a multiple of 16 / 8, long strides); 15 = 9 at N = 256 with
 * the fast-convolution Tx mask: the symbol's transforms and the mask's two 1024-point transforms on the matrix pipe as well.  Variant: 0 plain, 1 subcarrier allocation, 2 / 3 = Tx mask in direct / fast-
 * convolution form.  (Test and profiling aid; the results do not depend on it beyond fp32 rounding.) */
int wofdm_plan_kernel_id(wofdm_plan *plan, int32_t id[2]);

/* Built geometries.  For the seven structures at n_fft = 256, cp = 32 with the reference's tails, 16 symbols per frame, 21 taps and
 * noise_before_truncate = 1 (ids 1 ... 7: wtx, wrx, WOLA, CPW, CPwtx, CPwrx, CP) the library holds a second build of the plain
 * generate-mode kernel with the structure lengths as compile-time constants; a plain plan of such a geometry launches it (layouts
 * 10 and 11; the counters are the same, bit for bit).  wofdm_plan_kernel_geo: *id = the id of the built geometry of the kernel that
 * wofdm_plan_launch runs, 0 = geometry at run time (any other geometry, allocation and Tx-mask plans, the injected and instrumented
 * entry points, WOFDM_OPT_GENERIC_GEOMETRY); wofdm_plan_kernel_id does not depend on it.  wofdm_cfg_geo_id: the id of cfg's
 * geometry (every length equal to a built one's), 0 if none, a negative error for an invalid cfg; host only, no device needed. */
int wofdm_plan_kernel_geo(wofdm_plan *plan, int32_t *id);
int wofdm_cfg_geo_id(const wofdm_cfg *cfg);

/* Diagnostic choice among the kernels of the family (A/B measurements and the tests; the results do not depend
 * on it beyond fp32 rounding, the defaults are the fastest kernels).  Takes effect for the launches that follow;
 * returns WOFDM_E_UNSUPPORTED -- and leaves the plan as it was -- when no kernel fits the geometry under the option.
 *   WOFDM_OPT_FIR_VALU       1 = the 21-tap FIR (conv, main_BER_calculation.m:260) on the VALU in every layout
 *                            (round-1 kernels) instead of the matrix pipe; 0 = default
 *   WOFDM_OPT_MAX_SPW        at most 1, 2 or 4 OFDM symbols per wavefront; 0 = default (the most that fits)
 *   WOFDM_OPT_TXMASK_DIRECT  1 = the Tx mask (wofdm_plan_set_tx_mask) always as a direct-form convolution instead
 *                            of fast convolution where that fits; 0 = default
 *   WOFDM_OPT_DFT_VALU       1 = the 256-point IDFT / DFT (dftmtx, main_BER_calculation.m:306, 370) as in-register radix-16
 *                            stages on the VALU (layouts 6, 7) instead of split-f16 products on the matrix pipe (layouts
 *                            10, 11); likewise n_fft = 512, 1024 (8 instead of 12), 64, 128 (2 instead of 13, 14, 16) and the Tx-mask
 *                            kernel at n_fft = 256 (9 instead of 15); 0 = default
 *   WOFDM_OPT_GENERIC_GEOMETRY 1 = the kernel that reads the structure lengths at run time also where the geometry is a built one
 *                            (wofdm_plan_kernel_geo then reports 0; identical results); 0 = default */
#define WOFDM_OPT_FIR_VALU       0
#define WOFDM_OPT_MAX_SPW        1
#define WOFDM_OPT_TXMASK_DIRECT  2
#define WOFDM_OPT_DFT_VALU       3
#define WOFDM_OPT_GENERIC_GEOMETRY 4
int wofdm_plan_set_option(wofdm_plan *plan, int32_t option, int32_t value);

/* One-shot, host pointers in / host counters out (synchronous):
 * counts[pairs][n_snr][n_channels][4] accumulated into. */
int wofdm_run(const wofdm_cfg *cfg, int device, const float *w_tx, const float *w_rx,
              const float *h, const float *snr_db, uint64_t *counts);
int wofdm_run_injected(const wofdm_cfg *cfg, int device, const float *w_tx, const float *w_rx,
                       const float *h, const float *snr_db, const uint8_t *labels,
                       const float *unit_noise, uint64_t *counts);

/* Closed-form ICI + ISI power per subcarrier of the structure in cfg, for every (window pair, channel):
 * power[pairs][n_channels][n_fft] (host, float) = sum_{n' != n} |A_0[n,n']|^2 + sum_{n'} |A_1[n,n']|^2 with
 * A_m = W K P V_rx R H_m V_tx Gamma W^-1.  Replaces calculate_interference
 * (matlab/main_interference_calculation.m:177-225; its scalar is the sum over n) and interf_power
 * (python/ofdm_utils/interf_calc.py:20-113; its np.diag(PISI + PICI1) is power[0][0][:]).  Uses n_fft, cp,
 * cs, tail_tx, tail_rx, prefix_rm, circ_shift, n_taps, n_channels, n_window_pairs of cfg.
 * Synchronous; host pointers. */
int wofdm_interference(const wofdm_cfg *cfg, int device, const float *w_tx, const float *w_rx,
                       const float *h, float *power);

/* The same closed form for the system of main_channel_mask.m: only the bins flagged in active[n_fft] carry data
 * (zero padding + ifftshift, matlab/main_channel_mask.m:387-390; NULL = every bin loaded) and every windowed symbol
 * passes the spectral Tx mask tx_mask[2P-1] (dft_rc_filt, main_channel_mask.m:398-417; the semantics of
 * wofdm_plan_set_tx_mask; NULL = no mask), inside calculate_interference (matlab/main_interference_calculation.m:177-225).
 * The mask's spill into the next symbol's row lengthens the on-air pulse of a symbol to B + P - 1 samples, so three
 * symbol periods carry energy: power[pairs][n_channels][n_fft] = sum_{n' != n} |A_0[n,n']|^2 + sum_{m=1,2} sum_{n'}
 * |A_m[n,n']|^2 over the loaded bins n' and wanted[pairs][n_channels][n_fft] (or NULL) = |A_0[n,n]|^2, which the mask
 * attenuates too; both are 0 on unloaded bins n.  The masked pulses are formed on the device once per window pair, not
 * per channel (they take pairs * n_fft * (B + P - 1) complex samples of device memory); the mask's impulse response is
 * prepared once per call (host, double precision, stored in single).  Uses the cfg fields wofdm_interference uses,
 * every n_fft in {64, 128, 256, 512, 1024}, under the same geometry limits and no further one: cp + cs - tail_tx <= 64,
 * tail_tx <= 16, tail_rx <= 64, n_taps <= 21, and cp + cs <= 64 at n_fft = 1024 -- within them the pulse with the
 * channel always ends inside the three periods; outside them, or with more than 65535 window pairs,
 * WOFDM_E_UNSUPPORTED.  Non-finite gains or an allocation without a loaded bin are WOFDM_E_INVALID.  Every argument is
 * checked before the device is touched, and a failed call leaves power and wanted as they were.  With active == NULL and
 * tx_mask == NULL power holds the bits wofdm_interference gives; every sum is formed in a fixed order: repeated
 * calls give identical results.  Synchronous; host pointers; holds the same gate as wofdm_interference from its device
 * synchronisation to the end of its kernels. */
int wofdm_interference_masked(const wofdm_cfg *cfg, int device, const float *w_tx, const float *w_rx,
                              const float *h, const uint8_t *active /* [n_fft] or NULL */,
                              const float *tx_mask /* [2P-1] or NULL */,
                              float *power  /* [pairs][n_channels][n_fft] */,
                              float *wanted /* same shape, or NULL */);

/* Tx-side spectrum estimate: the waveform of no_symbols consecutive symbols X[no_symbols][n_fft][2] (host,
 * complex values on the bins, zeros on unloaded ones) through IDFT, CP/CS copy, Tx window w_tx[P] and the
 * overlap-add of `overlap` tail samples (tail_tx for the Tx-windowed structures, 0 otherwise), then the sum
 * over consecutive slices of 8 n_fft samples (zero-padded remainder included) of |FFT|^2, fftshift-ed:
 * psd[8 n_fft] (host).  Replaces the Tx chain and psd_estimate of wOFDMSystem.estimate_obr
 * (python/ofdm_utils/timefreq_simulation.py:242-258, 101-123); the caller divides by the reference's slice
 * count (full slices + 1).  Uses n_fft, cp, cs of cfg; n_fft in {64, 128, 256}.  Synchronous. */
int wofdm_tx_psd(const wofdm_cfg *cfg, int device, const float *w_tx, const float *X, int no_symbols,
                 int overlap, float *psd);

/* The same estimate for a batch of jobs in one call, n_fft in {64, 128, 256, 512, 1024} (transform length
 * 8 n_fft up to 8192).  Job j transmits symbol block jobs[j].block of X[n_blocks][no_symbols][n_fft][2] (host)
 * with its own cp, cs (P_j = n_fft + cp + cs), overlap (0 <= 2 overlap <= P_j) and Tx window; w_tx holds the
 * jobs' windows concatenated (P_0 values, then P_1, ...).  psd[n_jobs][8 n_fft] (host): per job the undivided
 * slice sums, fftshift-ed, as wofdm_tx_psd (the caller divides by full slices + 1).  The sums are formed in a
 * fixed order: repeated calls give identical results.  Synchronous; holds the gate of the entry points above. */
typedef struct wofdm_psd_job {
    int32_t block;            /* symbol block of X this job transmits */
    int32_t cp, cs;           /* P_j = n_fft + cp + cs */
    int32_t overlap;          /* overlapping tail samples: tail_tx or 0 */
} wofdm_psd_job;
int wofdm_tx_psd_batch(int32_t n_fft, int device, int32_t n_jobs, const wofdm_psd_job *jobs,
                       const float *w_tx, int32_t n_blocks, int32_t no_symbols, const float *X,
                       float *psd);

/* wofdm_tx_psd_batch with an optional spectral Tx mask per job (dft_rc_filt, main_channel_mask.m:398-417;
 * semantics of wofdm_plan_set_tx_mask).  job_mask[n_jobs]: index into the mask table, or -1 = job unmasked
 * (NULL = all unmasked).  mask_len[n_masks]: 2 P - 1 of the jobs that use the mask (checked against every such
 * job); mask_gain: the tables' real DFT-domain gains, natural bin order, concatenated.
 * A masked job's windowed symbols are each zero-padded to 2 P - 1 samples, multiplied by the gains in the DFT
 * domain and transformed back; the first P samples replace the symbol, the other P - 1 are added to the first
 * P - 1 samples of the next symbol's row (the first symbol receives no spill, the last one's is dropped); then
 * the overlap-add and the periodogram as for an unmasked job.  The mask runs as fast convolution over 8 n_fft
 * points, so a masked job needs 3 P - 2 <= 8 n_fft (every cp + cs <= n_fft / 2 fits), else WOFDM_E_UNSUPPORTED;
 * non-finite gains, a job_mask entry outside [-1, n_masks) or a mask_len other than 2 P_j - 1 are
 * WOFDM_E_INVALID.  Each mask in use is prepared once per call (host, double precision; its spectrum is stored
 * in single precision), and a masked job keeps no_symbols (2 P - 1) filtered samples in device memory.  An unmasked
 * job gives the bits wofdm_tx_psd_batch gives for it; every sum is formed in a fixed order: repeated calls give
 * identical results.  Synchronous; holds the same gate as wofdm_tx_psd_batch from its device synchronisation to
 * the end of its kernels. */
int wofdm_tx_psd_batch_masked(int32_t n_fft, int device, int32_t n_jobs, const wofdm_psd_job *jobs,
                              const float *w_tx, int32_t n_masks, const int32_t *mask_len,
                              const float *mask_gain, const int32_t *job_mask,
                              int32_t n_blocks, int32_t no_symbols, const float *X, float *psd);

/* The transmitter's last stage, a memoryless power amplifier (wofdm_rx_profile_pa, wofdm_tx_psd_batch_pa).  It compresses the
 * peaks wofdm_tx_papr counts: that raises the error vector on every loaded bin and puts back, as spectral regrowth, the
 * out-of-band radiation the Tx window and the mask removed.  With r = |x| and rho = r / a_sat the output is y = g x; the phase
 * is untouched (AM/AM only, no AM/PM).
 *   WOFDM_PA_LINEAR  y = x, no arithmetic at all
 *   WOFDM_PA_RAPP    AM/AM of a solid-state amplifier, smoothness p = smooth: g = (1 + rho^(2p))^(-1/(2p)), evaluated above rho =
 *                    1 as (1 / rho) (1 + rho^(-2p))^(-1/(2p)), so that no finite input overflows; g = 1 at r = 0
 *   WOFDM_PA_CLIP    the soft limiter, the p -> infinity limit: g = 1 for rho <= 1, else 1 / rho
 * a_sat^2 = ref_power 10^(ibo_db / 10): the input back-off counts from a reference power, which the two routes take a little
 * differently -- wofdm_rx_profile_pa gets it from the caller per window pair (rx_profile.pa_ref_power: the mean over the symbol
 * periods, the mean the PAPR histogram's axis counts from), wofdm_tx_psd_batch_pa measures it on the device over a job's whole
 * waveform, the last ramp-down included.  The kernels evaluate g in single precision (hardware log2 / exp2), one device
 * function for both routes; rx_profile.pa_gain is the double-precision mirror.
 *   Limits, both routes.  WOFDM_E_UNSUPPORTED: smooth outside [0.5, 16] for the Rapp model (the other two ignore it), ibo_db
 * outside [-40, 60], a model other than the three, more than WOFDM_PA_MAX_POINTS points; WOFDM_E_INVALID: a non-finite
 * ibo_db or smooth, reserved != 0. */
#define WOFDM_PA_LINEAR 0
#define WOFDM_PA_RAPP   1
#define WOFDM_PA_CLIP   2
#define WOFDM_PA_MAX_POINTS 16
typedef struct wofdm_pa_point {
    int32_t model;
    float   ibo_db;    /* input back-off: a_sat^2 = ref_power 10^(ibo_db / 10) */
    float   smooth;    /* p of the Rapp model; ignored by the other two */
    int32_t reserved;  /* 0 */
} wofdm_pa_point;

/* wofdm_tx_psd_batch_masked behind the amplifier: spectral regrowth.  pa[n_pa] is a table of amplifiers, job_pa[n_jobs] the
 * index of a job's, or -1 = none (NULL = none anywhere).  A job's reference power is the mean of |x|^2 over all len = overlap +
 * no_symbols (P - overlap) samples of its own finished waveform -- window, mask and overlap-add done, the last ramp-down
 * included --, summed on the device in a fixed order; a_sat is formed from it in double precision and stored in single.  One
 * elementwise kernel, and the reduction in front of it, run between the waveform kernels and the periodogram.  job_power
 * [n_jobs][2] (or NULL): the mean power of a job's waveform before and behind its amplifier (equal without one).  A job
 * without power passes through unchanged.  A job with job_pa = -1, or with a WOFDM_PA_LINEAR point, gives the bits
 * wofdm_tx_psd_batch_masked gives for it; repeated calls give identical bits.  Every check of wofdm_tx_psd_batch_masked
 * applies, and the amplifier's limits above; WOFDM_E_INVALID: n_pa < 0, NULL pa with n_pa > 0, a job_pa entry outside
 * [-1, n_pa).  Every argument is checked before the device is touched. */
int wofdm_tx_psd_batch_pa(int32_t n_fft, int device, int32_t n_jobs, const wofdm_psd_job *jobs,
                          const float *w_tx, int32_t n_masks, const int32_t *mask_len,
                          const float *mask_gain, const int32_t *job_mask,
                          int32_t n_pa, const wofdm_pa_point *pa, const int32_t *job_pa,
                          int32_t n_blocks, int32_t no_symbols, const float *X, float *psd,
                          float *job_power);                 /* [n_jobs][2] = {mean |x|^2, mean |y|^2}, or NULL */

/* Peak-to-average power ratio (PAPR) of the on-air frames, per symbol period, as a histogram -- for exactly the frames the
 * BER loop transmits.  The reference has no PAPR figure: this entry point replaces no line of it; it completes the
 * window / Tx-mask study beside the BER, interference and spectrum entry points above.
 *   Frames: window pair p transmits the frames [frame_offset, frame_offset + frames_per_cell) of cell = p as a plan with
 * n_snr = n_channels = 1 draws them (label stream of philox.h, all 64 bits of seed and of the frame index; MATLAB Gray QAM at
 * bits_per_sc bits; symbol 0, the pilot, is an ordinary random symbol), with the allocation active[n_fft] (semantics of
 * wofdm_plan_set_allocation; NULL = every bin loaded) and the spectral Tx mask tx_mask[2P-1] (semantics of
 * wofdm_plan_set_tx_mask: no spill into symbol 0, the last symbol's spill dropped; NULL = no mask): IDFT, CP/CS copy, Tx
 * window w_tx[pairs][P], mask, overlap-add of the tail_tx tail samples -- tx[tail_tx + S B], B = P - tail_tx.
 *   Periods: symbol period s = 0 .. S-1 is tx[s B, (s + 1) B); the trailing tail_tx samples (the last symbol's ramp-down)
 * belong to no period.  peak = max |tx|^2 and energy = sum |tx|^2 over the period, PAPR = B peak / energy (linear), and
 *   bin = clamp(floor((10 log10(PAPR) - lo_db) / step_db), 0, n_bins - 1):
 * values outside the range land in the end bins; a period without energy counts in bin 0 and takes no part in the maximum.
 *   Outputs (host): hist[pairs][n_bins] is ACCUMULATED into; max_papr[pairs] (or NULL) becomes max(old, largest PAPR of the
 * call); periods[pairs][frames_per_cell][S][2] = {peak, energy} (or NULL) is a test and diagnostic aid, refused with
 * WOFDM_E_UNSUPPORTED above WOFDM_TX_PAPR_MAX_PERIODS periods in total.  Counts are integers and max_papr a maximum: neither
 * depends on the order of the additions, and {peak, energy} are reduced in a fixed order -- repeated calls give identical
 * results, and a frame range split over several calls gives the histogram of one call.
 *   Uses n_fft, bits_per_sc, syms_per_frame, cp, cs, tail_tx, n_window_pairs, seed, frame_offset, frames_per_cell of cfg and
 * nothing else.  n_fft in {64, 128, 256, 512, 1024}, S in 2 .. 16, k in {2, 4, 6}, cp, cs <= n_fft, 2 tail_tx <= P; with a
 * mask 3 P - 2 <= 8 n_fft as for wofdm_tx_psd_batch_masked (the mask runs as fast convolution over 8 n_fft points) -- so
 * n_fft = 1024 is served here although the BER kernels' mask stops at 512; n_bins <= 8192; fewer than 2^28 pairs.  Outside:
 * WOFDM_E_UNSUPPORTED.  WOFDM_E_INVALID: NULL cfg, w_tx or hist, n_bins < 1, step_db not positive or not finite, lo_db not
 * finite, non-finite mask gains, an allocation without a loaded bin.  Every argument is checked before the device is
 * touched, and a failed call leaves hist, max_papr and periods as they were.
 *   Device memory is bounded whatever frames_per_cell is: the (pair, frame) items, pair-major, are processed in chunks of
 *     min(65535, WOFDM_TX_PAPR_CHUNK_BYTES / (8 (S n_fft + T + [mask] S (2P-1))))  frames, T = tail_tx + S B
 * -- symbol grid, waveform and (masked) filtered symbols of a frame in single-precision complex -- plus 64 bytes of job
 * tables per frame, the windows, pairs * n_bins counters and, if asked for, periods.  The mask's spectrum is prepared once per
 * call (host, double precision, stored in single).  Synchronous; host pointers; holds the same gate as the other synchronous
 * entry points from its device synchronisation to the end of its kernels. */
#define WOFDM_TX_PAPR_CHUNK_BYTES (256u << 20)
#define WOFDM_TX_PAPR_MAX_PERIODS (1 << 20)
int wofdm_tx_papr(const wofdm_cfg *cfg, int device,
                  const float *w_tx,        /* [pairs][P] */
                  const uint8_t *active,    /* [n_fft] or NULL */
                  const float *tx_mask,     /* [2P-1] or NULL */
                  float lo_db, float step_db, int32_t n_bins,
                  uint64_t *hist,           /* [pairs][n_bins], ACCUMULATED into */
                  float *max_papr,          /* [pairs], linear; max(old, new); or NULL */
                  float *periods);          /* [pairs][frames][S][2] = {peak, energy}, or NULL */

/* *ms = milliseconds (HIP events) the kernels of the calling thread's last successful wofdm_tx_papr call took, first chunk
 * to last; 0 before any.  Measurement aid (tools/bench_tx_papr.py). */
int wofdm_tx_papr_kernel_ms(float *ms);

/* Per-subcarrier error profile of the frames the BER loop runs: where in the band the bit errors, the symbol errors and the
 * error-vector power sit.  The call simulates the frames [frame_offset, frame_offset + frames_per_cell) of every cell exactly
 * as a plan draws them (label and noise streams of philox.h, all 64 bits of seed and of the frame index, cell = (pair n_snr +
 * snr) n_channels + channel) through a second, unfused implementation of the frame pipeline: the Tx chain of wofdm_tx_papr
 * (allocation active[n_fft], semantics of wofdm_plan_set_allocation; spectral Tx mask tx_mask[2P-1], semantics of
 * wofdm_plan_set_tx_mask, as fast convolution over 8 n_fft points -- so n_fft = 1024 is served), then per cell conv(channel,
 * .), add_wgn with Ps and Pn measured over the same wofdm_noise_len samples in either noise_before_truncate order, truncation,
 * and per symbol prefix removal, Rx window, fold, circular shift and DFT, the pilot LS estimate H = Y0 / X0 of symbol 0, Xhat
 * = Y_s / H for s >= 1, the hard decision and the comparison with the transmitted labels.  Replaces, per subcarrier instead
 * of per frame, matlab/main_BER_calculation.m:260-272 (with 277-355) and the `offset+1:end-offset` bookkeeping of
 * matlab/main_channel_mask.m:367-369; python/ofdm_utils/wofdm_simulation.py:205-235.  The reference has no per-bin
 * figure.
 *   Outputs (host), ACCUMULATED into: errs[cells][n_fft][2] = {bit errors, symbol errors} and err_power[cells][n_fft] = sum
 * |Xhat - X|^2 (or NULL) over the frames_per_cell (S - 1) decisions a loaded bin takes in the call; unloaded bins receive
 * nothing.  Summed over the bins, errs gives counts[cell][0] and counts[cell][2] of wofdm_plan_launch on the same cfg up to
 * decisions that fp32 rounding tips (the kernels share no transform, FIR or slicer code with the frame kernels).  Integer
 * counts do not depend on the order of additions, and every float sum is formed in a fixed order -- per frame over the
 * symbols and waves in order, fp32; over the frames of a cell in frame order, fp64 -- so repeated calls give identical
 * results, and a frame range split over several calls gives the integer counters of one call.
 *   Limits: n_fft in {64, 128, 256, 512, 1024}, S in 2 .. 16, k in {2, 4, 6}, n_taps <= 21, tail_rx even and <= 64, n_fft +
 * tail_rx + prefix_rm == P - tail_tx, cp, cs <= n_fft, 2 tail_tx <= P, with a mask 3 P - 2 <= 8 n_fft, fewer than 2^28
 * cells; outside: WOFDM_E_UNSUPPORTED.  No frame image lives in LDS, so the 160 KiB limit of wofdm_plan_create does not
 * apply.  WOFDM_E_INVALID: a NULL cfg, w_tx, w_rx, h, snr_db or errs, counts below 1, negative lengths, non-finite windows,
 * taps, SNR points or mask gains, an allocation without a loaded bin.  Every argument is checked before the device is
 * touched, and a failed call leaves errs and err_power as they were.
 *   Device memory is bounded whatever frames_per_cell is: the (cell, frame) items, cell-major, are processed in chunks of
 *     min(65535, WOFDM_RX_PROFILE_CHUNK_BYTES / (8 (S n_fft + T + [mask] S (2P-1) + n_fft)))  frames, T = tail_tx + S B
 * -- symbol grid, waveform, (masked) filtered symbols and the per-bin partial sums of a frame -- plus 64 bytes of job tables
 * per frame, the windows, taps and 24 bytes per (cell, bin) of totals.  Synchronous; host pointers; holds the same gate as the
 * other synchronous entry points from its device synchronisation to the end of its kernels.  This is a diagnostic route,
 * not the hot path: a workgroup per frame, no matrix-pipe arithmetic. */
#define WOFDM_RX_PROFILE_CHUNK_BYTES (256u << 20)
int wofdm_rx_profile(const wofdm_cfg *cfg, int device,
                     const float *w_tx,      /* [pairs][P] */
                     const float *w_rx,      /* [pairs][N+tail_rx] */
                     const float *h,         /* [n_channels][n_taps][2] */
                     const float *snr_db,    /* [n_snr] */
                     const uint8_t *active,  /* [n_fft] or NULL */
                     const float *tx_mask,   /* [2P-1] or NULL */
                     uint64_t *errs,         /* [cells][n_fft][2] = {bit errors, symbol errors}, ACCUMULATED into */
                     double *err_power);     /* [cells][n_fft] = sum |Xhat - X|^2, ACCUMULATED into; or NULL */

/* wofdm_rx_profile beside an asynchronous adjacent-band neighbour: what the victim of wofdm_rx_profile loses, bin by bin, to a
 * second transmitter that is not symbol-aligned with it -- the interference the Rx window is there to reject.  The reference
 * has no such experiment (matlab/main_channel_mask.m frees half the band for a neighbour and stops at the transmitter).
 *   Victim: exactly wofdm_rx_profile -- frames, cells, streams 0 and 1, allocation, mask, both noise_before_truncate orders,
 * outputs, ordered sums, the gate.
 *   Neighbour: the victim's numerology and Tx chain (cfg, k, the Tx window of the cell's pair, the same tx_mask or none) on the
 * allocation aci_active[n_fft] (any set; usually the complement of active), with labels of its own: stream 2 of philox.h
 * (WOFDM_STREAM_ACI), counter (u bps + blk, frame lo, frame hi, 2 << 28 | cell), key and slot layout of stream 0.  It sends S + 1
 * symbols u = 0 ... S, a waveform xi of tail_tx + (S + 1) B samples, placed so that its symbol u begins at victim time
 * (u - 1) B + aci_delay, 0 <= aci_delay < B: the on-air sample t of the victim's frame carries a xi[t + B - aci_delay] with a
 * = 10^(aci_level_db / 20), an index inside xi for every t of the frame, so the frame has a neighbour from its first sample
 * (pilot included) to its last; what the neighbour sent before t = 0 passes its channel like the rest.  Its channel is
 * aci_h[channel of the cell] ([n_channels][n_taps][2]), or the victim's h[channel] if aci_h is NULL.
 *   Received: r = conv(h, x) + conv(aci_h, a xi shifted) + g n.  Ps, Pn and so g are measured on the victim's conv alone, over
 * the samples wofdm_rx_profile uses: snr_db stays the victim's SNR and the neighbour comes on top.  Outputs: errs and err_power
 * on the victim's loaded bins, ACCUMULATED into, as in wofdm_rx_profile.
 *   An aci_active that loads no bin is valid and means no neighbour: the call then IS wofdm_rx_profile (same kernels, same
 * chunks, same bits).  WOFDM_E_INVALID: a NULL aci_active, a non-finite aci_level_db (or one whose amplitude overflows single
 * precision), non-finite aci_h taps, a negative aci_delay; WOFDM_E_UNSUPPORTED: aci_delay >= B = P - tail_tx; and every limit
 * and check of wofdm_rx_profile.  Every argument is checked before the device is touched; a failed call leaves errs and
 * err_power as they were.  Repeated calls give identical bits, a split frame range the integer counters of one call.
 *   Chunks: min(65535, WOFDM_RX_PROFILE_CHUNK_BYTES / (8 (S n_fft + (S + 1) n_fft + T + (T + B) + [mask] (2 S + 1) (2P-1) +
 * n_fft)))  frames -- both symbol grids, both waveforms, (masked) both sets of filtered symbols, the per-bin partials. */
int wofdm_rx_profile_aci(const wofdm_cfg *cfg, int device,
                         const float *w_tx,           /* [pairs][P] */
                         const float *w_rx,           /* [pairs][N+tail_rx] */
                         const float *h,              /* [n_channels][n_taps][2] */
                         const float *snr_db,         /* [n_snr] */
                         const uint8_t *active,       /* [n_fft] or NULL */
                         const float *tx_mask,        /* [2P-1] or NULL */
                         const uint8_t *aci_active,   /* [n_fft] bins the neighbour loads */
                         const float *aci_h,          /* [n_channels][n_taps][2]; NULL = the victim's h */
                         int32_t aci_delay,           /* samples, 0 <= aci_delay < B */
                         float aci_level_db,          /* dB; neighbour amplitude 10^(level/20), finite */
                         uint64_t *errs,              /* [cells][n_fft][2], ACCUMULATED into */
                         double *err_power);          /* [cells][n_fft], ACCUMULATED into; or NULL */

/* *ms = milliseconds (HIP events) the kernels of the calling thread's last successful wofdm_rx_profile or
 * wofdm_rx_profile_aci call took (whichever came last), first chunk to last; 0 before any.  Measurement aid
 * (tools/bench_rx_profile.py, tools/bench_rx_profile_aci.py).  A successful wofdm_rx_profile_sync call (below) counts as
 * such a call too: the figure is then that of its whole sweep (tools/bench_rx_profile_sync.py); so does a successful
 * wofdm_rx_profile_doppler call, with all its tracks (tools/bench_rx_profile_doppler.py), and a successful
 * wofdm_rx_profile_pa call, with all its points (tools/bench_rx_profile_pa.py), and a successful wofdm_rx_profile_pn call,
 * with its walk and all its points (tools/bench_rx_profile_pn.py). */
int wofdm_rx_profile_kernel_ms(float *ms);

/* wofdm_rx_profile under receiver timing and carrier-frequency offset: what the victim of wofdm_rx_profile loses, bin by bin
 * and symbol by symbol, when the receiver's windows begin early or late and its oscillator is off -- the tolerance the cyclic
 * suffix, the prefix removal and the Rx window trade.  The reference has no such experiment: its receiver is synchronised.  A
 * call takes a LIST of points and runs the Tx chain and the power pass once per frame, whatever n_points is.
 *   Victim: exactly wofdm_rx_profile -- frames, cells, streams 0 and 1, allocation, mask, both noise_before_truncate orders, Ps,
 * Pn and the noise gain g (which never sees the offsets), the gate.
 *   Received signal, for every integer on-air index a: r[a] = conv[a] + g n[a], conv = conv(h, x), zero outside [0, T + L - 1);
 * n[a] the unit normal of stream 1 at sample index a mod 2^32 (block (uint32) a >> 1, word pair a & 1), so negative indices
 * land on counter words no frame uses.  Nothing precedes the frame and nothing follows it: it is alone on the air.
 *   Per point: sample m, 0 <= m < n_fft + tail_rx, of symbol s sits at a = s B + prefix_rm + timing + m and is multiplied, signal
 * and noise, by e^{+2 pi i cfo a / n_fft} (cfo_tracked = 0, a free-running oscillator) or by e^{+2 pi i cfo m / n_fft}
 * (cfo_tracked = 1: the common phase of every symbol removed); then Rx window, fold, shift, DFT, the pilot LS estimate from
 * symbol 0 -- the pilot sees the offsets the data sees --, equaliser and slicer as in wofdm_rx_profile.  With the + sign a
 * positive cfo moves what was sent on bin n - 1 onto bin n.  The phase at the window's start, exp(2 pi i frac(cfo (s B +
 * prefix_rm + timing) / n_fft)), is prepared per (point, symbol) on the host in double precision from cfo as stored and kept
 * in single; the kernel forms only the in-window factor in single precision -- with |cfo| <= 4 its argument stays at a few
 * turns and its rounding near 3e-6 rad, below the 2e-5 stage tolerance: hence the limit on cfo.
 *   Outputs (host), ACCUMULATED into: errs[n_points][cells][n_fft][2] and err_power[n_points][cells][n_fft] (or NULL) per point
 * as in wofdm_rx_profile; sym_errs[n_points][cells][S-1][2] = {bit errors, symbol errors} and sym_power[n_points][cells][S-1] =
 * sum |Xhat - X|^2 (either may be NULL) over the loaded bins per data symbol s = 1 ... S-1 -- the error against the distance
 * from the pilot, the figure a free-running offset needs.  Integer counters are exact; float sums are formed in a fixed order
 * -- per symbol a lane's bins ascending, then the ordered wave sum; per frame in fp32 as in wofdm_rx_profile; over the frames
 * of a cell in frame order, fp64, one addition per frame onto the running total --, so repeated calls give identical bits, a
 * split frame range gives the integer counters of one call, and a point's results do not depend on which other points share
 * its call.  A point with timing = 0 and cfo = 0, under either flag, gives the bits of wofdm_rx_profile, err_power bytes
 * included (as long as no cell's frames are split over two chunks of that call).
 *   Every limit and check of wofdm_rx_profile applies.  WOFDM_E_INVALID: NULL points or errs, n_points < 1, a non-finite cfo,
 * reserved != 0, cfo_tracked other than 0 or 1; WOFDM_E_UNSUPPORTED: n_points > WOFDM_SYNC_MAX_POINTS, |timing| >= B = P -
 * tail_tx, |cfo| > 4.  Every argument is checked before the device is touched; a failed call leaves all four outputs as they were.
 *   Chunks: min(65535, WOFDM_RX_PROFILE_CHUNK_BYTES / (8 (S n_fft + T + [mask] S (2P-1)) + 8 n_points (n_fft + S)))  frames --
 * symbol grid, waveform, (masked) filtered symbols, and per point the per-bin and per-symbol partials.
 *   Measured on an MI355X (tools/bench_rx_profile_sync.py, profiles/rx_profile_sync.txt): 9 timing points on 64 cells x 2000
 * frames x 16 symbols at n_fft = 256 take 98 ms of kernels (134 ms masked), 2.7 (2.0) times one wofdm_rx_profile call on the
 * same cells and frames in the same run -- 0.30 (0.22) of a call per point. */
#define WOFDM_SYNC_MAX_POINTS 64
typedef struct wofdm_sync_point {
    int32_t timing;       /* theta, samples: the receiver's windows begin theta samples late (> 0) or early (< 0) */
    float   cfo;          /* epsilon, in subcarrier spacings */
    int32_t cfo_tracked;  /* 0: free-running oscillator; 1: the common phase of every symbol removed */
    int32_t reserved;     /* 0 */
} wofdm_sync_point;
int wofdm_rx_profile_sync(const wofdm_cfg *cfg, int device,
                          const float *w_tx,                /* [pairs][P] */
                          const float *w_rx,                /* [pairs][N+tail_rx] */
                          const float *h,                   /* [n_channels][n_taps][2] */
                          const float *snr_db,              /* [n_snr] */
                          const uint8_t *active,            /* [n_fft] or NULL */
                          const float *tx_mask,             /* [2P-1] or NULL */
                          int32_t n_points, const wofdm_sync_point *points,
                          uint64_t *errs,                   /* [n_points][cells][n_fft][2], ACCUMULATED into */
                          double *err_power,                /* [n_points][cells][n_fft], or NULL */
                          uint64_t *sym_errs,               /* [n_points][cells][S-1][2], or NULL */
                          double *sym_power);               /* [n_points][cells][S-1], or NULL */

/* wofdm_rx_profile over channels that MOVE within the frame: what the victim of wofdm_rx_profile loses, bin by bin and symbol
 * by symbol, when the taps drift under a receiver that equalises with the pilot of symbol 0 alone -- the mobility the channel
 * generator names (channels.gen_chan_track: Veh-A, 2 GHz, 100 km/h, f_D = 185 Hz), where both the Rx window (ICI rejection)
 * and the distance from the pilot matter.  Every other call here holds one snapshot of the channel for the whole frame.  A call
 * takes a LIST of tracks, typically the same realisations at several speeds, and runs the Tx chain once per frame, whatever
 * n_tracks is; every track sees the same labels and the same noise, so a comparison across tracks is paired.
 *   Victim: exactly wofdm_rx_profile -- frames, cells, streams 0 and 1, allocation, mask, both noise_before_truncate orders, the
 * gate; the noise of on-air sample a is the unit normal the plain kernel uses for it.
 *   Channel: h_track[track][channel][q] is the tap vector at on-air index q knot_step (knot q).  For the receive index a, q =
 * min(a div knot_step, n_knots - 2), f = (a - q knot_step) / knot_step and h_l[a] = K[q][l] + f (K[q+1][l] - K[q][l]) -- in this
 * form, so that equal knots give the knot back exactly --, and conv[a] = sum_l h_l[a] x[a - l], 0 <= a < T + n_taps - 1: the tap
 * is taken at the OUTPUT sample's time.  Ps, Pn and the noise gain g are measured as in wofdm_rx_profile, on this conv, per
 * track.  Rx window, fold, shift, DFT, the pilot LS estimate from symbol 0, equaliser, slicer and counters are unchanged.
 *   Outputs (host), ACCUMULATED into, with the shapes and the ordered sums of wofdm_rx_profile_sync, "track" for "point":
 * errs[n_tracks][cells][n_fft][2], err_power[n_tracks][cells][n_fft] (or NULL), sym_errs[n_tracks][cells][S-1][2] and
 * sym_power[n_tracks][cells][S-1] (either may be NULL).  Integer counters are exact; float sums per frame in fp32 in the sync
 * kernel's order, over the frames of a cell in fp64, one addition per frame --, so repeated calls give identical bits, a split
 * frame range gives the integer counters of one call, and a track's results do not depend on which other tracks share its
 * call.  A track whose knots all equal h[channel] gives the bits of wofdm_rx_profile, err_power bytes included (as long as no
 * cell's frames are split over two chunks of that call).
 *   Every limit and check of wofdm_rx_profile applies.  WOFDM_E_INVALID: NULL h_track or errs, n_tracks < 1, n_knots < 2,
 * knot_step < 1, a non-finite knot, a track that does not cover the frame: (n_knots - 1) knot_step < tail_tx + S B + n_taps - 2;
 * WOFDM_E_UNSUPPORTED: n_tracks > WOFDM_DOPPLER_MAX_TRACKS, n_knots > WOFDM_DOPPLER_MAX_KNOTS.  Every argument is checked
 * before the device is touched; a failed call leaves all four outputs as they were.
 *   Chunks: min(65535, WOFDM_RX_PROFILE_CHUNK_BYTES / (8 (S n_fft + T + [mask] S (2P-1)) + 8 n_tracks (n_fft + S)))  frames --
 * wofdm_rx_profile_sync's formula with the tracks for its points.
 *   A successful call counts for wofdm_rx_profile_kernel_ms.
 *   Measured on an MI355X (tools/bench_rx_profile_doppler.py, profiles/rx_profile_doppler.txt): on 64 cells x 2000 frames x
 * 16 symbols at n_fft = 256 one track takes 41.7 ms of kernels (72.3 ms masked), 1.17 (1.09) times one wofdm_rx_profile call on
 * the same cells and frames in the same run; four tracks take 94.3 (122.1) ms, 2.65 (1.84) times -- 0.49 (0.25) of a plain call
 * per additional track. */
#define WOFDM_DOPPLER_MAX_TRACKS 16
#define WOFDM_DOPPLER_MAX_KNOTS  64
int wofdm_rx_profile_doppler(const wofdm_cfg *cfg, int device,
                             const float *w_tx,             /* [pairs][P] */
                             const float *w_rx,             /* [pairs][N+tail_rx] */
                             const float *h_track,          /* [n_tracks][n_channels][n_knots][n_taps][2] */
                             int32_t n_tracks, int32_t n_knots, int32_t knot_step,
                             const float *snr_db,           /* [n_snr] */
                             const uint8_t *active,         /* [n_fft] or NULL */
                             const float *tx_mask,          /* [2P-1] or NULL */
                             uint64_t *errs,                /* [n_tracks][cells][n_fft][2], ACCUMULATED into */
                             double *err_power,             /* [n_tracks][cells][n_fft], or NULL */
                             uint64_t *sym_errs,            /* [n_tracks][cells][S-1][2], or NULL */
                             double *sym_power);            /* [n_tracks][cells][S-1], or NULL */

/* wofdm_rx_profile behind the power amplifier (wofdm_pa_point above): what the victim of wofdm_rx_profile loses, bin by bin and
 * symbol by symbol, when the transmitter's last stage compresses the peaks of the waveform -- "which window pair is best at 3 dB
 * back-off".  A call takes a LIST of points (model, back-off, smoothness) and runs the Tx chain once per frame, whatever
 * n_points is; every point sees the same labels and the same noise, so back-offs compare pairwise.
 *   Victim: exactly wofdm_rx_profile -- frames, cells, streams 0 and 1, allocation, mask, both noise_before_truncate orders, the
 * gate; the noise of on-air sample a is the unit normal the plain kernel uses for it.
 *   Amplifier: it acts on the finished on-air waveform x[tail_tx + S B] -- after the window, the mask and the overlap-add, the
 * last ramp-down included, before the channel.  Point i of a cell uses a_sat^2 = ref_power[pair of the cell] 10^(ibo_db_i / 10),
 * formed on the host in double precision and stored in single.  The amplified waveforms are materialised per point by a small
 * kernel, which also forms the two power sums of pa_power; a WOFDM_PA_LINEAR point reads the unamplified waveform itself.
 *   Powers: Ps is measured per point on conv(h, y), as wofdm_rx_profile_doppler measures it per track -- snr_db stays the SNR
 * at the receiver, the power the back-off gives away is not charged to the link --, Pn with the first point.  Rx window, fold,
 * shift, DFT, the pilot LS estimate from symbol 0 (the pilot went through the amplifier too), equaliser, slicer and counters
 * are unchanged.
 *   Outputs (host), ACCUMULATED into, with the shapes and the ordered sums of wofdm_rx_profile_sync, "point" on the leading
 * axis: errs[n_points][cells][n_fft][2], err_power[n_points][cells][n_fft] (or NULL), sym_errs[n_points][cells][S-1][2] and
 * sym_power[n_points][cells][S-1] (either may be NULL), and pa_power[n_points][cells][2] = {sum |x|^2, sum |y|^2} over the T =
 * tail_tx + S B samples of the cell's frames (or NULL): per frame in fp32 in a fixed order, over the frames in fp64 in frame
 * order.  Integer counters are exact; float sums per frame in fp32 in the sync kernel's order, over the frames of a cell in
 * fp64, one addition per frame --, so repeated calls give identical bits, a split frame range gives the integer counters of one
 * call, and a point's results do not depend on which other points share its call.  A WOFDM_PA_LINEAR point gives the bits of
 * wofdm_rx_profile, err_power bytes included (as long as no cell's frames are split over two chunks of that call).
 *   Every limit and check of wofdm_rx_profile applies, and the amplifier's limits above.  WOFDM_E_INVALID: NULL points, errs or
 * ref_power, n_points < 1, a ref_power that is not finite and positive.  Every
 * argument is checked before the device is touched; a failed call leaves all five outputs as they were.
 *   Chunks: min(65535, WOFDM_RX_PROFILE_CHUNK_BYTES / (8 (S n_fft + T + [mask] S (2P-1)) + 8 n_points (n_fft + S + T)))  frames --
 * wofdm_rx_profile_sync's formula plus one waveform per point.
 *   A successful call counts for wofdm_rx_profile_kernel_ms.
 *   Measured on an MI355X (tools/bench_rx_profile_pa.py, profiles/rx_profile_pa.txt): on 64 cells x 2000 frames x 16 symbols at
 * n_fft = 256 one point takes 56.5 ms of kernels (88.8 ms masked), 1.44 (1.25) times one wofdm_rx_profile call on the same cells
 * and frames in the same run; four points take 133.6 (152.8) ms, 3.41 (2.15) times -- 0.66 (0.30) of a plain call per
 * additional point. */
int wofdm_rx_profile_pa(const wofdm_cfg *cfg, int device,
                        const float *w_tx,                  /* [pairs][P] */
                        const float *w_rx,                  /* [pairs][N+tail_rx] */
                        const float *h,                     /* [n_channels][n_taps][2] */
                        const float *snr_db,                /* [n_snr] */
                        const uint8_t *active,              /* [n_fft] or NULL */
                        const float *tx_mask,               /* [2P-1] or NULL */
                        int32_t n_points, const wofdm_pa_point *points,
                        const float *ref_power,             /* [pairs]: mean on-air power the back-off counts from */
                        uint64_t *errs,                     /* [n_points][cells][n_fft][2], ACCUMULATED into */
                        double *err_power,                  /* [n_points][cells][n_fft], or NULL */
                        uint64_t *sym_errs,                 /* [n_points][cells][S-1][2], or NULL */
                        double *sym_power,                  /* [n_points][cells][S-1], or NULL */
                        double *pa_power);                  /* [n_points][cells][2], or NULL */

/* wofdm_rx_profile under oscillator PHASE NOISE: what the victim of wofdm_rx_profile loses, bin by bin and symbol by symbol,
 * when the receiver's oscillator phase is a random walk (a Lorentzian line) -- the carrier-frequency offset of
 * wofdm_rx_profile_sync is a deterministic ramp, every other call holds the phase still.  The walk does two things: it turns a
 * whole symbol by a common phase error (CPE), which under the pilot-of-symbol-0 receiver grows with the distance from the
 * pilot -- hence the per-symbol outputs --, and it smears every subcarrier onto its neighbours (ICI), the quantity the Rx
 * window is there to reject.  The reference has no such experiment.  A call takes a LIST of points (linewidth, tracked or
 * not) and runs the Tx chain, the power pass and the walk once per frame, whatever n_points is; every point sees the same
 * labels, the same noise and the same unit walk, so linewidths compare pairwise.
 *   Victim: exactly wofdm_rx_profile -- frames, cells, streams 0 and 1, allocation, mask, both noise_before_truncate orders, Ps,
 * Pn and the noise gain g (which never sees the phase), the gate; the noise of on-air sample a is the unit normal the plain
 * kernel uses for it.
 *   Walk: the increment xi[j] of on-air index j >= 0 of (seed, cell, frame) is one component of a complex unit normal of
 * stream 3 of philox.h: complex index c = j >> 1 from block c >> 1, word pair c & 1 (the layout of the noise of stream 1),
 * counter (c >> 1, frame lo, frame hi, 3 << 28 | cell), key = seed; the real part for even j, the imaginary part for odd j.
 * The two uniforms are formed in single precision as the noise forms them (their values are exact), the Box-Muller step
 * sqrt(-2 ln u1) (cos, sin) 2 pi u2 in double precision.  The unit walk u[a] = xi[0] + ... + xi[a], 0 <= a < S B, is
 * accumulated and kept in double precision on the device, once per frame (a workgroup-wide prefix sum in a fixed order).
 *   Per point: linewidth is beta, the two-sided 3 dB width of the Lorentzian line in subcarrier spacings, 0 <= beta <= 1; the
 * walk's variance per sample is sigma^2 = 2 pi beta / n_fft, and sigma / (2 pi) is formed on the host in double precision from
 * beta as stored.  Sample m, 0 <= m < n_fft + tail_rx, of symbol s sits at a = s B + prefix_rm + m -- the windows of a
 * receiver at timing 0 read exactly the on-air indices [0, S B) -- and is multiplied, signal and noise, before the Rx window
 * by e^{i sigma u[a]} (cpe_tracked = 0, a free-running oscillator) or by e^{i sigma (u[a] - ubar_s)} (cpe_tracked = 1: a
 * genie removes the common phase error), ubar_s the unweighted mean of u over the n_fft + tail_rx samples under the symbol's
 * window, formed in double precision in a fixed order; then Rx window, fold, shift, DFT, the pilot LS estimate from symbol 0
 * -- the pilot sees what the data sees --, equaliser and slicer as in wofdm_rx_profile.  The phase is reduced in double
 * precision, t = (sigma / 2 pi) u less its nearest integer, and only then rounded to single for the sine and cosine: the
 * rotation is good to about 2e-7 rad for every beta and n_fft, an order below the in-window factor of wofdm_rx_profile_sync,
 * so there is no limit of the |cfo| <= 4 kind.
 *   Outputs (host), ACCUMULATED into, with the shapes and the ordered sums of wofdm_rx_profile_sync, "point" on the leading
 * axis: errs[n_points][cells][n_fft][2], err_power[n_points][cells][n_fft] (or NULL), sym_errs[n_points][cells][S-1][2] and
 * sym_power[n_points][cells][S-1] (either may be NULL).  Integer counters are exact; float sums per frame in fp32 in the sync
 * kernel's order, over the frames of a cell in fp64, one addition per frame --, so repeated calls give identical bits, a split
 * frame range gives the integer counters of one call, and a point's results do not depend on which other points share its
 * call.  A point with linewidth = 0, under either flag, gives the bits of wofdm_rx_profile, err_power bytes included (as long
 * as no cell's frames are split over two chunks of that call).
 *   Every limit and check of wofdm_rx_profile applies.  WOFDM_E_INVALID: NULL points or errs, n_points < 1, a non-finite or
 * negative linewidth, cpe_tracked other than 0 or 1, reserved != 0; WOFDM_E_UNSUPPORTED: n_points > WOFDM_PN_MAX_POINTS,
 * linewidth > 1.  Every argument is checked before the device is touched; a failed call leaves all four outputs as they were.
 *   Chunks: min(65535, WOFDM_RX_PROFILE_CHUNK_BYTES / (8 (S n_fft + T + [mask] S (2P-1)) + 8 S B + 8 n_points (n_fft + S)))
 * frames -- wofdm_rx_profile_sync's formula plus the walk, S B doubles.
 *   A successful call counts for wofdm_rx_profile_kernel_ms.
 *   Measured on an MI355X (tools/bench_rx_profile_pn.py, profiles/rx_profile_pn.txt): on 64 cells x 2000 frames x 16 symbols at
 * n_fft = 256 one point takes 55.9 ms of kernels (83.1 ms masked), 1.43 (1.17) times one wofdm_rx_profile call on the same cells
 * and frames in the same run; four points take 79.1 (106.9) ms, 2.02 (1.51) times -- 0.20 (0.11) of a plain call per
 * additional point, beside wofdm_rx_profile_sync's 0.30 (0.22) per point measured the same way. */
#define WOFDM_PN_MAX_POINTS 16
typedef struct wofdm_pn_point {
    float   linewidth;    /* beta: two-sided 3 dB Lorentzian linewidth in subcarrier spacings, 0 <= beta <= 1 */
    int32_t cpe_tracked;  /* 0: free-running oscillator; 1: the common phase error of every symbol removed (a genie) */
    int32_t reserved[2];  /* 0 */
} wofdm_pn_point;
int wofdm_rx_profile_pn(const wofdm_cfg *cfg, int device,
                        const float *w_tx,                  /* [pairs][P] */
                        const float *w_rx,                  /* [pairs][N+tail_rx] */
                        const float *h,                     /* [n_channels][n_taps][2] */
                        const float *snr_db,                /* [n_snr] */
                        const uint8_t *active,              /* [n_fft] or NULL */
                        const float *tx_mask,               /* [2P-1] or NULL */
                        int32_t n_points, const wofdm_pn_point *points,
                        uint64_t *errs,                     /* [n_points][cells][n_fft][2], ACCUMULATED into */
                        double *err_power,                  /* [n_points][cells][n_fft], or NULL */
                        uint64_t *sym_errs,                 /* [n_points][cells][S-1][2], or NULL */
                        double *sym_power);                 /* [n_points][cells][S-1], or NULL */

/* wofdm_rx_profile with the five impairments COMBINED: the amplifier of wofdm_rx_profile_pa, the moving channel of
 * wofdm_rx_profile_doppler, the neighbour of wofdm_rx_profile_aci, the receiver offsets of wofdm_rx_profile_sync and the phase
 * noise of wofdm_rx_profile_pn in one chain -- "which window pair is best at 3 dB back-off, 100 km/h, a 1e-3 linewidth and a
 * neighbour 10 dB up".  The effects do not add: the amplifier's regrowth and the neighbour's leakage both land on what the Rx
 * window rejects, and carrier offset and phase noise share the rotation.  A call takes a LIST of points, each switching on any
 * subset of the five; the Tx chain, the walk and (where a point wants it) the neighbour run once per frame, and every point
 * sees the same labels, noise, walk and neighbour.
 *   Model, one chain in the order of the physics, each stage exactly the one its own call documents:
 *   1. the Tx chain of wofdm_rx_profile, once per frame;
 *   2. the point's amplifier on the finished waveform (wofdm_rx_profile_pa's materialising kernel; pa_model = WOFDM_PA_LINEAR
 *      reads x itself);
 *   3. the channel: track >= 0 picks h_track[track], with the taps taken at the OUTPUT sample's time as in
 *      wofdm_rx_profile_doppler; track = -1 the static h;
 *   4. where aci_on, the neighbour of wofdm_rx_profile_aci -- S + 1 symbols of stream 2 on aci_active, generated once per
 *      frame if any point wants it, linear, through the static aci_h (NULL: h) -- at the point's amplitude
 *      10^(aci_level_db / 20) and offset B - aci_delay; an aci_active that loads no bin is no neighbour;
 *   5. g n: Ps is measured per point on the point's waveform and channel (as _pa and _doppler do), Pn with the first point;
 *      neither sees the neighbour, the offsets or the phase;
 *   6. the windows begin at s B + prefix_rm + timing;
 *   7. the received sample -- signal, neighbour and noise -- is multiplied by wofdm_rx_profile_sync's factor and then by
 *      wofdm_rx_profile_pn's: two multiplies, each in the form its own call has, each exactly (1, 0) when neutral;
 *   8. Rx window, fold, shift, DFT, pilot of symbol 0, equaliser, slicer and counters, unchanged.
 *   Three interactions have a rule of their own.
 *   The walk under a timing offset: the unit walk stays wofdm_rx_profile_pn's, u[a] for 0 <= a < S B, in its order of
 *   additions.  A sample at on-air index a outside [0, S B) reads u[clamp(a, 0, S B - 1)]: the oscillator holds its phase
 *   outside the frame.  At timing = 0 the clamp is never met (the largest index read is exactly S B - 1).  The tracked mean
 *   is taken over the same clamped values.
 *   The tap time under a timing offset: the knots must cover tail_tx + S B + n_taps - 2 + max(0, the largest timing of the
 *   call), else WOFDM_E_INVALID.  For a < 0 every product is zero; the tap time used there is 0, so no tap is ever formed from
 *   a wrapped index.
 *   The static channel beside tracks: the library stages h as one more track, h at every knot -- with equal knots the
 *   interpolated tap is the knot, bit for bit --, so there is one tap path and track = -1 gives the bits of h.
 *   Identities: a call whose point has one impairment on returns, for that point, the BYTES of that impairment's own entry
 *   point with the same cfg and seed (all five outputs of wofdm_rx_profile_pa; the per-bin outputs of wofdm_rx_profile_aci), and
 *   an all-off point those of wofdm_rx_profile (as long as no cell's frames are split over two chunks of either call).
 *   Arguments: h is always needed; h_track [n_tracks][n_channels][n_knots][n_taps][2] with n_tracks <=
 * WOFDM_DOPPLER_MAX_TRACKS, n_knots, knot_step as in wofdm_rx_profile_doppler, NULL (and the three integers ignored) when no
 * point names a track; aci_active and aci_h as in wofdm_rx_profile_aci, both may be NULL when no point has aci_on; ref_power
 * [pairs] as in wofdm_rx_profile_pa, may be NULL when every point is linear.
 *   Outputs: the five of wofdm_rx_profile_pa, "point" on the leading axis, ACCUMULATED into, with its NULL rules and its
 * ordered sums; pa_power of a linear point is {sum |x|^2, sum |x|^2}.
 *   Limits, the union of the five calls': |timing| < B, |cfo| <= 4, 0 <= linewidth <= 1, 0 <= aci_delay < B, a finite level
 * whose amplitude is finite in single precision, the amplifier's limits, the knots' limits, -1 <= track < n_tracks, flags 0 or
 * 1, reserved 0, n_points in [1, WOFDM_LINK_MAX_POINTS], and no needed argument NULL.  Every argument is checked before the
 * device is touched; a failed call leaves all five outputs as they were.
 *   Chunks: min(65535, WOFDM_RX_PROFILE_CHUNK_BYTES / (8 (S n_fft + T + [mask] S (2P-1)) + 8 n_points (n_fft + S + T) + 8 S B +
 * [a point has aci_on] 8 ((S + 1) n_fft + T + B + [mask] (S + 1) (2P-1))))  frames -- wofdm_rx_profile_pa's formula plus the
 * walk plus the neighbour's buffers.
 *   A successful call holds the launch gate and counts for wofdm_rx_profile_kernel_ms.
 *   Measured on an MI355X (tools/bench_rx_profile_link.py, profiles/rx_profile_link.txt): on 64 cells x 2000 frames x 16 symbols at
 * n_fft = 256 a point costs 73 ms of kernels (98 ms masked) whatever single impairment it switches on, 1.88 (1.39) times one
 * wofdm_rx_profile call on the same cells and frames in the same run and 1.2 to 1.7 times that impairment's own entry point --
 * every point pays the power pass and per-lane taps; one point with everything on takes 94.2 (143.0) ms, four such points 201.4
 * (275.4) ms, 5.17 (3.90) times -- 0.92 (0.62) of a plain call per additional point. */
#define WOFDM_LINK_MAX_POINTS 16
typedef struct wofdm_link_point {
    int32_t pa_model; float pa_ibo_db; float pa_smooth;    /* wofdm_pa_point's; WOFDM_PA_LINEAR = no amplifier      */
    int32_t track;                                         /* index into h_track, or -1 = the static channel h      */
    int32_t timing; float cfo; int32_t cfo_tracked;        /* wofdm_sync_point's                                    */
    float   linewidth; int32_t cpe_tracked;                /* wofdm_pn_point's                                      */
    int32_t aci_on; int32_t aci_delay; float aci_level_db; /* neighbour on the air for this point; delay, level     */
    int32_t reserved[4];                                   /* 0                                                     */
} wofdm_link_point;
int wofdm_rx_profile_link(const wofdm_cfg *cfg, int device,
                          const float *w_tx,                /* [pairs][P] */
                          const float *w_rx,                /* [pairs][N+tail_rx] */
                          const float *h,                   /* [n_channels][n_taps][2] */
                          const float *snr_db,              /* [n_snr] */
                          const uint8_t *active,            /* [n_fft] or NULL */
                          const float *tx_mask,             /* [2P-1] or NULL */
                          const float *h_track,             /* [n_tracks][n_channels][n_knots][n_taps][2], or NULL */
                          int32_t n_tracks, int32_t n_knots, int32_t knot_step,
                          const uint8_t *aci_active,        /* [n_fft], or NULL */
                          const float *aci_h,               /* [n_channels][n_taps][2], or NULL = h */
                          const float *ref_power,           /* [pairs], or NULL */
                          int32_t n_points, const wofdm_link_point *points,
                          uint64_t *errs,                   /* [n_points][cells][n_fft][2], ACCUMULATED into */
                          double *err_power,                /* [n_points][cells][n_fft], or NULL */
                          uint64_t *sym_errs,               /* [n_points][cells][S-1][2], or NULL */
                          double *sym_power,                /* [n_points][cells][S-1], or NULL */
                          double *pa_power);                /* [n_points][cells][2], or NULL */

/* wofdm_rx_profile_link with SOFT decisions: beside the hard counters of every point, what a coded receiver could carry -- the
 * bit-interleaved coded modulation (BICM) rate, the generalized mutual information (GMI) of the max-log bit metrics the
 * demapper would hand a decoder, per bin and per data symbol.  At the error rates the combined impairments give, uncoded BER is
 * set by the few bins in a null and ranks window pairs otherwise than the rate does; EVM cannot stand in for it, the
 * disturbance (regrowth, ICI, phase noise) not being Gaussian.
 *   Definition.  For a point, a loaded bin n and a data symbol s >= 1 of a frame, with the quantities of the link chain:
 *     e      = G[n] Y_s[n], the equalised value the slicer sees, G[n] = X_0[n] / Y_0[n] the point's pilot equaliser;
 *     v      = g^2 Pn / NL, the per-sample noise variance add_wgn put on the air for this frame and point -- g, Pn, NL exactly
 *              what pass 1 measures (v = Ps / NL 10^(-snr / 10)); where pass 1 runs per point, the point's;
 *     W2     = sum_{m < n_fft + tail_rx} w_rx[m]^2 of the pair, formed on the host in double precision, passed in single;
 *     nu[n]  = |G[n]|^2 v W2, the noise variance the receiver would ASSUME on the bin: it never sees the neighbour, the
 *              offsets, the phase or the amplifier's distortion -- hence the scales below;
 *     L_i    = ( min_{x: bit_i(x) = 1} |e - x|^2 - min_{x: bit_i(x) = 0} |e - x|^2 ) / nu[n], the max-log metric of bit i of the
 *              label, i = 0 the top bit, over the unit-power constellation with the slicer's MATLAB Gray labelling; L_i > 0
 *              decides for bit 0, and its sign is the slicer's decision.  The kernel forms the difference per axis (the other
 *              axis' distance is common to both minima), at most 8 levels per axis;
 *     pen_j  = sum_{i < k} log2(1 + exp(-(1 - 2 b_i) c_j L_i)), b_i the transmitted bit, for every scale c_j of the call,
 *              evaluated as max(-z, 0) + log1p(exp(-|z|)) in base 2 with the hardware exp2 / log2 (below 2^-6 the log1p is
 *              its series, so the small penalties keep their relative accuracy).
 *   The call accumulates bit_penalty[point][cell][scale][n], the sum of pen_j over the frames and data symbols, and
 * sym_penalty[point][cell][scale][s - 1], the sum over the frames and loaded bins.  k - penalty / decisions is an achievable
 * rate for EVERY scale, so the caller takes the maximum over the scales -- per bin, per symbol or per cell.  The matched scale
 * is not 1: the pilot's own noise alone pushes it to about 0.5, interference the receiver does not model far lower (0.01 where
 * ISI dominates), and an octave grid gives up as much as 10 % of the rate against a fine one -- so a list, 1 <= n_scales <=
 * WOFDM_SOFT_MAX_SCALES, each finite and positive.
 *   Order of additions: a wave writes the penalties of its symbol's bins, fp32, to a scratch [frame][point][S-1][scale][n_fft]
 * and leaves their sum over the loaded bins -- a lane's bins n = lane + 64 j ascending, then the wave sum of the per-symbol
 * error power -- beside it; a second kernel adds, per (point, scale, bin), the data symbols of a frame ascending in single
 * precision; a third makes ONE addition per frame onto the running fp64 total of the cell, frames ascending (the same for the
 * symbols' sums).
 * No float atomics; repeated calls give identical bytes, the totals do not depend on where a chunk ends, a scale's results do
 * not depend on which other scales share its call, nor a point's on the other points.  Unloaded bins are exactly 0; a loaded bin
 * with Y_0 = 0 behaves as err_power does.
 *   The five outputs of wofdm_rx_profile_link are, for the same cfg, seed and points, the BYTES of wofdm_rx_profile_link (as
 * long as no cell's frames are split over two chunks of either call): the hard counters and powers are produced by the same
 * statements.
 *   Every argument, limit and check of wofdm_rx_profile_link applies.  WOFDM_E_INVALID: NULL scales or bit_penalty, n_scales <
 * 1, a scale that is not finite or not positive; WOFDM_E_UNSUPPORTED: n_scales > WOFDM_SOFT_MAX_SCALES.  Every argument is
 * checked before the device is touched; a failed call leaves all seven outputs as they were.
 *   Chunks: min(65535, WOFDM_RX_PROFILE_CHUNK_BYTES / (wofdm_rx_profile_link's bytes of a frame + 4 n_points n_scales ((S - 1)
 * n_fft + S)))  frames -- the link call's formula plus the fp32 penalties of every (point, scale): per data symbol the bins, and
 * the symbols' sums.
 *   A successful call holds the launch gate and counts for wofdm_rx_profile_kernel_ms.
 *   Measured on an MI355X (tools/bench_rx_profile_soft.py, profiles/rx_profile_soft.txt): on 64 cells x 2000 frames x 16 symbols
 * at n_fft = 256 an all-off point takes 96.2 ms of kernels with one scale and 136.7 ms with sixteen (masked 123.0 and 166.1 ms),
 * 1.40 and 1.98 (1.33 and 1.80) times wofdm_rx_profile_link with the same point in the same run; the everything-on point 122.4
 * and 175.7 (176.3 and 211.9) ms, 1.37 and 1.97 (1.23 and 1.48) times -- about 30 ms that do not depend on the scales and 0.02 to
 * 0.04 of a link call per further scale.  Other n_fft: not measured. */
#define WOFDM_SOFT_MAX_SCALES 16
int wofdm_rx_profile_soft(const wofdm_cfg *cfg, int device,
                          const float *w_tx,                /* [pairs][P] */
                          const float *w_rx,                /* [pairs][N+tail_rx] */
                          const float *h,                   /* [n_channels][n_taps][2] */
                          const float *snr_db,              /* [n_snr] */
                          const uint8_t *active,            /* [n_fft] or NULL */
                          const float *tx_mask,             /* [2P-1] or NULL */
                          const float *h_track,             /* [n_tracks][n_channels][n_knots][n_taps][2], or NULL */
                          int32_t n_tracks, int32_t n_knots, int32_t knot_step,
                          const uint8_t *aci_active,        /* [n_fft], or NULL */
                          const float *aci_h,               /* [n_channels][n_taps][2], or NULL = h */
                          const float *ref_power,           /* [pairs], or NULL */
                          int32_t n_points, const wofdm_link_point *points,
                          int32_t n_scales, const float *scales,
                          uint64_t *errs,                   /* [n_points][cells][n_fft][2], ACCUMULATED into */
                          double *err_power,                /* [n_points][cells][n_fft], or NULL */
                          uint64_t *sym_errs,               /* [n_points][cells][S-1][2], or NULL */
                          double *sym_power,                /* [n_points][cells][S-1], or NULL */
                          double *pa_power,                 /* [n_points][cells][2], or NULL */
                          double *bit_penalty,              /* [n_points][cells][n_scales][n_fft], ACCUMULATED into */
                          double *sym_penalty);             /* [n_points][cells][n_scales][S-1], or NULL */

/* wofdm_rx_profile_soft behind a TRACKING receiver.  Every other receive profile equalises with the one least-squares estimate of
 * symbol 0 and holds it for the frame, and the only relief on offer is a genie (cfo_tracked, cpe_tracked) no receiver has.
 * This call gives the receiver two mechanisms of a real one: a comb of pilot subcarriers in every data symbol, from which it
 * estimates the symbol's common phase, and a postamble, a second known symbol at the frame's end, between which and the pilot it
 * interpolates the channel estimate.  Which window pair is best on a link that drifts is a question for this receiver: a window
 * that rejects ICI and one that merely rotates less rank differently once the common rotation is estimated and removed.
 *   Per call: pilots [n_fft], or NULL for no comb; a non-zero entry makes the bin a pilot bin.  Per link point one
 * wofdm_tracking_point {cpe, post}: cpe = 1 switches on the comb's phase estimate, post = 1 makes symbol S - 1 a postamble.  The
 * Tx side is untouched: a pilot bin carries the label the stream gives it, and the receiver knows it, as it already knows symbol
 * 0; with post it also knows symbol S - 1.
 *   Definition.  For a point, a frame and a data symbol s -- 1 <= s <= S - 1, with post 1 <= s <= S - 2 --, Y_s the link chain's
 * DFT outputs, X_s the transmitted points and t = s / (S - 1):
 *     H0[n]  = Y_0[n] / X_0[n] on the loaded bins; with post HL[n] = Y_{S-1}[n] / X_{S-1}[n];
 *     Hh_s   = H0 without post.  With post cL = sum_{n loaded} HL[n] conj(H0[n]), rho = cL / |cL| (1 if cL = 0), and
 *              Hh_s = H0 + t (HL conj(rho) - H0): the SHAPE is interpolated with the postamble's common rotation taken off, so a
 *              free-running oscillator does not wreck the interpolation;
 *     q_s    = with cpe: c_s / |c_s| (1 if c_s = 0), c_s = sum_{p in pilots} Y_s[p] conj(Hh_s[p] X_s[p]) -- the channel-weighted
 *              estimate: a plain phase average over equalised pilots lets faded bins dominate --; with post and no cpe:
 *              e^{i t arg rho}, arg the principal value, which is right while the drift over the frame stays under half a turn;
 *              with neither: 1;
 *     e      = Y_s[n] conj(q_s) / Hh_s[n], and nu_s[n] = v W2 / |Hh_s[n]|^2, v and W2 wofdm_rx_profile_soft's.
 *   The slicer, the error vector and the demapper all see this one e, and everything behind it is wofdm_rx_profile_soft's.
 *   Pilot bins count no decision, no error, no power and no penalty on ANY point of the call: they are exact zeros, as unloaded
 * bins are; symbol S - 1 of a point with post likewise, per symbol and in the bins' sums.  A bin of point i so takes
 * frames (S - 1 - post_i) decisions.
 *   Order of additions: cL and c_s are formed by one wave, a lane's bins n = lane + 64 j ascending, then the wave sum of the
 * per-symbol error power, on either component; everything else as wofdm_rx_profile_soft.  For a point with post the waves visit
 * the symbols in the order 0, S - 1, 1, ... S - 2; for every other point in the soft call's order.
 *   Identities, by bytes: with pilots NULL and every point {0, 0} all seven outputs are wofdm_rx_profile_soft's; with a comb a
 * {0, 0} point has its bytes on every data bin of errs, err_power and bit_penalty.  A point's results do not depend on the
 * other points of the call, a scale's not on the other scales; repeated calls give identical bytes; the totals do not depend on
 * where a chunk ends.
 *   Every argument, limit and check of wofdm_rx_profile_soft applies, then, in this order, WOFDM_E_INVALID for: a pilot on a bin
 * that is not loaded; a comb that leaves no loaded bin for data; and point by point cpe or post outside {0, 1}; reserved not 0;
 * post with syms_per_frame < 3; cpe without a pilot bin.  NULL tracking is WOFDM_E_INVALID.  Every argument is checked before
 * the device is touched; a failed call leaves all seven outputs as they were.
 *   Chunks: wofdm_rx_profile_soft's formula -- the receiver has no per-frame buffers of its own.
 *   A successful call holds the launch gate and counts for wofdm_rx_profile_kernel_ms.
 *   Measured on an MI355X (tools/bench_rx_profile_tracking.py, profiles/rx_profile_tracking.txt): on 64 cells x 2000 frames x 16
 * symbols at n_fft = 256, one point with a free-running carrier offset and linewidth, a comb on every eighth loaded bin, against
 * wofdm_rx_profile_soft with the same point in the same run (96.4 ms of kernels with one scale, 139.1 ms with sixteen; masked 123.2
 * and 167.1 ms; spread over the rounds 0.3 ms): the {0, 0} receiver 1.012 and 0.999 (masked 1.011 and 1.010) times, {1, 0} 1.038 and
 * 1.005 (1.031 and 1.023), {0, 1} 1.032 and 1.002 (1.027 and 1.032), {1, 1} 1.043 and 1.009 (1.036 and 1.027) -- at most 4.6 ms, more
 * than the spread: the comb correlation and one pass over the bins per data symbol, the second estimate and one more barrier per
 * frame; how the 4 ms split between them was not measured.  Other n_fft: not measured. */
typedef struct wofdm_tracking_point {
    int32_t cpe;                                           /* 1: the comb's common-phase estimate per data symbol        */
    int32_t post;                                          /* 1: symbol S - 1 is a postamble                             */
    int32_t reserved[2];                                   /* 0                                                          */
} wofdm_tracking_point;
int wofdm_rx_profile_tracking(const wofdm_cfg *cfg, int device,
                              const float *w_tx,            /* [pairs][P] */
                              const float *w_rx,            /* [pairs][N+tail_rx] */
                              const float *h,               /* [n_channels][n_taps][2] */
                              const float *snr_db,          /* [n_snr] */
                              const uint8_t *active,        /* [n_fft] or NULL */
                              const float *tx_mask,         /* [2P-1] or NULL */
                              const float *h_track,         /* [n_tracks][n_channels][n_knots][n_taps][2], or NULL */
                              int32_t n_tracks, int32_t n_knots, int32_t knot_step,
                              const uint8_t *aci_active,    /* [n_fft], or NULL */
                              const float *aci_h,           /* [n_channels][n_taps][2], or NULL = h */
                              const float *ref_power,       /* [pairs], or NULL */
                              int32_t n_points, const wofdm_link_point *points,
                              int32_t n_scales, const float *scales,
                              const uint8_t *pilots,        /* [n_fft], or NULL */
                              const wofdm_tracking_point *tracking, /* [n_points] */
                              uint64_t *errs,               /* [n_points][cells][n_fft][2], ACCUMULATED into */
                              double *err_power,            /* [n_points][cells][n_fft], or NULL */
                              uint64_t *sym_errs,           /* [n_points][cells][S-1][2], or NULL */
                              double *sym_power,            /* [n_points][cells][S-1], or NULL */
                              double *pa_power,             /* [n_points][cells][2], or NULL */
                              double *bit_penalty,          /* [n_points][cells][n_scales][n_fft], ACCUMULATED into */
                              double *sym_penalty);         /* [n_points][cells][n_scales][S-1], or NULL */

/* The CODED link: wofdm_rx_profile_tracking with an 8-bit soft-bit interface behind the demapper and a K = 7 Viterbi decoder behind
 * that.  The GMI of the calls above is a bound for an ideal code at the best metric scale; a receiver with a fixed-point demapper
 * and a real decoder falls short of it by an amount that depends on where in the band and in the frame the bad soft bits sit.
 *   Soft bit.  For a point, a frame, a data symbol s, a data bin n (loaded, no pilot bin) and label bit i (0 = the top bit), z_i
 * = (1 - 2 b_i) Lambda_i is what the demapper forms in single precision -- e and nu the tracking receiver's; the scales do not
 * enter --, and d = clamp(rint(llr_scale z_i), -127, 127), round half even, an int8; NaN gives 0.  d > 0: the demapper agrees
 * with the transmitted bit.  This is the random-coset view: the Philox labels are the scrambler, the transmitted codeword is all
 * zero, and the frames are those of every other entry point.  Unloaded bins, pilot bins and the postamble of a point with post
 * hold 0.
 *   Order.  A symbol's position j = r k + i, r the rank of bin n among the data bins ascending; n_c = k D, D the data bins.  The
 * interleaver perm [n_c] is a permutation of 0 ... n_c - 1: coded-stream index c reads position perm[c]; NULL is the identity.
 *   Code.  K = 7, generators 133 / 171 octal: register r_t = (u_t << 6) | s_{t-1}, state s_{t-1} = (u_{t-1} ... u_{t-6}) with
 * u_{t-1} in bit 5; A_t = parity(r_t & 0133), B_t = parity(r_t & 0171); s_t = (u_t << 5) | (s_{t-1} >> 1).  The predecessors of
 * state s are p0 = (s << 1) & 63 and p1 = p0 | 1, its input bit s >> 5.  Free distance 10.
 *   Rates, by the pattern index t mod period:   rate 0 = 1/2: A and B always;   rate 1 = 2/3: A 1 1, B 1 0;   rate 2 = 3/4: A 1 1 0,
 * B 1 0 1.  The kept outputs of step t, A before B, t ascending, consume c = 0, 1, 2, ...; T = wofdm_code_steps(rate, n_c) is the
 * largest T whose kept outputs number at most n_c (n_c = 56: 28 / 37 / 42; 57: 28 / 38 / 42; 64: 32 / 42 / 48; 6144: 3072 / 4096 /
 * 4608), left-over positions are ignored.  One zero-terminated codeword per point, frame and data symbol: the last 6 steps are the
 * tail, and T >= 7.
 *   Decoder.  Pure integer arithmetic: the metric to minimise is the sum of d over the kept outputs whose hypothesised coded bit
 * is 1, int32 throughout.  Only paths from state 0 are considered (2^30 on the other states at t = 0, which is equivalent for
 * every T here); the survivor into a state is p0 unless p1's metric is strictly smaller; the traceback starts from state 0 at
 * step T.  A decoded u_t != 0 for t < T - 6 is an info-bit error, any u_t != 0 a codeword error.  One wave per codeword, one
 * state per lane; the survivors stay in LDS.
 *   The call takes every argument of wofdm_rx_profile_tracking through `tracking`, then llr_scale, perm, and 1 <= n_codes <=
 * WOFDM_CODE_MAX codes, all decoded from the same soft bits; then the seven outputs, which are wofdm_rx_profile_tracking's bytes;
 * then code_errs[point][cell][code][s - 1] = {info-bit errors, codeword errors}, ACCUMULATED into; then soft_bits[cell][frame]
 * [point][s - 1][n][8] (bytes k ... 7 are 0), or NULL -- overwritten, not accumulated, chunk by chunk as the call goes.  A point
 * with post adds nothing for symbol S - 1.
 *   Identities, by bytes: the counters are integers added by integer atomics, so code_errs depends neither on where a chunk ends,
 * nor on the other points or codes of the call, nor on whether soft_bits is requested; repeated calls are identical.
 *   Checks: wofdm_rx_profile_tracking's, then in this order WOFDM_E_INVALID for NULL codes or code_errs; llr_scale not finite or
 * not positive; n_codes < 1 (WOFDM_E_UNSUPPORTED for n_codes > WOFDM_CODE_MAX); code by code a rate outside {0, 1, 2}, reserved not
 * 0, T < 7; perm not a permutation; and WOFDM_E_UNSUPPORTED for soft_bits of more than 2^30 bytes.  Every argument is checked
 * before the device is touched; a failed check leaves all outputs as they were.  (A device failure in a later chunk leaves
 * soft_bits holding the earlier chunks' blocks: it is copied as the call goes; every other output is written at the end.)
 *   Chunks: wofdm_rx_profile_tracking's formula plus 8 n_points (S - 1) n_fft bytes per frame, the soft bits.
 *   A successful call holds the launch gate and counts for wofdm_rx_profile_kernel_ms (with soft_bits, the copies included).
 *   Measured on an MI355X (tools/bench_rx_profile_coded.py, profiles/rx_profile_coded.txt): on 64 cells x 2000 frames x 16 symbols
 * at n_fft = 256, 16-QAM, one point behind the (1, 1) receiver and a comb on every eighth loaded bin (n_c = 448), the tracking
 * call takes 104.9 ms of kernels, this call 130.5 ms with one code and 182.2 ms with three (masked 133.5, 148.4 and 200.2 ms):
 * 25.9 ms per code, 0.25 (masked 0.19) of a tracking call; the soft-bit stores cost nothing measurable.  Other n_fft: not measured. */
#define WOFDM_CODE_MAX 4
#define WOFDM_CODE_MAX_STEPS 4608                          /* wofdm_viterbi_decode: the most steps of a codeword         */
typedef struct wofdm_code {
    int32_t rate;                                          /* 0: 1/2, 1: 2/3, 2: 3/4                                     */
    int32_t reserved[3];                                   /* 0                                                          */
} wofdm_code;
int wofdm_rx_profile_coded(const wofdm_cfg *cfg, int device,
                           const float *w_tx,               /* [pairs][P] */
                           const float *w_rx,               /* [pairs][N+tail_rx] */
                           const float *h,                  /* [n_channels][n_taps][2] */
                           const float *snr_db,             /* [n_snr] */
                           const uint8_t *active,           /* [n_fft] or NULL */
                           const float *tx_mask,            /* [2P-1] or NULL */
                           const float *h_track,            /* [n_tracks][n_channels][n_knots][n_taps][2], or NULL */
                           int32_t n_tracks, int32_t n_knots, int32_t knot_step,
                           const uint8_t *aci_active,       /* [n_fft], or NULL */
                           const float *aci_h,              /* [n_channels][n_taps][2], or NULL = h */
                           const float *ref_power,          /* [pairs], or NULL */
                           int32_t n_points, const wofdm_link_point *points,
                           int32_t n_scales, const float *scales,
                           const uint8_t *pilots,           /* [n_fft], or NULL */
                           const wofdm_tracking_point *tracking, /* [n_points] */
                           float llr_scale,
                           const int32_t *perm,             /* [n_c], or NULL */
                           int32_t n_codes, const wofdm_code *codes,
                           uint64_t *errs,                  /* [n_points][cells][n_fft][2], ACCUMULATED into */
                           double *err_power,               /* [n_points][cells][n_fft], or NULL */
                           uint64_t *sym_errs,              /* [n_points][cells][S-1][2], or NULL */
                           double *sym_power,               /* [n_points][cells][S-1], or NULL */
                           double *pa_power,                /* [n_points][cells][2], or NULL */
                           double *bit_penalty,             /* [n_points][cells][n_scales][n_fft], ACCUMULATED into */
                           double *sym_penalty,             /* [n_points][cells][n_scales][S-1], or NULL */
                           uint64_t *code_errs,             /* [n_points][cells][n_codes][S-1][2], ACCUMULATED into */
                           int8_t *soft_bits);              /* [cells][frames][n_points][S-1][n_fft][8], or NULL */

/* Host only: the steps T of a codeword of rate 0, 1 or 2 over n_c coded-stream positions (above); WOFDM_E_INVALID otherwise. */
int wofdm_code_steps(int32_t rate, int32_t n_c);

/* The decoder alone, on soft bits of the caller's: n_cw codewords of n_c soft bits each, d > 0 for a coded bit 0, any int8
 * (-128 included); coded-stream index c of a codeword reads soft[cw][perm[c]] (NULL: c).  bits[cw][t], t < T =
 * wofdm_code_steps(rate, n_c), are the decoded u_t, the tail included; metric[cw] the survivor's metric at state 0.  It decodes
 * any codeword, not only the all-zero one.  WOFDM_E_INVALID: NULL soft or bits, a rate outside {0, 1, 2}, n_c or n_cw < 1, T < 7,
 * perm not a permutation; WOFDM_E_UNSUPPORTED: T > WOFDM_CODE_MAX_STEPS.  Checked before the device is touched.  The call
 * holds the launch gate while its kernel runs; it neither counts for nor resets wofdm_rx_profile_kernel_ms. */
int wofdm_viterbi_decode(int device, int32_t rate, int32_t n_c,
                         const int32_t *perm,               /* [n_c], or NULL */
                         int32_t n_cw,
                         const int8_t *soft,                /* [n_cw][n_c] */
                         uint8_t *bits,                     /* [n_cw][T] */
                         int32_t *metric);                  /* [n_cw], or NULL */

/* The same decoder for codewords of any length up to WOFDM_CODE_LONG_MAX_STEPS steps: arguments, checks, code, metric, start and
 * tie rule are wofdm_viterbi_decode's, and on every word that call takes, bits and metric are that call's -- exact maximum-
 * likelihood decoding, no truncated window.  WOFDM_E_UNSUPPORTED only for T > WOFDM_CODE_LONG_MAX_STEPS.  One wave per codeword,
 * one state per lane; the survivor history streams to device memory in blocks of 64 steps, 512 bytes each, so the scratch is
 * 512 ceil(T / 64) bytes per codeword (8 MiB at the largest T), and the call walks the codewords in groups whose scratch stays
 * within WOFDM_RX_PROFILE_CHUNK_BYTES.  int32 suffices for the metric: |d| <= 128 and two outputs per step, so |metric| <= 256 T
 * <= 2^28 beside the 2^30 of the start.  The call holds the launch gate while its kernels run; it neither counts for nor resets
 * wofdm_rx_profile_kernel_ms. */
#define WOFDM_CODE_LONG_MAX_STEPS 1048576
int wofdm_viterbi_decode_long(int device, int32_t rate, int32_t n_c,
                              const int32_t *perm,          /* [n_c], or NULL */
                              int32_t n_cw,
                              const int8_t *soft,           /* [n_cw][n_c] */
                              uint8_t *bits,                /* [n_cw][T] */
                              int32_t *metric);             /* [n_cw], or NULL */

/* The coded link with FRAME-SPANNING codewords: wofdm_rx_profile_coded's soft bits -- the same frames, quantiser, order within a
 * symbol, n_c = k D and random-coset view --, but ONE zero-terminated codeword per point and frame over the point's data symbols,
 * interleaved in time as well as in frequency, decoded by the streaming decoder of wofdm_viterbi_decode_long.
 *   Codeword.  A point has S_d = S - 1 data symbols, S - 2 with post; its codeword has n_f = n_c S_d coded-stream positions and T =
 * wofdm_code_steps(rate, n_f) steps per code.  (A point with S_d = 0 would carry no codeword and count nothing; the tracking
 * receiver's own checks ask for S >= 3 with post, so S_d >= 1 in every call that passes them.)
 *   Frame interleaver.  Coded-stream index c sits in data symbol 1 + j, j = c mod S_d, and with q = c div S_d at the symbol's
 * position perm[(q + j sym_rot) mod n_c] (NULL perm: the identity).  For each j this is a bijection of the symbol's positions;
 * consecutive coded bits go to consecutive symbols and, for sym_rot != 0, to different places of the band.  With S_d = 1 and sym_rot
 * = 0 it is perm itself: the per-symbol call's codeword.
 *   Arguments: every argument of wofdm_rx_profile_coded through codes, then sym_rot; the seven outputs of
 * wofdm_rx_profile_tracking, which are that call's bytes; frame_errs[point][cell][code] = {info-bit errors (decoded u_t != 0, t < T
 * - 6), codeword errors}, ACCUMULATED into; soft_bits as in wofdm_rx_profile_coded, the same bytes.
 *   Identities, by bytes: frame_errs depends neither on where a chunk ends, nor on the other points or codes of the call, nor on
 * whether soft_bits is requested; repeated calls are identical; it equals wofdm_viterbi_decode_long on the exported soft bits
 * gathered through the frame interleaver; with S = 2, no post and sym_rot = 0 it is code_errs[...][0] of wofdm_rx_profile_coded.
 *   Checks: wofdm_rx_profile_coded's -- without code_errs, and without its T < 7 per symbol: a symbol holds no codeword here --,
 * then in this order WOFDM_E_INVALID for sym_rot outside [0, n_c); for NULL frame_errs; for a code whose T < 7 at an S_d in use;
 * and WOFDM_E_UNSUPPORTED for a T > WOFDM_CODE_LONG_MAX_STEPS (which n_fft <= 1024, k <= 6 and S <= 64 never reach).  Every argument
 * is checked before the device is touched; a failed check leaves all outputs as they were.
 *   Chunks: wofdm_rx_profile_coded's formula plus 512 n_points ceil(T_max / 64) bytes per frame, the survivor history, T_max the
 * longest codeword of the call; the codes of a chunk are decoded by one launch each and share the history.
 *   A successful call holds the launch gate and counts for wofdm_rx_profile_kernel_ms.
 *   Measured: tools/bench_rx_profile_coded_frame.py, profiles/rx_profile_coded_frame.txt. */
int wofdm_rx_profile_coded_frame(const wofdm_cfg *cfg, int device,
                                 const float *w_tx,             /* [pairs][P] */
                                 const float *w_rx,             /* [pairs][N+tail_rx] */
                                 const float *h,                /* [n_channels][n_taps][2] */
                                 const float *snr_db,           /* [n_snr] */
                                 const uint8_t *active,         /* [n_fft] or NULL */
                                 const float *tx_mask,          /* [2P-1] or NULL */
                                 const float *h_track,          /* [n_tracks][n_channels][n_knots][n_taps][2], or NULL */
                                 int32_t n_tracks, int32_t n_knots, int32_t knot_step,
                                 const uint8_t *aci_active,     /* [n_fft], or NULL */
                                 const float *aci_h,            /* [n_channels][n_taps][2], or NULL = h */
                                 const float *ref_power,        /* [pairs], or NULL */
                                 int32_t n_points, const wofdm_link_point *points,
                                 int32_t n_scales, const float *scales,
                                 const uint8_t *pilots,         /* [n_fft], or NULL */
                                 const wofdm_tracking_point *tracking, /* [n_points] */
                                 float llr_scale,
                                 const int32_t *perm,           /* [n_c], or NULL */
                                 int32_t n_codes, const wofdm_code *codes,
                                 int32_t sym_rot,               /* in [0, n_c) */
                                 uint64_t *errs,                /* [n_points][cells][n_fft][2], ACCUMULATED into */
                                 double *err_power,             /* [n_points][cells][n_fft], or NULL */
                                 uint64_t *sym_errs,            /* [n_points][cells][S-1][2], or NULL */
                                 double *sym_power,             /* [n_points][cells][S-1], or NULL */
                                 double *pa_power,              /* [n_points][cells][2], or NULL */
                                 double *bit_penalty,           /* [n_points][cells][n_scales][n_fft], ACCUMULATED into */
                                 double *sym_penalty,           /* [n_points][cells][n_scales][S-1], or NULL */
                                 uint64_t *frame_errs,          /* [n_points][cells][n_codes][2], ACCUMULATED into */
                                 int8_t *soft_bits);            /* [cells][frames][n_points][S-1][n_fft][8], or NULL */

/* The coded link with a quasi-cyclic LDPC code and a layered min-sum decoder.
 *   The code is (J, L), 3 <= J <= 6, J < L <= 24, over a word of n transmitted positions.
 *   Lift.  Z = wofdm_ldpc_lift(J, L, n) is the smallest prime Z >= max(L, ceil(n / L)) whose multiplicative order of 2 is at least L.
 * The check matrix has J x L blocks of Z x Z.
 *   Blocks.  Block (i, j) is zero for j < i; otherwise it is the circulant that joins check i Z + r to variable j Z + ((r + s(i, j))
 * mod Z), s(i, j) = (i 2^j) mod Z.  Row i has degree L - i.  The structure has no 4-cycle: Z is prime and the 2^j, j < L, are
 * distinct mod Z.
 *   Parity and information.  Block columns 0 ... J - 1 are the parity part, block upper triangular with permutations on the
 * diagonal; the full length is n0 = L Z >= n.  The code is shortened by s = n0 - n: variables n ... n0 - 1 are known zeros and are
 * not transmitted.  The information bits are variables J Z ... n - 1, K = (L - J) Z - s of them; K >= 1, or the code is invalid.
 *   Encoder (wofdm_ldpc_encode below; wofdm_rx_profile_ldpc needs none, its codeword is all zero in the random-coset view).
 * Back-substitution from block row J - 1 up to 0: a row's parity block is the XOR of the row's other blocks through the diagonal
 * block's permutation.
 *   Decoder: pure integer, layered, normalised min-sum.  Start: Q[v] = d[v] (int8, any value, -128 included) for v < n and 127
 * for the shortened positions -- ordinary variables from there on --; R[e] = 0 on every edge.  One iteration is the layers i = 0 ...
 * J - 1 in order; a layer touches each variable at most once, so its checks are independent.  For a check and each of its edges j:
 * t_j = Q[v_j] - R_j, a_j = min(|t_j|, 127); m1 <= m2 the two smallest a over the edges; the new magnitude is (3 m) >> 2 with m =
 * m2 on an edge whose a_j = m1 and m1 elsewhere (ties need no rule: m2 = m1 then); the new sign is negative where the number of
 * negative t on the OTHER edges is odd, t = 0 counting as positive; Q[v_j] = t_j + R_j(new).  |Q| <= 128 + 6 * 95, so int16 holds
 * it and there is no saturation rule.  After each full iteration the hard decision is x[v] = (Q[v] < 0) over all n0 variables; if
 * every check's parity is even the word has converged and decoding stops, otherwise it goes on, up to max_iter, 1 <= max_iter <=
 * 64.  Outputs: x[0 ... n - 1], the iterations run, the converged flag.
 *   wofdm_ldpc_kernel: one workgroup per (codeword, code), Q as int16 and R as int8 in LDS, 304 + 2 L Z + Z (J L - J (J - 1) / 2)
 * bytes (each array rounded up to four): 33 KiB at (4, 8, 6272), at most 131 KiB at n = WOFDM_LDPC_MAX_BITS and J = 6, within the
 * 160 KiB of a workgroup (a code beyond that would be WOFDM_E_UNSUPPORTED; none in the ranges above is). */
#define WOFDM_LDPC_MAX_BITS 16384
typedef struct wofdm_ldpc_code {
    int32_t J, L;              /* 3 <= J <= 6, J < L <= 24 */
    int32_t max_iter;          /* 1 ... 64 */
    int32_t reserved;          /* 0 */
} wofdm_ldpc_code;

/* Host only: the lift Z (>= 5) of the (J, L) code over n positions, or WOFDM_E_INVALID (negative) outside the ranges above, for n
 * outside 1 ... 2^24, or where K < 1. */
int wofdm_ldpc_lift(int32_t J, int32_t L, int32_t n);

/* The decoder alone, on n_cw words of n soft bits each: coded-stream index c (variable c of the code) is read at soft[w][perm[c]]
 * (NULL perm: the identity), as in wofdm_viterbi_decode_long.  bits[w][v] = x[v], iters[w] the iterations run, converged[w] 0 / 1.
 *   Checks, all before the device is touched, in this order: WOFDM_E_INVALID for NULL soft or bits; J, L; max_iter; n or n_cw < 1;
 * WOFDM_E_UNSUPPORTED for n > WOFDM_LDPC_MAX_BITS; WOFDM_E_INVALID for K < 1; WOFDM_E_UNSUPPORTED for a decoder state beyond a
 * workgroup's LDS (a guard: no code of the ranges above reaches it); WOFDM_E_INVALID for a perm that is no permutation.  A failed
 * check leaves the outputs as they were.  The call holds the launch gate while its kernel runs; it neither counts for nor resets
 * wofdm_rx_profile_kernel_ms. */
int wofdm_ldpc_decode(int device, int32_t J, int32_t L, int32_t max_iter, int32_t n,
                      const int32_t *perm,                  /* [n], or NULL */
                      int32_t n_cw,
                      const int8_t *soft,                   /* [n_cw][n] */
                      uint8_t *bits,                        /* [n_cw][n] */
                      int32_t *iters,                       /* [n_cw], or NULL */
                      uint8_t *converged);                  /* [n_cw], or NULL */

/* The coded link with LDPC codewords over the frame: wofdm_rx_profile_coded_frame's soft bits, frame interleaver (perm, sym_rot)
 * and random-coset view -- the transmitted codeword is all zero --, decoded by wofdm_ldpc_kernel.
 *   Codewords.  A point's frame has n_f = n_c S_d coded-stream positions behind the frame interleaver (S_d = S - 1, S - 2 with
 * post).  It carries W = ceil(n_f / WOFDM_LDPC_MAX_BITS) codewords of n = floor(n_f / W) positions each; codeword w holds the
 * coded-stream indices w n ... w n + n - 1 -- contiguous ranges, so every codeword sees every data symbol --, and the left-over
 * positions are ignored.  Every code of the call is lifted for this n.
 *   Arguments: every argument of wofdm_rx_profile_coded_frame through perm; n_codes (1 ... WOFDM_CODE_MAX) codes; sym_rot; the seven
 * outputs of wofdm_rx_profile_tracking, that call's bytes; ldpc_errs[point][cell][code] = {info-bit errors (x[v] != 0, J Z <= v <
 * n), codeword errors (any info bit wrong), unconverged codewords, iterations run}, ACCUMULATED into; soft_bits as in the coded
 * calls, the same bytes.
 *   Identities, by bytes: ldpc_errs depends neither on where a chunk ends, nor on the other points or codes of the call, nor on
 * whether soft_bits is requested; repeated calls are identical; it equals wofdm_ldpc_decode on the exported soft bits gathered
 * through the frame interleaver.
 *   Checks: wofdm_rx_profile_coded_frame's through perm and the size of soft_bits (codes NULL and n_codes in their places, no
 * rates), then in this order WOFDM_E_INVALID for sym_rot outside [0, n_c); for NULL ldpc_errs; then code by code for J, L,
 * max_iter outside their ranges, reserved != 0, K < 1 at an S_d in use, and (WOFDM_E_UNSUPPORTED, the same guard as the decoder's)
 * a decoder state beyond a workgroup's LDS.  Every argument is checked before the device is touched; a failed check leaves all
 * outputs as they were.
 *   Chunks: wofdm_rx_profile_coded's formula -- the decoder's state is in LDS.  One launch per code.
 *   A successful call holds the launch gate and counts for wofdm_rx_profile_kernel_ms.
 *   Measured: tools/bench_rx_profile_ldpc.py, profiles/rx_profile_ldpc.txt. */
int wofdm_rx_profile_ldpc(const wofdm_cfg *cfg, int device,
                          const float *w_tx,             /* [pairs][P] */
                          const float *w_rx,             /* [pairs][N+tail_rx] */
                          const float *h,                /* [n_channels][n_taps][2] */
                          const float *snr_db,           /* [n_snr] */
                          const uint8_t *active,         /* [n_fft] or NULL */
                          const float *tx_mask,          /* [2P-1] or NULL */
                          const float *h_track,          /* [n_tracks][n_channels][n_knots][n_taps][2], or NULL */
                          int32_t n_tracks, int32_t n_knots, int32_t knot_step,
                          const uint8_t *aci_active,     /* [n_fft], or NULL */
                          const float *aci_h,            /* [n_channels][n_taps][2], or NULL = h */
                          const float *ref_power,        /* [pairs], or NULL */
                          int32_t n_points, const wofdm_link_point *points,
                          int32_t n_scales, const float *scales,
                          const uint8_t *pilots,         /* [n_fft], or NULL */
                          const wofdm_tracking_point *tracking, /* [n_points] */
                          float llr_scale,
                          const int32_t *perm,           /* [n_c], or NULL */
                          int32_t n_codes, const wofdm_ldpc_code *codes,
                          int32_t sym_rot,               /* in [0, n_c) */
                          uint64_t *errs,                /* [n_points][cells][n_fft][2], ACCUMULATED into */
                          double *err_power,             /* [n_points][cells][n_fft], or NULL */
                          uint64_t *sym_errs,            /* [n_points][cells][S-1][2], or NULL */
                          double *sym_power,             /* [n_points][cells][S-1], or NULL */
                          double *pa_power,              /* [n_points][cells][2], or NULL */
                          double *bit_penalty,           /* [n_points][cells][n_scales][n_fft], ACCUMULATED into */
                          double *sym_penalty,           /* [n_points][cells][n_scales][S-1], or NULL */
                          uint64_t *ldpc_errs,           /* [n_points][cells][n_codes][4], ACCUMULATED into */
                          int8_t *soft_bits);            /* [cells][frames][n_points][S-1][n_fft][8], or NULL */

/* Random information words: the coded link without the all-zero view.
 *   The three coded calls above count a decoded 1 as an error: the Philox labels are the scrambler and the transmitted codeword
 * is all zero.  That is exact for a decoder that treats 0 and 1 alike, and neither of these does -- the Viterbi survivor is p0
 * unless p1 is STRICTLY smaller, the min-sum decoder counts t = 0 as positive and decides x = (Q < 0) --, so every tie and every
 * soft bit that is exactly 0 falls towards the transmitted word.  Here the transmitted word is random.
 *   Information stream.  A fifth Philox stream, 4 (WOFDM_STREAM_INFO of csrc/wofdm_link.h), beside the four of csrc/philox.h: block b of (seed, cell, frame) is
 * philox4x32_10 of counter (b, frame lo, frame hi, 4 << 28 | cell) under key (seed lo, seed hi), frame the global frame index as
 * in the other streams; bit i of the frame's stream is bit i mod 32 of word (i mod 128) div 32 of block i div 128.  The stream
 * depends neither on the point nor on the code: every point and every code of a call carries the same information, so they
 * compare pairwise, as labels and noise already do.  wofdm_coset_info (host only) writes bits 0 ... n_bits - 1 as bytes;
 * WOFDM_E_INVALID for NULL bits, n_bits < 0 or cell >= 2^28. */
int wofdm_coset_info(uint64_t seed, uint32_t cell, uint64_t frame, int32_t n_bits,
                     uint8_t *bits);                        /* [n_bits] */

/* The K = 7 encoder of wofdm_rx_profile_coded's code on the GPU: n_cw information words of T - 6 bits each (bytes; bit 0 counts), T
 * = wofdm_code_steps(rate, n_c); six zero tail steps are appended; coded[w][c] is the kept output with coded-stream index c, A
 * before B, punctured as defined there, and the left-over positions c >= the kept outputs' number are 0.  Every output is a parity
 * of seven information bits, so a lane takes one step and stores at the closed-form positions of its outputs; it equals the
 * Python mirror conv_encode bit for bit.  Checks, those of wofdm_viterbi_decode_long and before the device is touched:
 * WOFDM_E_INVALID for NULL info or coded, a rate outside {0, 1, 2}, n_c or n_cw < 1, T < 7; WOFDM_E_UNSUPPORTED for T >
 * WOFDM_CODE_LONG_MAX_STEPS.  The call holds the launch gate while its kernel runs; it neither counts for nor resets
 * wofdm_rx_profile_kernel_ms. */
int wofdm_conv_encode(int device, int32_t rate, int32_t n_c, int32_t n_cw,
                      const uint8_t *info,                  /* [n_cw][T - 6] */
                      uint8_t *coded);                      /* [n_cw][n_c] */

/* The encoder of the (J, L) code over n positions on the GPU: n_cw information words of K bits each (bytes; bit 0 counts) on
 * variables J Z ... n - 1, word[w][v] = x[v] for v < n.  Back-substitution from block row J - 1 up to 0: check r of row i XORs
 * x[j Z + (r + s(i, j)) mod Z] over j > i, and the result is variable i Z + (r + s(i, i)) mod Z.  One workgroup per word, the
 * word as bits in LDS, a row's Z checks strided over the threads, one barrier per row; it equals the Python mirror ldpc_encode bit
 * for bit.  Checks: wofdm_ldpc_decode's without max_iter and perm, in that order, before the device is touched.  The call holds
 * the launch gate while its kernel runs; it neither counts for nor resets wofdm_rx_profile_kernel_ms. */
int wofdm_ldpc_encode(int device, int32_t J, int32_t L, int32_t n, int32_t n_cw,
                      const uint8_t *info,                  /* [n_cw][K] */
                      uint8_t *word);                       /* [n_cw][n] */

/* Both decoders on random transmitted words, on the same frames: wofdm_rx_profile_coded_frame's and wofdm_rx_profile_ldpc's
 * frames, soft bits d, frame interleaver (perm, sym_rot), n_f, T, W, n and Z, with 0 ... WOFDM_CODE_MAX Viterbi codes and 0 ...
 * WOFDM_CODE_MAX LDPC codes, at least one in all.  The receive chain runs once for both families.
 *   Transmitted words.  A Viterbi code's word is the encoder's (wofdm_conv_encode) of the frame's stream bits 0 ... T - 7; LDPC word w
 * of a code carries stream bits w n ... w n + K - 1 on variables J Z ... n - 1 (wofdm_ldpc_encode).  The decoder for coded-stream
 * index c sees d' = x_c ? -d : d, x_c the transmitted coded bit (|d| <= 127: the negation is exact; left-over and shortened
 * positions have x = 0): the implied scrambler is label XOR x, and not a single frame changes.
 *   Counting.  Viterbi: an info-bit error is a decoded u_t != stream bit t, t < T - 6; a codeword error is any u_t wrong, the
 * tail checked against 0.  LDPC: info-bit errors are x[v] != the transmitted x[v] on J Z <= v < n, a codeword error any of them;
 * unconverged words and iterations as in wofdm_rx_profile_ldpc.
 *   Arguments: every argument of wofdm_rx_profile_coded_frame through perm; n_codes, codes; n_ldpc, ldpc_codes; sym_rot; the seven
 * outputs of wofdm_rx_profile_tracking, that call's bytes; frame_errs[point][cell][code] as wofdm_rx_profile_coded_frame's and
 * ldpc_errs[point][cell][code] as wofdm_rx_profile_ldpc's, ACCUMULATED into, each NULL exactly where its count is 0; soft_bits as
 * in the coded calls, the same bytes (d, not d').
 *   Fused: no codeword is ever in device memory.  The streaming Viterbi instantiation draws one Philox block per 128 steps, forms a
 * step's A and B from seven stream bits and XORs the traceback's 64-bit decision masks with the stream; the LDPC instantiation
 * draws its word's information bits, encodes them in LDS -- 4 ceil(L Z / 32) bytes beside the decoder's --, flips the signs
 * while it gathers and compares with the kept word at the end.  One launch per code.
 *   Identities, by bytes: the counters depend neither on where a chunk ends, nor on the other points or codes (of either family)
 * of the call, nor on whether soft_bits is requested; repeated calls are identical; they equal wofdm_viterbi_decode_long and
 * wofdm_ldpc_decode on the exported soft bits gathered through the frame interleaver and flipped by the transmitted words.
 *   Checks, in this order: wofdm_rx_profile_coded_frame's through perm and the size of soft_bits (llr_scale; perm; soft_bits), then
 * WOFDM_E_INVALID for n_codes or n_ldpc < 0; WOFDM_E_UNSUPPORTED for either above WOFDM_CODE_MAX; WOFDM_E_INVALID for both 0; for
 * NULL codes or ldpc_codes where the count is > 0; for sym_rot outside [0, n_c); for NULL frame_errs or ldpc_errs where the count
 * is > 0; then the Viterbi codes as wofdm_rx_profile_coded_frame checks them (rate, reserved; T < 7; T beyond the limit) and the
 * LDPC codes as wofdm_rx_profile_ldpc does, the LDS guard with the word's bits included.  Every argument is checked before the
 * device is touched; a failed check leaves all outputs as they were.
 *   Chunks: wofdm_rx_profile_coded_frame's formula, its history term only where n_codes > 0.
 *   A successful call holds the launch gate and counts for wofdm_rx_profile_kernel_ms.
 *   Measured: tools/bench_rx_profile_coset.py, profiles/rx_profile_coset.txt. */
int wofdm_rx_profile_coset(const wofdm_cfg *cfg, int device,
                           const float *w_tx,             /* [pairs][P] */
                           const float *w_rx,             /* [pairs][N+tail_rx] */
                           const float *h,                /* [n_channels][n_taps][2] */
                           const float *snr_db,           /* [n_snr] */
                           const uint8_t *active,         /* [n_fft] or NULL */
                           const float *tx_mask,          /* [2P-1] or NULL */
                           const float *h_track,          /* [n_tracks][n_channels][n_knots][n_taps][2], or NULL */
                           int32_t n_tracks, int32_t n_knots, int32_t knot_step,
                           const uint8_t *aci_active,     /* [n_fft], or NULL */
                           const float *aci_h,            /* [n_channels][n_taps][2], or NULL = h */
                           const float *ref_power,        /* [pairs], or NULL */
                           int32_t n_points, const wofdm_link_point *points,
                           int32_t n_scales, const float *scales,
                           const uint8_t *pilots,         /* [n_fft], or NULL */
                           const wofdm_tracking_point *tracking, /* [n_points] */
                           float llr_scale,
                           const int32_t *perm,           /* [n_c], or NULL */
                           int32_t n_codes, const wofdm_code *codes,
                           int32_t n_ldpc, const wofdm_ldpc_code *ldpc_codes,
                           int32_t sym_rot,               /* in [0, n_c) */
                           uint64_t *errs,                /* [n_points][cells][n_fft][2], ACCUMULATED into */
                           double *err_power,             /* [n_points][cells][n_fft], or NULL */
                           uint64_t *sym_errs,            /* [n_points][cells][S-1][2], or NULL */
                           double *sym_power,             /* [n_points][cells][S-1], or NULL */
                           double *pa_power,              /* [n_points][cells][2], or NULL */
                           double *bit_penalty,           /* [n_points][cells][n_scales][n_fft], ACCUMULATED into */
                           double *sym_penalty,           /* [n_points][cells][n_scales][S-1], or NULL */
                           uint64_t *frame_errs,          /* [n_points][cells][n_codes][2], ACCUMULATED into; NULL where n_codes = 0 */
                           uint64_t *ldpc_errs,           /* [n_points][cells][n_ldpc][4], ACCUMULATED into; NULL where n_ldpc = 0 */
                           int8_t *soft_bits);            /* [cells][frames][n_points][S-1][n_fft][8], or NULL */

/* Retransmissions with soft combining (HARQ, hybrid automatic repeat request): a word that does not decode is sent again, and the
 * receiver combines the attempts before it decodes.  The LDPC decoder's syndrome stop rule is the ACK.
 *   Groups.  rounds = R, 1 <= R <= WOFDM_HARQ_MAX_ROUNDS.  The frames of a cell are taken in groups of R consecutive GLOBAL frame
 * indices g R ... g R + R - 1; frames_per_cell and frame_offset must both be multiples of R.  Frame g R + r is transmission r + 1
 * of the group's words.  Every frame is exactly the frame every other entry point runs -- labels, noise, walk and channel of the
 * cell --: not a single frame changes.
 *   Transmitted word.  The group's information stream is wofdm_coset_info's of (seed, cell, frame g R), the group's FIRST frame;
 * LDPC word w of a code is formed from it exactly as in wofdm_rx_profile_coset (W, n, Z, K and the shortening unchanged), and
 * every transmission of the group carries the same x.  Transmission r reaches the decoder as d'_r[c] = x_c ? -d_r[c] : d_r[c], d_r
 * the soft bits of frame g R + r behind the frame interleaver.
 *   Decoder input at round r (0-based), formed in int32: combine = 1 (Chase combining) q[c] = clamp(sum over j <= r of d'_j[c],
 * -127, 127); combine = 0 (plain ARQ) q[c] = clamp(d'_r[c], -127, 127).  Shortened positions are 127.  The clamp keeps the
 * decoder's |Q| <= 128 + 6 * 95: there is still no saturation rule.
 *   Rounds.  Each round starts the decoder of wofdm_ldpc_decode afresh -- Q = q, R = 0 on every edge --, with up to max_iter
 * iterations.  The first round that converges (even syndrome) is the ACK: the word stops there and ignores its later frames.  A
 * word that never converges stops after round R with that round's decisions.
 *   The Viterbi codes are out of scope: without a CRC that decoder has no stop rule, so it cannot tell an ACK.
 *   Counters.  harq_errs[point][cell][code][WOFDM_HARQ_FIELDS], ACCUMULATED into: [0 ... 7] the words ACKed at round 1 ... 8
 * (entries >= R stay 0); [8] the words never ACKed; [9] the words with a wrong information bit at the stop (x[v] != the
 * transmitted x[v] on J Z <= v < n); [10] of those, the ACKed ones -- undetected errors --; [11] the information-bit errors at
 * the stop; [12] the iterations run over all rounds. */
#define WOFDM_HARQ_MAX_ROUNDS 8
#define WOFDM_HARQ_FIELDS 13

/* The combining decoder alone, with no flipping: the caller's soft bits are the d'.  Word w has the rows soft[w][0 ... rounds - 1],
 * variable c of row r read at soft[w][r][perm[c]] (NULL perm: the identity).  bits[w][v] = x[v] at the stop, round[w] the 1-based
 * stop round, iters[w] the iterations over all rounds, converged[w] 0 / 1; round, iters and converged may be NULL.
 *   Checks, all before the device is touched, in wofdm_ldpc_decode's order with rounds and combine behind max_iter:
 * WOFDM_E_INVALID for NULL soft or bits; J, L; max_iter; rounds outside 1 ... WOFDM_HARQ_MAX_ROUNDS; combine outside {0, 1}; n or
 * n_cw < 1; WOFDM_E_UNSUPPORTED for n > WOFDM_LDPC_MAX_BITS; WOFDM_E_INVALID for K < 1; WOFDM_E_UNSUPPORTED for a decoder state
 * beyond a workgroup's LDS (the guard of wofdm_rx_profile_coset, the word's bits included); WOFDM_E_INVALID for a perm that is no
 * permutation.  A failed check leaves the outputs as they were.  The call holds the launch gate while its kernel runs; it
 * neither counts for nor resets wofdm_rx_profile_kernel_ms. */
int wofdm_ldpc_harq_decode(int device, int32_t J, int32_t L, int32_t max_iter, int32_t n,
                           const int32_t *perm,             /* [n], or NULL */
                           int32_t n_cw, int32_t rounds, int32_t combine,
                           const int8_t *soft,              /* [n_cw][rounds][n] */
                           uint8_t *bits,                   /* [n_cw][n] */
                           int32_t *round,                  /* [n_cw], or NULL */
                           int32_t *iters,                  /* [n_cw], or NULL */
                           uint8_t *converged);             /* [n_cw], or NULL */

/* The coded link with retransmissions, on wofdm_rx_profile_coset's frames: the scheme above on the soft bits of every group.
 *   Arguments: every argument of wofdm_rx_profile_coset through perm; n_ldpc (1 ... WOFDM_CODE_MAX) ldpc_codes; sym_rot; rounds;
 * combine; the seven outputs of wofdm_rx_profile_tracking; harq_errs; soft_bits.  The tracking outputs and the exported soft bits
 * are the bytes of wofdm_rx_profile_coded_frame over all frames: the receive chain runs every frame, ACKed or not.
 *   wofdm_ldpc_harq_kernel: one workgroup per (group, point, word of the frame) and launch per code; LDS as the coset LDPC
 * decoder's, the word drawn and encoded once; each round re-forms q from the r + 1 rows of soft bits in device memory -- no
 * running sum is kept in LDS --, and the ACK is the workgroup's OR.
 *   Identities, by bytes: harq_errs depends neither on where a chunk ends, nor on the other points or codes of the call, nor on
 * whether soft_bits is requested; repeated calls are identical; a call over frames split at a multiple of R adds up to the call
 * over all; it equals wofdm_ldpc_harq_decode on the exported soft bits gathered through the frame interleaver and flipped by the
 * transmitted words of each group's first frame; with R = 1 and ldpc_errs = wofdm_rx_profile_coset's, [0] = words - ldpc_errs[2],
 * [8] = ldpc_errs[2], [9] = ldpc_errs[1], [11] = ldpc_errs[0], [12] = ldpc_errs[3].
 *   Checks, in this order: wofdm_rx_profile_coded_frame's through perm and the size of soft_bits, then WOFDM_E_INVALID for n_ldpc <
 * 0; WOFDM_E_UNSUPPORTED for n_ldpc > WOFDM_CODE_MAX; WOFDM_E_INVALID for n_ldpc = 0; for NULL ldpc_codes; for sym_rot outside
 * [0, n_c); for NULL harq_errs; for rounds outside 1 ... WOFDM_HARQ_MAX_ROUNDS; for combine outside {0, 1}; for a frames_per_cell,
 * then a frame_offset, that is no multiple of rounds; then the LDPC codes as wofdm_rx_profile_coset checks them.  Every argument
 * is checked before the device is touched; a failed check leaves all outputs as they were.
 *   Chunks: wofdm_rx_profile_ldpc's formula rounded down to a multiple of R, and R where that would be 0: a group never
 * straddles a chunk.
 *   A successful call holds the launch gate and counts for wofdm_rx_profile_kernel_ms.
 *   Measured: tools/bench_rx_profile_harq.py, profiles/rx_profile_harq.txt. */
int wofdm_rx_profile_harq(const wofdm_cfg *cfg, int device,
                          const float *w_tx,             /* [pairs][P] */
                          const float *w_rx,             /* [pairs][N+tail_rx] */
                          const float *h,                /* [n_channels][n_taps][2] */
                          const float *snr_db,           /* [n_snr] */
                          const uint8_t *active,         /* [n_fft] or NULL */
                          const float *tx_mask,          /* [2P-1] or NULL */
                          const float *h_track,          /* [n_tracks][n_channels][n_knots][n_taps][2], or NULL */
                          int32_t n_tracks, int32_t n_knots, int32_t knot_step,
                          const uint8_t *aci_active,     /* [n_fft], or NULL */
                          const float *aci_h,            /* [n_channels][n_taps][2], or NULL = h */
                          const float *ref_power,        /* [pairs], or NULL */
                          int32_t n_points, const wofdm_link_point *points,
                          int32_t n_scales, const float *scales,
                          const uint8_t *pilots,         /* [n_fft], or NULL */
                          const wofdm_tracking_point *tracking, /* [n_points] */
                          float llr_scale,
                          const int32_t *perm,           /* [n_c], or NULL */
                          int32_t n_ldpc, const wofdm_ldpc_code *ldpc_codes,
                          int32_t sym_rot,               /* in [0, n_c) */
                          int32_t rounds,                /* 1 ... WOFDM_HARQ_MAX_ROUNDS */
                          int32_t combine,               /* 1: Chase combining, 0: plain ARQ */
                          uint64_t *errs,                /* [n_points][cells][n_fft][2], ACCUMULATED into */
                          double *err_power,             /* [n_points][cells][n_fft], or NULL */
                          uint64_t *sym_errs,            /* [n_points][cells][S-1][2], or NULL */
                          double *sym_power,             /* [n_points][cells][S-1], or NULL */
                          double *pa_power,              /* [n_points][cells][2], or NULL */
                          double *bit_penalty,           /* [n_points][cells][n_scales][n_fft], ACCUMULATED into */
                          double *sym_penalty,           /* [n_points][cells][n_scales][S-1], or NULL */
                          uint64_t *harq_errs,           /* [n_points][cells][n_ldpc][WOFDM_HARQ_FIELDS], ACCUMULATED into */
                          int8_t *soft_bits);            /* [cells][frames][n_points][S-1][n_fft][8], or NULL */

/* Philox4x32-10 known-answer hook (runs one block on the GPU). */
int wofdm_philox_kat(int device, const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);

#ifdef __cplusplus
}
#endif
#endif
