// wofdm_abi.hip -- extern "C" boundary of libwofdm_hip.so (declared in include/wofdm.h).
// Plans own the constants in HBM; launches are asynchronous on the caller's stream.
#include "../../include/wofdm.h"
#include "wofdm_kernel.h"
#include "wofdm_link.h"
#include "philox.h"

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <utility>
#include <vector>

namespace {

thread_local char g_err[512] = "";
thread_local float g_papr_ms = 0.f;    // wofdm_tx_papr_kernel_ms
thread_local float g_rxprof_ms = 0.f;  // wofdm_rx_profile_kernel_ms

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(e_ == hipErrorOutOfMemory ? WOFDM_E_NOMEM : WOFDM_E_HIP, "%s: %s",    \
                        #expr, hipGetErrorString(e_));                                        \
    } while (0)

struct geom {
    int N, k, S, mu, rho, beta, delta, gamma, kappa, L, P, B, T, NL;
};

int check_cfg(const wofdm_cfg *c, geom *g)
{
    if (!c) return fail(WOFDM_E_INVALID, "cfg is NULL");
    const int N = c->n_fft;
    if (N != 64 && N != 128 && N != 256 && N != 512 && N != 1024)
        return fail(WOFDM_E_UNSUPPORTED, "n_fft=%d not in {64,128,256,512,1024}", N);
    if (c->bits_per_sc != 2 && c->bits_per_sc != 4 && c->bits_per_sc != 6)
        return fail(WOFDM_E_UNSUPPORTED, "bits_per_sc=%d not in {2,4,6}", c->bits_per_sc);
    if (c->syms_per_frame < 2 || c->syms_per_frame > WOFDM_MAX_SYMS)
        return fail(WOFDM_E_UNSUPPORTED, "syms_per_frame=%d not in [2,%d]", c->syms_per_frame,
                    WOFDM_MAX_SYMS);
    if (c->n_taps < 1 || c->n_taps > WOFDM_MAX_TAPS)
        return fail(WOFDM_E_UNSUPPORTED, "n_taps=%d not in [1,%d]", c->n_taps, WOFDM_MAX_TAPS);
    if (c->cp < 0 || c->cs < 0 || c->tail_tx < 0 || c->tail_rx < 0 || (c->tail_rx & 1) ||
        c->prefix_rm < 0 || c->circ_shift < 0 || c->circ_shift >= N)
        return fail(WOFDM_E_INVALID, "negative length, odd tail_rx or circ_shift >= n_fft");
    if (c->cp > N || c->cs > N || c->tail_rx > N)
        return fail(WOFDM_E_INVALID, "cp, cs and tail_rx must not exceed n_fft");
    if (c->n_channels < 1 || c->n_snr < 1 || c->n_window_pairs < 1)
        return fail(WOFDM_E_INVALID, "n_channels, n_snr, n_window_pairs must be >= 1");
    g->N = N; g->k = c->bits_per_sc; g->S = c->syms_per_frame;
    g->mu = c->cp; g->rho = c->cs; g->beta = c->tail_tx; g->delta = c->tail_rx;
    g->gamma = c->prefix_rm; g->kappa = c->circ_shift; g->L = c->n_taps;
    g->P = N + g->mu + g->rho; g->B = g->P - g->beta; g->T = g->beta + g->S * g->B;
    g->NL = c->noise_before_truncate ? g->T + g->L - 1 : g->S * g->B;
    if (2 * g->beta > g->P) return fail(WOFDM_E_INVALID, "2*tail_tx exceeds the symbol length");
    // the Rx reshape of matlab/main_BER_calculation.m:262-263 needs B == N + delta + gamma
    if (g->B != N + g->delta + g->gamma)
        return fail(WOFDM_E_INVALID, "n_fft+cp+cs-tail_tx (%d) != n_fft+tail_rx+prefix_rm (%d)",
                    g->B, N + g->delta + g->gamma);
    if (g->mu + g->rho > wofdm_cpcs_max(N) || g->beta > 16 || g->delta > 64)
        return fail(WOFDM_E_UNSUPPORTED, "kernel limits: cp+cs <= %d, tail_tx <= 16, tail_rx <= 64",
                    wofdm_cpcs_max(N));
    if (g->B > 64 * wofdm_rb(N))
        return fail(WOFDM_E_UNSUPPORTED, "cp+cs-tail_tx=%d exceeds the 64 samples the kernel's "
                    "FIR tiling allows", g->B - N);
    const uint64_t cells = (uint64_t)c->n_channels * c->n_snr * c->n_window_pairs;
    if (cells >= (1u << 28)) return fail(WOFDM_E_UNSUPPORTED, "more than 2^28 cells");
    return WOFDM_OK;
}

}  // namespace

struct wofdm_plan {
    int device = 0;
    wofdm_cfg cfg{};
    geom g{};
    uint32_t n_cells = 0;
    float *d_wtx = nullptr, *d_wrx = nullptr, *d_nlin = nullptr;
    float2 *d_h = nullptr;
    int *d_geo = nullptr;
    float2 *d_nscr = nullptr;          // unit-noise scratch rows, one per workgroup (large DFTs)
    uint64_t nscr_elems = 0;           // float2 elements allocated there
    wofdm_kparams base{};
    wofdm_kernel_fn fn[4] = {nullptr, nullptr, nullptr, nullptr};   // kernels of the variant in use
    int var = WOFDM_VAR_PLAIN;         // kernel variant in use (configure())
    bool has_alloc = false, has_mask = false;
    // wofdm_plan_set_option: diagnostic kernel choice
    bool force_direct_mask = false;    // WOFDM_OPT_TXMASK_DIRECT: never the FFT form
    bool fir_valu = false;             // WOFDM_OPT_FIR_VALU: FIR on the VALU in every layout
    bool dft_valu = false;             // WOFDM_OPT_DFT_VALU: N = 256 transforms on the VALU (layouts 6, 7 instead of 10, 11)
    int max_spw = 0;                   // WOFDM_OPT_MAX_SPW: 0 = no cap
    bool generic_geo = false;          // WOFDM_OPT_GENERIC_GEOMETRY: never a kernel with the geometry built in
    int geo = 0;                       // id of the built geometry of fn[WOFDM_MODE_GEN] (wofdm_geo_table); 0: geometry at run time
    uint32_t *d_amask = nullptr;       // [N/4] words, byte r bit 7: subcarrier j + r N/4 not loaded
    float2 *d_tmask = nullptr;         // [2P-1] circular impulse response of the Tx mask
    float2 *d_tspec = nullptr;         // [WOFDM_TXFFT_LEN] its fast-convolution spectrum (FFT form)
    float *d_tspec4 = nullptr;         // the same x 2^4 in layout 15's order: [kc][re | im][lane][j] <-> bin lane + 64 j + 256 kc
    unsigned *d_status = nullptr;      // kernel status word (wofdm_kparams::status)
    unsigned long long *d_work = nullptr;   // work counter of the launch in flight (wofdm_kparams::work)
    // wofdm_work_split's share of the static heads and the chunk of the tail (developer override: WOFDM_SPLIT_ALPHA, a fraction
    // in [0, 1), and WOFDM_SPLIT_CHUNK, read when the plan is created; tools/README.md)
    uint32_t split_alpha_256 = WOFDM_SPLIT_ALPHA_256, split_chunk = WOFDM_SPLIT_CHUNK;
    bool split_forced = false;         // either of them given: every launch with more items than workgroups has a tail
    uint4 *d_fira = nullptr;           // [n_ch][4][64] Toeplitz operands of the matrix-pipe FIR (MFMA A layout)
    float firm_sx = 1.f, firm_sh = 1.f; // powers of two carried by the f16 samples / f16 taps there
    uint4 *d_dftc = nullptr;           // [10][64] operands of the matrix-pipe 256-point transforms (build_dftc)
    float *d_rxs = nullptr;            // [n_snr][n_ch] power of two that centres the received samples in the f16 range
#ifdef WOFDM_AUDIT
    uint32_t *audit = nullptr;
    uint32_t audit_items = 0;
#endif
    int occ = 1, cus = 1, layout = 1;  // layout id of the kernels in use (wofdm_pick_layout)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

namespace {

// words of the allocation table (wofdm_plan_set_allocation: N/4 in the plain order, then the layouts' own orders)
size_t wofdm_amask_words(int N)
{
    const size_t NQ = (size_t)N / 4;
    return N == 256 ? 2 * NQ + 256 : NQ + (NQ > 256 ? NQ : 256);
}

// id of the geometry in wofdm_geo_table (every field equal), else 0
int geo_id_of(const geom &g)
{
    return wofdm_geo_id(wofdm_geo_row{g.N, g.S, g.mu, g.rho, g.beta, g.delta, g.gamma, g.kappa, g.L, g.P, g.B, g.T, g.NL});
}

// Select the kernel variant from the plan's options and size everything that depends on it
// (symbols per wave, LDS bytes, frame buffer length, occupancy).  Plan state changes only on success.
int configure(wofdm_plan *pl)
{
    const geom &g = pl->g;
    // the mask runs as fast convolution where its transform length allows, else in direct form
    const bool fft_ok = g.N <= WOFDM_TXFFT_MAX_N && 3 * g.P - 2 <= WOFDM_TXFFT_LEN && !pl->force_direct_mask;
    const int var = pl->has_mask ? (fft_ok ? WOFDM_VAR_TXFFT : WOFDM_VAR_TXMASK)
                                 : (pl->has_alloc ? WOFDM_VAR_ALLOC : WOFDM_VAR_PLAIN);
    const bool masked = var == WOFDM_VAR_TXMASK || var == WOFDM_VAR_TXFFT;
    const bool firm = !pl->fir_valu;
    const bool mdft = !pl->dft_valu;
    int layout = masked ? wofdm_pick_layout_masked(g.N, g.B, firm) : wofdm_pick_layout(g.N, g.S, g.B, true, firm, mdft);
    // (layout 15: the fast-convolution mask at N = 256 with all four transforms on the matrix pipe)
    if (var == WOFDM_VAR_TXFFT && g.N == 256 && layout == 9 && mdft && WOFDM_TXFFT_LEN == 1024) layout = 15;
    if (pl->max_spw > 0 && wofdm_layout_info(layout, g.N).spw > pl->max_spw)
        layout = (pl->max_spw == 1) ? 1 : wofdm_pick_layout(g.N, g.S, g.B, false);
    // (WOFDM_DEV_LDS_PAD: developer builds only -- unused LDS bytes per workgroup, to measure how the rate depends on the
    // number of workgroups a CU holds; never defined in the shipped library)
#ifndef WOFDM_DEV_LDS_PAD
#define WOFDM_DEV_LDS_PAD 0
#endif
    const auto lds_of = [&](int lay) {
        return wofdm_lds_bytes(g.N, g.T, lay, g.S, g.B)
               + (var == WOFDM_VAR_TXMASK ? wofdm_txmask_lds_bytes(g.N) : 0u)
               + (var == WOFDM_VAR_TXFFT && lay != 15 ? wofdm_txfft_lds_bytes() : 0u) + (unsigned)(WOFDM_DEV_LDS_PAD);
    };
    // (layouts 8 / 12 pitch their LDS rows by (B + 3) & ~3 words: at N = 1024 a stride that is no multiple of four can need more
    // than the 160 KiB where the VALU kernel with one symbol per wave, which keeps the frame as it is on air, still fits)
    if (!masked && layout != 1 && wofdm_layout_info(layout, g.N).fir == WOFDM_FIR_ONE && lds_of(layout) > 160u * 1024u
        && lds_of(1) <= 160u * 1024u)
        layout = 1;
    const unsigned lds = lds_of(layout);
    if (lds > 160u * 1024u)
        return fail(WOFDM_E_UNSUPPORTED, "frame needs %u bytes of LDS (160 KiB per workgroup)", lds);
    wofdm_kernel_fn fn[4];
    for (int m = 0; m < 4; ++m) {
        fn[m] = wofdm_select_kernel(g.N, g.k, layout, m, var);
        if (!fn[m])
            return fail(WOFDM_E_UNSUPPORTED, "no kernel for n_fft=%d bits_per_sc=%d variant %d%s", g.N, g.k,
                        var, masked ? " (the Tx mask needs n_fft <= 512)" : "");
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(fn[m]),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    // Generate mode of a plain plan whose geometry is a row of wofdm_geo_table: the kernel with that row's lengths built in (the
    // same statements on the same operands, so the same counters; WOFDM_OPT_GENERIC_GEOMETRY keeps the generic kernel).  Injected,
    // instrumented, allocation and masked plans keep the generic kernels.
    int geo = 0;
    if (var == WOFDM_VAR_PLAIN && (layout == 10 || layout == 11) && !pl->generic_geo) {
        geo = geo_id_of(g);
        if (geo && wofdm_geo_layout(geo) != layout) geo = 0;
        if (geo && !wofdm_geo_unit_matches(g.N, g.k)) geo = 0;      // (the generic unit is another build of the source: its kernels run)
    }
    if (geo) {
        fn[WOFDM_MODE_GEN] = wofdm_select_kernel_geo(g.N, g.k, geo);
        if (!fn[WOFDM_MODE_GEN])
            return fail(WOFDM_E_UNSUPPORTED, "no kernel for the built geometry %d at n_fft=%d bits_per_sc=%d", geo, g.N, g.k);
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(fn[WOFDM_MODE_GEN]),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    int occ = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &occ, reinterpret_cast<const void *>(fn[WOFDM_MODE_GEN]), 64 * wofdm_waves(layout, g.N, g.S, g.B), lds));
    if (occ < 1) return fail(WOFDM_E_UNSUPPORTED, "kernel does not fit a CU (LDS %u bytes)", lds);
    // (the LDS goes in units of 1 280 bytes (WOFDM_LDS_GRANULE), which the occupancy API does not know: wofdm_lds_workgroups_per_cu)
    if (occ > wofdm_lds_workgroups_per_cu(lds)) occ = wofdm_lds_workgroups_per_cu(lds);
    const int fbuf = wofdm_fbuf_len(g.N, g.T, layout, g.S, g.B);
    HIP_TRY(hipMemcpy(pl->d_geo + WOFDM_G_FBUF, &fbuf, sizeof(int), hipMemcpyHostToDevice));
    const int spwr = wofdm_spwr(layout, g.N, g.S, g.B);
    HIP_TRY(hipMemcpy(pl->d_geo + WOFDM_G_SPWR, &spwr, sizeof(int), hipMemcpyHostToDevice));
    for (int m = 0; m < 4; ++m) pl->fn[m] = fn[m];
    pl->var = var; pl->layout = layout; pl->geo = geo; pl->occ = occ; pl->base.lds_bytes = lds;
    // scale of the on-air samples inside the kernel (wofdm_kparams): 1/N of the IDFT, times the
    // f16 centring of the matrix-pipe layouts
    const bool fm = wofdm_layout_info(layout, g.N).fir != WOFDM_FIR_VALU;
    pl->base.tx_scale = (fm ? pl->firm_sx : 1.0f) / (float)g.N;
    pl->base.dump_unscale_tx = fm ? 1.0f / pl->firm_sx : 1.0f;
    pl->base.dump_unscale_rx = fm ? 1.0f / (pl->firm_sx * pl->firm_sh) : 1.0f;
    return WOFDM_OK;
}

// Host transforms for the masks of wofdm_tx_psd_batch_masked, fp64, O(M log M).  fft_pow2: in place, sign = -1 forward,
// +1 inverse (unnormalised), twiddles straight from cos / sin.
using cplx = std::complex<double>;
void fft_pow2(std::vector<cplx> &a, int sign)
{
    const size_t n = a.size();
    for (size_t i = 1, j = 0; i < n; ++i) {
        size_t bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) std::swap(a[i], a[j]);
    }
    std::vector<cplx> w(n / 2 ? n / 2 : 1);
    for (size_t k = 0; k < n / 2; ++k) {
        const double ang = sign * 2.0 * M_PI * (double)k / (double)n;
        w[k] = cplx(std::cos(ang), std::sin(ang));
    }
    for (size_t len = 2; len <= n; len <<= 1) {
        const size_t half = len / 2, step = n / len;
        for (size_t i = 0; i < n; i += len)
            for (size_t k = 0; k < half; ++k) {
                const cplx u = a[i + k], v = a[i + k + half] * w[k * step];
                a[i + k] = u + v;
                a[i + k + half] = u - v;
            }
    }
}

// g = IDFT_L(mask) for any L (Bluestein: k n = (k^2 + n^2 - (n - k)^2) / 2, chirp e^{i pi k^2 / L} from k^2 mod 2 L)
std::vector<cplx> idft_any(const float *mask, int L)
{
    size_t Mb = 1;
    while (Mb < (size_t)(2 * L - 1)) Mb <<= 1;
    std::vector<cplx> c((size_t)L), a(Mb, cplx(0.0, 0.0)), b(Mb, cplx(0.0, 0.0));
    for (int k = 0; k < L; ++k) {
        const double ang = M_PI * (double)(((long long)k * k) % (2LL * L)) / (double)L;
        c[(size_t)k] = cplx(std::cos(ang), std::sin(ang));
    }
    for (int k = 0; k < L; ++k) a[(size_t)k] = (double)mask[k] * c[(size_t)k];
    b[0] = std::conj(c[0]);
    for (int k = 1; k < L; ++k) b[(size_t)k] = b[Mb - (size_t)k] = std::conj(c[(size_t)k]);
    fft_pow2(a, -1);
    fft_pow2(b, -1);
    for (size_t i = 0; i < Mb; ++i) a[i] *= b[i];
    fft_pow2(a, +1);
    std::vector<cplx> g((size_t)L);
    for (int n = 0; n < L; ++n) g[(size_t)n] = a[(size_t)n] * c[(size_t)n] / ((double)Mb * (double)L);
    return g;
}

// Fast-convolution spectrum of a mask of L = 2 P - 1 gains (the recipe of wofdm_plan_set_tx_mask): FFT_MF of
// gt[t] = g[(t - (P-1)) mod L], t < 3 P - 2 <= MF, with the 1 / MF of the inverse transform folded in; rounded to fp32
// only when stored.
void mask_fastconv_spectrum(const float *mask, int L, int MF, float2 *spec)
{
    const int P = (L + 1) / 2, G = 3 * P - 2;
    const std::vector<cplx> g = idft_any(mask, L);
    std::vector<cplx> gt((size_t)MF, cplx(0.0, 0.0));
    for (int t = 0; t < G && t < MF; ++t) gt[(size_t)t] = g[(size_t)(((t - (P - 1)) % L + L) % L)];
    fft_pow2(gt, -1);
    for (int f = 0; f < MF; ++f)
        spec[f] = make_float2((float)(gt[(size_t)f].real() / MF), (float)(gt[(size_t)f].imag() / MF));
}

// The gate of launch() below: one mutex and one "last launch" event per device for the whole process.  The two synchronous
// entry points that launch kernels of their own (wofdm_interference, wofdm_tx_psd: kernels WITH swizzled packed arithmetic)
// hold the mutex from their device synchronisation to the end of their kernels, so that no frame launch of another thread
// can slip in beside them.
std::mutex g_gate_mu;
hipEvent_t g_gate_last[64] = {};

int launch(wofdm_plan *pl, int mode, wofdm_kparams &kp, uint64_t total_items, int force_grid,
           hipStream_t stream)
{
    wofdm_kernel_fn fn = pl->fn[mode];
    if (!fn) return fail(WOFDM_E_UNSUPPORTED, "no kernel for n_fft=%d", pl->g.N);
    if (total_items == 0) return WOFDM_OK;
    uint64_t grid = (uint64_t)pl->cus * (uint64_t)pl->occ;
#ifdef WOFDM_DEV_OCC               // developer builds only: workgroups launched per CU (occupancy experiments)
    grid = (uint64_t)pl->cus * (uint64_t)(WOFDM_DEV_OCC);
#endif
    if (grid > total_items) grid = total_items;
    if (force_grid > 0) grid = (uint64_t)force_grid;
    const size_t row = wofdm_noise_scratch_len(pl->g.N, pl->layout);
    if (row && grid * row > pl->nscr_elems) {       // only a forced grid can outgrow the plan's scratch
        HIP_TRY(hipDeviceSynchronize());
        if (pl->d_nscr) (void)hipFree(pl->d_nscr);
        pl->d_nscr = nullptr; pl->nscr_elems = 0;
        HIP_TRY(hipMalloc(&pl->d_nscr, grid * row * sizeof(float2)));
        pl->nscr_elems = grid * row;
    }
    kp.noise_scratch = pl->d_nscr;
    kp.status = pl->d_status;
    kp.dftc = pl->d_dftc;
    kp.rx_scale = pl->d_rxs;
    const bool dynamic = (mode == WOFDM_MODE_GEN || mode == WOFDM_MODE_INJECT) && wofdm_layout_dynamic(pl->layout, pl->g.N)
                         && (pl->split_forced || (pl->occ >= 2 && total_items / grid >= WOFDM_SPLIT_MIN_ITEMS));
    const wofdm_split sp = wofdm_work_split(total_items, grid, dynamic, pl->split_alpha_256, pl->split_chunk);
    kp.head_q = sp.head_q; kp.head_r = sp.head_r; kp.tail0 = sp.tail0; kp.total = total_items;
    kp.chunk = sp.chunk;
    kp.work = pl->d_work;
    kp.lds_bytes = pl->base.lds_bytes;
    float2 *tm = pl->var == WOFDM_VAR_TXFFT ? (pl->layout == 15 ? reinterpret_cast<float2 *>(pl->d_tspec4) : pl->d_tspec) : pl->d_tmask;
    kp.tx_scale = pl->base.tx_scale;
    kp.dump_unscale_tx = pl->base.dump_unscale_tx;
    kp.dump_unscale_rx = pl->base.dump_unscale_rx;
#ifdef WOFDM_AUDIT
    kp.audit = pl->audit; kp.audit_items = pl->audit_items;
#endif
#ifdef WOFDM_DELAY
    {
        const char *dp = std::getenv("WOFDM_DELAY_POINT"), *dw = std::getenv("WOFDM_DELAY_WAVES"), *dn = std::getenv("WOFDM_DELAY_LEN");
        kp.delay_point = dp ? (uint32_t)std::strtoul(dp, nullptr, 0) : 0;
        kp.delay_waves = dw ? (uint32_t)std::strtoul(dw, nullptr, 0) : 0;
        kp.delay_len = dn ? (uint32_t)std::strtoul(dn, nullptr, 0) : 8;
    }
#endif
    void *args[] = {&kp, &pl->d_wtx, &pl->d_wrx, &pl->d_h, &pl->d_nlin, &pl->d_geo, &pl->d_amask, &tm,
                    &pl->d_fira};
    // One frame kernel at a time per device, whatever streams the callers use: the kernels of layouts 10 / 11 / 12 issue MFMAs
    // in a rhythm that corrupts op_sel-swizzled packed arithmetic of OTHER waves on their SIMDs (wofdm_kernel.hip, mma33);
    // they hold no such instruction themselves, every other kernel of the library does.  Each launch waits for the
    // previous launch of this process on the device (an event; free when it is the same stream) -- a kernel fills the GPU
    // on its own, so nothing is lost.
    // (What the library can NOT order is work it does not launch: kernels of the caller's own -- torch, rocBLAS, RCCL -- on other
    // streams of the device, or another process's.  include/wofdm.h and INTEGRATION.md state the requirement: nothing else runs
    // on the device while a launch of layouts 10 ... 16 (transforms on the matrix pipe: wofdm_layout_info) is in flight, or the
    // plan is switched to the VALU transforms -- option dft_valu, whose kernels issue one cache-line-aligned chain at a time:
    // hazard 1's safe shape.)
    {
        std::lock_guard<std::mutex> lock(g_gate_mu);
        hipEvent_t *last = g_gate_last;
        const int dev = pl->device & 63;
        if (last[dev]) HIP_TRY(hipStreamWaitEvent(stream, last[dev], 0));
        else HIP_TRY(hipEventCreateWithFlags(&last[dev], hipEventDisableTiming));
        // (the work counter is the plan's: zeroed behind the previous launch, whichever stream that ran on)
        if (kp.tail0 < kp.total) HIP_TRY(hipMemsetAsync(pl->d_work, 0, sizeof(unsigned long long), stream));
        HIP_TRY(hipLaunchKernel(reinterpret_cast<const void *>(fn), dim3((unsigned)grid),
                                dim3(64u * (unsigned)wofdm_waves(pl->layout, pl->g.N, pl->g.S, pl->g.B)), args, kp.lds_bytes, stream));
        HIP_TRY(hipEventRecord(last[dev], stream));
    }
    return WOFDM_OK;
}

// After a synchronisation: has any kernel of this plan reported a problem?
int check_status(wofdm_plan *pl)
{
    unsigned st = 0;
    HIP_TRY(hipMemcpy(&st, pl->d_status, sizeof st, hipMemcpyDeviceToHost));
    if (st != 0)
        return fail(WOFDM_E_HIP, "kernel status 0x%x: a wave timed out waiting for its workgroup "
                    "(results must not be used)", st);
    return WOFDM_OK;
}

int check_launch_args(wofdm_plan *pl, uint64_t frames_per_cell)
{
    if (!pl) return fail(WOFDM_E_INVALID, "plan is NULL");
    if (frames_per_cell > (1ull << 40)) return fail(WOFDM_E_INVALID, "frames_per_cell too large");
    return WOFDM_OK;
}

// ---- the auxiliary entry points (wofdm_interference*, wofdm_tx_psd*, wofdm_tx_papr, wofdm_rx_profile*) ----

// Owner of a device allocation: whichever way its entry point returns, everything is freed.
template <typename T> struct dev_buf {
    T *p = nullptr;
    dev_buf() = default;
    dev_buf(dev_buf &&o) noexcept : p(o.p) { o.p = nullptr; }      // (move-only: the copy operations are deleted with it)
    ~dev_buf() { if (p) (void)hipFree(p); }
    bool alloc(size_t count) { return hipMalloc(&p, count * sizeof(T)) == hipSuccess; }
    bool upload(const void *host, size_t count) { return hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice) == hipSuccess; }
    operator T *() const { return p; }
};

// the device an auxiliary entry point runs on, made current
int use_device(int device)
{
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev)
        return fail(WOFDM_E_HIP, "device %d not available (%d visible); there is no CPU fallback", device, ndev);
    HIP_TRY(hipSetDevice(device));
    return WOFDM_OK;
}

// The checks of a table of amplifier points (include/wofdm.h, both routes), and the points as the kernels read them
int check_pa_points(int32_t n, const wofdm_pa_point *pts, std::vector<wofdm_papoint> *out)
{
    if (n > WOFDM_PA_MAX_POINTS) return fail(WOFDM_E_UNSUPPORTED, "%d amplifier points exceed %d", n, WOFDM_PA_MAX_POINTS);
    out->resize((size_t)(n > 0 ? n : 0));
    for (int i = 0; i < n; ++i) {
        const wofdm_pa_point &q = pts[i];
        if (!std::isfinite(q.ibo_db) || !std::isfinite(q.smooth))
            return fail(WOFDM_E_INVALID, "amplifier point %d: ibo_db and smooth must be finite", i);
        if (q.reserved != 0) return fail(WOFDM_E_INVALID, "amplifier point %d: reserved=%d must be 0", i, q.reserved);
        if (q.model != WOFDM_PA_LINEAR && q.model != WOFDM_PA_RAPP && q.model != WOFDM_PA_CLIP)
            return fail(WOFDM_E_UNSUPPORTED, "amplifier point %d: model %d is not known", i, q.model);
        if (q.ibo_db < -40.f || q.ibo_db > 60.f)
            return fail(WOFDM_E_UNSUPPORTED, "amplifier point %d: ibo_db=%g outside [-40, 60]", i, (double)q.ibo_db);
        if (q.model == WOFDM_PA_RAPP && (q.smooth < 0.5f || q.smooth > 16.f))
            return fail(WOFDM_E_UNSUPPORTED, "amplifier point %d: smooth=%g outside [0.5, 16]", i, (double)q.smooth);
        const double p2 = q.model == WOFDM_PA_RAPP ? 2.0 * (double)q.smooth : 2.0;
        (*out)[(size_t)i] = {q.model, (float)p2, (float)(1.0 / p2), 0};
    }
    return WOFDM_OK;
}

// the channels' taps as the kernels read them: [n_channels][WOFDM_LT] float2, zero padded
std::vector<float2> pack_taps(const wofdm_cfg *cfg, const geom &g, const float *h)
{
    std::vector<float2> hp((size_t)cfg->n_channels * WOFDM_LT, make_float2(0.f, 0.f));
    for (int c = 0; c < cfg->n_channels; ++c)
        for (int l = 0; l < g.L; ++l)
            hp[(size_t)c * WOFDM_LT + l] = make_float2(h[2 * ((size_t)c * g.L + l)], h[2 * ((size_t)c * g.L + l) + 1]);
    return hp;
}

// ---- what wofdm_tx_papr and the receive profiles share: the Tx chain of a chunk of frames, and the loop over a call's chunks ----

// The frames of a Tx chain: P samples a symbol, B = P - tail_tx from one symbol to the next, T samples a frame; Lm taps of the
// mask's circular impulse response, FL points of its fast convolution
struct tx_geom {
    int N, k, S, P, beta, B, T, Lm, FL;
};
tx_geom tx_geom_of(const wofdm_cfg *cfg)
{
    tx_geom g{};
    g.N = cfg->n_fft; g.k = cfg->bits_per_sc; g.S = cfg->syms_per_frame;
    g.P = g.N + cfg->cp + cfg->cs; g.beta = cfg->tail_tx; g.B = g.P - g.beta; g.T = g.beta + g.S * g.B;
    g.Lm = 2 * g.P - 1; g.FL = 8 * g.N;
    return g;
}

// The Tx chain's checks, each refusal in its one wording; a caller makes them in the order its header documents.
int check_tx_grid(const wofdm_cfg *cfg)
{
    const int N = cfg->n_fft, k = cfg->bits_per_sc, S = cfg->syms_per_frame;
    if (N != 64 && N != 128 && N != 256 && N != 512 && N != 1024)
        return fail(WOFDM_E_UNSUPPORTED, "n_fft=%d not in {64,128,256,512,1024}", N);
    if (k != 2 && k != 4 && k != 6) return fail(WOFDM_E_UNSUPPORTED, "bits_per_sc=%d not in {2,4,6}", k);
    if (S < 2 || S > WOFDM_MAX_SYMS) return fail(WOFDM_E_UNSUPPORTED, "syms_per_frame=%d not in [2,%d]", S, WOFDM_MAX_SYMS);
    return WOFDM_OK;
}
// (the two callers refuse a symbol that does not fit in words of their own)
bool tx_symbol_fits(const wofdm_cfg *cfg, const tx_geom &g) { return cfg->cp <= g.N && cfg->cs <= g.N && 2 * g.beta <= g.P; }
int check_mask_length(const float *tx_mask, const tx_geom &g)
{
    if (tx_mask && g.P > wofdm_txmask_batch_pmax(g.N))
        return fail(WOFDM_E_UNSUPPORTED, "the Tx mask needs 3 P - 2 <= 8 n_fft, i.e. P = n_fft + cp + cs <= %d at n_fft = %d (P = %d)",
                    wofdm_txmask_batch_pmax(g.N), g.N, g.P);
    return WOFDM_OK;
}
int check_mask_gains(const float *tx_mask, const tx_geom &g)
{
    for (int i = 0; tx_mask && i < g.Lm; ++i)
        if (!std::isfinite(tx_mask[i])) return fail(WOFDM_E_INVALID, "mask gains must be finite");
    return WOFDM_OK;
}
// the allocation as the kernels read it, 0 / 1 per bin (no allocation: hact stays empty, every bin is loaded)
int check_allocation(const uint8_t *active, int N, std::vector<uint8_t> *hact)
{
    if (!active) return WOFDM_OK;
    hact->resize((size_t)N);
    int n_act = 0;
    for (int n = 0; n < N; ++n) n_act += ((*hact)[(size_t)n] = active[n] ? 1 : 0);
    return n_act ? WOFDM_OK : fail(WOFDM_E_INVALID, "the allocation loads no subcarrier");
}

// What the Tx chains of a call share on the device: the Tx windows, and the spectrum of the mask's fast convolution
struct tx_shared {
    dev_buf<float> w;
    dev_buf<float2> spec;
    int stage(const float *w_tx, size_t n_w, const float *tx_mask, const tx_geom &g)
    {
        std::vector<float2> hspec;
        if (tx_mask) {
            hspec.resize((size_t)g.FL);
            mask_fastconv_spectrum(tx_mask, g.Lm, g.FL, hspec.data());
        }
        if (!w.alloc(n_w) || (tx_mask && !spec.alloc(hspec.size()))) return fail(WOFDM_E_NOMEM, "device allocation failed");
        if (!w.upload(w_tx, n_w) || (tx_mask && !spec.upload(hspec.data(), hspec.size()))) return fail(WOFDM_E_HIP, "upload failed");
        return WOFDM_OK;
    }
};
// One Tx chain's device side: its allocation, and of a chunk's frames the symbol grids, the waveforms, under a mask the filtered
// symbols, and the job tables
struct tx_chain {
    dev_buf<uint8_t> act;
    dev_buf<float2> X, x, Y;
    dev_buf<wofdm_bjob> jobs;
    dev_buf<wofdm_mjob> mjobs;
    // syms: the symbols of a frame (the neighbour has one more than g.S); whose: what the refusal adds to "allocation failed"
    int stage(const tx_geom &g, int syms, size_t chunk, const std::vector<uint8_t> &hact, bool masked, const char *whose)
    {
        if (!X.alloc(chunk * syms * g.N) || !x.alloc(chunk * (g.beta + (size_t)syms * g.B)) || !jobs.alloc(chunk) ||
            (!hact.empty() && !act.alloc(hact.size())) || (masked && (!Y.alloc(chunk * syms * g.Lm) || !mjobs.alloc(chunk))))
            return fail(WOFDM_E_NOMEM, "device allocation failed%s", whose);
        if (!hact.empty() && !act.upload(hact.data(), hact.size())) return fail(WOFDM_E_HIP, "upload failed");
        return WOFDM_OK;
    }
    // the chain's parameters but for the chunk itself (item0, n_jobs); wdiv: cells per window pair
    wofdm_pparams params(const wofdm_cfg *cfg, const tx_geom &g, int syms, uint32_t wdiv, const tx_shared &sh) const
    {
        wofdm_pparams pp{};
        pp.S = syms; pp.k = g.k; pp.P = g.P; pp.cp = cfg->cp; pp.cs = cfg->cs; pp.beta = g.beta; pp.n_bins = 1;
        pp.seed_lo = (uint32_t)cfg->seed; pp.seed_hi = (uint32_t)(cfg->seed >> 32);
        pp.frames = cfg->frames_per_cell; pp.frame_offset = cfg->frame_offset; pp.wdiv = wdiv;
        pp.wtx = sh.w; pp.amask = act; pp.spec = sh.spec; pp.jobs = jobs; pp.mjobs = mjobs;
        pp.X = X; pp.x = x; pp.Y = Y;
        return pp;
    }
};

// frames per chunk: what the budget holds, at most a grid's y dimension, at least one
uint64_t chunk_frames(uint64_t items, uint64_t budget, uint64_t job_bytes)
{
    return std::min<uint64_t>(items, std::min<uint64_t>(WOFDM_PAPR_MAX_JOBS, std::max<uint64_t>(1, budget / job_bytes)));
}

// The chunk loop of a call: launch(item0, n_jobs) enqueues one chunk on the null stream.  *err is what the loop ended with, *ms
// the time between the first chunk's enqueue and the last one's end.
template <typename F> int run_chunks(uint64_t items, uint64_t chunk, F launch, hipError_t *err, float *ms)
{
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess) {
        if (ev[0]) (void)hipEventDestroy(ev[0]);
        return fail(WOFDM_E_HIP, "event creation failed");
    }
    {
        // (no frame kernel of this process beside these kernels: the gate of launch() is held until they have finished)
        std::lock_guard<std::mutex> gate(g_gate_mu);
        (void)hipDeviceSynchronize();
        hipError_t e = hipEventRecord(ev[0], nullptr);
        for (uint64_t i0 = 0; e == hipSuccess && i0 < items; i0 += chunk) e = launch(i0, (int32_t)std::min<uint64_t>(chunk, items - i0));
        if (e == hipSuccess) e = hipEventRecord(ev[1], nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipEventElapsedTime(ms, ev[0], ev[1]);
        *err = e;
    }
    (void)hipEventDestroy(ev[0]);
    (void)hipEventDestroy(ev[1]);
    return WOFDM_OK;
}

}  // namespace

extern "C" {

int wofdm_version(void) { return WOFDM_ABI_VERSION; }

const char *wofdm_last_error(void) { return g_err; }

int wofdm_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return fail(WOFDM_E_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
    return n;
}

int wofdm_noise_len(const wofdm_cfg *cfg)
{
    geom g;
    int rc = check_cfg(cfg, &g);
    return rc ? rc : g.NL;
}

int wofdm_plan_create(wofdm_plan **out, const wofdm_cfg *cfg, int device, const float *w_tx,
                      const float *w_rx, const float *h, const float *snr_db)
{
    if (!out || !w_tx || !w_rx || !h || !snr_db) return fail(WOFDM_E_INVALID, "NULL argument");
    *out = nullptr;
    geom g;
    int rc = check_cfg(cfg, &g);
    if (rc) return rc;
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev)
        return fail(WOFDM_E_HIP, "device %d not available (%d visible); there is no CPU fallback",
                    device, ndev);
    HIP_TRY(hipSetDevice(device));

    wofdm_plan *pl = new (std::nothrow) wofdm_plan;
    if (!pl) return fail(WOFDM_E_NOMEM, "out of host memory");
    pl->device = device; pl->cfg = *cfg; pl->g = g;
    pl->n_cells = (uint32_t)cfg->n_channels * cfg->n_snr * cfg->n_window_pairs;

    const size_t n_wtx = (size_t)cfg->n_window_pairs * g.P;
    const size_t n_wrx = (size_t)cfg->n_window_pairs * (g.N + g.delta);
    std::vector<float2> hp((size_t)cfg->n_channels * WOFDM_LT, make_float2(0.f, 0.f));
    for (int c = 0; c < cfg->n_channels; ++c)
        for (int l = 0; l < g.L; ++l)
            hp[(size_t)c * WOFDM_LT + l] = make_float2(h[2 * ((size_t)c * g.L + l)],
                                                       h[2 * ((size_t)c * g.L + l) + 1]);
    // Matrix-pipe FIR (wofdm_kernel.hip, phase B of layouts 6 and 7): per channel the 16 x 64 block
    // A[2i + o][2jj + c] = {hr, -hi; hi, hr}[o][c] of tap i + 24 - jj (i < 8 outputs, jj < 32 window
    // samples), scaled by a power of two and split into f16 hi + lo, in the operand layout of
    // v_mfma_f32_16x16x32_f16: lane (m = lane % 16, kg = lane / 16) holds columns 8 kg .. 8 kg + 7
    // of row m of one K = 32 half.  fira[ch][2 half + part][lane] = 8 halves.
    double hmax = 0.0, wmax = 0.0;
    for (float v : std::vector<float>(h, h + 2 * (size_t)cfg->n_channels * g.L)) hmax = std::fmax(hmax, std::fabs((double)v));
    for (size_t i = 0; i < n_wtx; ++i) wmax = std::fmax(wmax, std::fabs((double)w_tx[i]));
    // taps: largest component in [512, 1024); samples: |x| <= wmax * 1.53 (largest 64-QAM point) * N
    // before the table's 1/N, kept below 2^15
    pl->firm_sh = hmax > 0.0 ? (float)std::exp2(9.0 - std::floor(std::log2(hmax))) : 1.0f;
    pl->firm_sx = wmax > 0.0 ? (float)std::exp2(std::floor(std::log2(32768.0 / (wmax * 1.53)))) : 1.0f;
    std::vector<_Float16> fira((size_t)cfg->n_channels * 4 * 64 * 8);
    for (int c = 0; c < cfg->n_channels; ++c)
        for (int a = 0; a < 4; ++a)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 8; ++e) {
                    const int hf = a >> 1, part = a & 1, m = lane & 15, kg = lane >> 4;
                    const int jj = 16 * hf + 4 * kg + (e >> 1), cc = e & 1, i = m >> 1, o = m & 1;
                    const int l = i + 24 - jj;
                    double val = 0.0;
                    if (l >= 0 && l < g.L) {
                        const double hr = h[2 * ((size_t)c * g.L + l)], hi = h[2 * ((size_t)c * g.L + l) + 1];
                        val = (o == 0 ? (cc == 0 ? hr : -hi) : (cc == 0 ? hi : hr)) * (double)pl->firm_sh;
                    }
                    const _Float16 vh = (_Float16)val;
                    const _Float16 vl = (_Float16)(val - (double)vh);
                    fira[(((size_t)c * 4 + a) * 64 + lane) * 8 + e] = part ? vl : vh;
                }
    std::vector<float> nlin(cfg->n_snr);
    for (int i = 0; i < cfg->n_snr; ++i) nlin[i] = (float)std::pow(10.0, -0.1 * (double)snr_db[i]);
    // Matrix-pipe 256-point transforms (wofdm_kernel.hip, mdft_fwd; layouts 10, 11): per lane (a = lane % 16, g = lane / 16)
    // the operand rows of th^(x y), th = exp(-2 pi i / 16), as {Fr, -Fi} (real outputs) / {Fi, Fr} (imaginary outputs) over
    // K = (index, re | im), split into f16 hi + lo:
    //   rows 0..3  stage 1, B operand: column k1 = a, K slot (g, j) <-> n1 = g + 4 j          (re hi, re lo, im hi, im lo)
    //   rows 4..7  stage 2, A operand: row a <-> k2 = a / 4 + 4 (a % 4), K slot (g, j) <-> n2 = 4 g + j
    //   rows 8, 9  the inter-stage twiddles exp(-2 pi i (4 g + j) a / 256), j < 4: real parts, imaginary parts (fp32)
    //   rows 10.. (N = 512, 1024: layout 12) the twiddles in front of the last, radix-N/256 stage, exp(-2 pi i c (lane + 64 j) / N),
    //             c = 1 .. N/256 - 1: real parts, imaginary parts  (N = 256: the same for 1024 points, the Tx mask of layout 15)
    // (rows beyond the first ten: N >= 512, N = 128, and N = 256 for the 1024-point transforms of the Tx mask -- layout 15)
    const int dft_nc = g.N >= 512 ? g.N / 256 : (g.N == 128 ? 2 : (g.N == 256 ? 4 : 1));
    const int dft_n2 = g.N == 256 ? 1024 : g.N;
    std::vector<uint32_t> dftc((size_t)(10 + 2 * (dft_nc - 1)) * 64 * 4);
    {
        const double PI = 3.14159265358979323846;
        for (int lane = 0; lane < 64; ++lane) {
            const int a = lane & 15, gq = lane >> 4;
            for (int j = 0; j < 4; ++j) {
                for (int st = 0; st < 2; ++st) {
                    const int x = st == 0 ? gq + 4 * j : 4 * gq + j;         // contracted index of the K slot
                    const int y = st == 0 ? a : (a >> 2) + 4 * (a & 3);      // output index of the lane
                    const double ang = -2.0 * PI * (double)((x * y) & 15) / 16.0;
                    double fr = std::cos(ang), fi = std::sin(ang);
                    if (((x * y) & 3) == 0) {                                 // multiples of a quarter turn: exact 0, +-1
                        fr = std::round(fr); fi = std::round(fi);
                    }
                    const double vals[2][2] = {{fr, -fi}, {fi, fr}};          // [re | im output][K = re | im input]
                    for (int o = 0; o < 2; ++o) {
                        uint32_t whi = 0, wlo = 0;
                        for (int c = 0; c < 2; ++c) {
                            const _Float16 vh = (_Float16)vals[o][c];
                            const _Float16 vl = (_Float16)(vals[o][c] - (double)vh);
                            uint16_t bh, bl;
                            std::memcpy(&bh, &vh, 2); std::memcpy(&bl, &vl, 2);
                            whi |= (uint32_t)bh << (16 * c);
                            wlo |= (uint32_t)bl << (16 * c);
                        }
                        dftc[((size_t)(4 * st + 2 * o + 0) * 64 + lane) * 4 + j] = whi;
                        dftc[((size_t)(4 * st + 2 * o + 1) * 64 + lane) * 4 + j] = wlo;
                    }
                }
                double ang = -2.0 * PI * (double)((4 * gq + j) * a) / 256.0;
                // (N = 64, 128 -- layouts 13 / 14: ONE 16-point stage; rows 8, 9 (and 10, 11 at N = 128) hold the twiddles in front
                // of the radix-N/16 stage, exp(-2 pi i (4 p + j) (lane % 16) / N), p = part of the symbol's N/16 stage-1 outputs)
                if (g.N <= 128) ang = -2.0 * PI * (double)(j * a) / (double)g.N;
                const float twr = (float)std::cos(ang), twi = (float)std::sin(ang);
                std::memcpy(&dftc[((size_t)8 * 64 + lane) * 4 + j], &twr, 4);
                std::memcpy(&dftc[((size_t)9 * 64 + lane) * 4 + j], &twi, 4);
                if (g.N == 128) {
                    const double a3 = -2.0 * PI * (double)((4 + j) * a) / 128.0;
                    const float t3r = (float)std::cos(a3), t3i = (float)std::sin(a3);
                    std::memcpy(&dftc[((size_t)10 * 64 + lane) * 4 + j], &t3r, 4);
                    std::memcpy(&dftc[((size_t)11 * 64 + lane) * 4 + j], &t3i, 4);
                }
                for (int c = 1; g.N >= 256 && c < dft_nc; ++c) {
                    const double a2 = -2.0 * PI * (double)((c * (lane + 64 * j)) % dft_n2) / (double)dft_n2;
                    const float t2r = (float)std::cos(a2), t2i = (float)std::sin(a2);
                    std::memcpy(&dftc[((size_t)(10 + 2 * (c - 1)) * 64 + lane) * 4 + j], &t2r, 4);
                    std::memcpy(&dftc[((size_t)(11 + 2 * (c - 1)) * 64 + lane) * 4 + j], &t2i, 4);
                }
            }
        }
    }
    // received samples in kernel units: natural units (unit-power symbols, 1/N in the IDFT: rms 1/sqrt(N)) x firm_sx x firm_sh x
    // |h|, plus noise; a power of two per (snr, channel) brings their rms to about 16 (everything behind is homogeneous
    // in it: the equaliser divides by the pilot)
    std::vector<float> rxs((size_t)cfg->n_snr * cfg->n_channels, 1.0f);
    for (int i = 0; i < cfg->n_snr; ++i)
        for (int c = 0; c < cfg->n_channels; ++c) {
            double e = 0.0;
            for (int l = 0; l < g.L; ++l) {
                const double hr = h[2 * ((size_t)c * g.L + l)], hi = h[2 * ((size_t)c * g.L + l) + 1];
                e += hr * hr + hi * hi;
            }
            const double rms = (double)pl->firm_sx * (double)pl->firm_sh * std::sqrt(e * (1.0 + (double)nlin[i]) / (double)g.N)
                               * std::fmax(wmax, 1e-30);
            if (rms > 0.0 && std::isfinite(rms))
                rxs[(size_t)i * cfg->n_channels + c] = (float)std::exp2(std::round(4.0 - std::log2(rms)));
        }

#define PLAN_TRY(expr)                                                                        \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            wofdm_plan_destroy(pl);                                                           \
            return fail(e_ == hipErrorOutOfMemory ? WOFDM_E_NOMEM : WOFDM_E_HIP, "%s: %s",    \
                        #expr, hipGetErrorString(e_));                                        \
        }                                                                                     \
    } while (0)

    PLAN_TRY(hipMalloc(&pl->d_wtx, n_wtx * sizeof(float)));
    PLAN_TRY(hipMalloc(&pl->d_wrx, n_wrx * sizeof(float)));
    PLAN_TRY(hipMalloc(&pl->d_h, hp.size() * sizeof(float2)));
    PLAN_TRY(hipMalloc(&pl->d_nlin, nlin.size() * sizeof(float)));
    PLAN_TRY(hipMemcpy(pl->d_wtx, w_tx, n_wtx * sizeof(float), hipMemcpyHostToDevice));
    PLAN_TRY(hipMemcpy(pl->d_wrx, w_rx, n_wrx * sizeof(float), hipMemcpyHostToDevice));
    PLAN_TRY(hipMemcpy(pl->d_h, hp.data(), hp.size() * sizeof(float2), hipMemcpyHostToDevice));
    PLAN_TRY(hipMemcpy(pl->d_nlin, nlin.data(), nlin.size() * sizeof(float), hipMemcpyHostToDevice));
    PLAN_TRY(hipMalloc(&pl->d_fira, fira.size() * sizeof(_Float16)));
    PLAN_TRY(hipMemcpy(pl->d_fira, fira.data(), fira.size() * sizeof(_Float16), hipMemcpyHostToDevice));
    PLAN_TRY(hipMalloc(&pl->d_dftc, dftc.size() * sizeof(uint32_t)));
    PLAN_TRY(hipMemcpy(pl->d_dftc, dftc.data(), dftc.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    PLAN_TRY(hipMalloc(&pl->d_rxs, rxs.size() * sizeof(float)));
    PLAN_TRY(hipMemcpy(pl->d_rxs, rxs.data(), rxs.size() * sizeof(float), hipMemcpyHostToDevice));
    PLAN_TRY(hipEventCreate(&pl->ev0));
    PLAN_TRY(hipEventCreate(&pl->ev1));

    int geo[WOFDM_G_COUNT];
    geo[WOFDM_G_S] = g.S; geo[WOFDM_G_MU] = g.mu; geo[WOFDM_G_RHO] = g.rho; geo[WOFDM_G_BETA] = g.beta;
    geo[WOFDM_G_DELTA] = g.delta; geo[WOFDM_G_GAMMA] = g.gamma; geo[WOFDM_G_KAPPA] = g.kappa;
    geo[WOFDM_G_L] = g.L; geo[WOFDM_G_P] = g.P; geo[WOFDM_G_B] = g.B; geo[WOFDM_G_T] = g.T;
    geo[WOFDM_G_NL] = g.NL; geo[WOFDM_G_NSNR] = cfg->n_snr; geo[WOFDM_G_NCH] = cfg->n_channels;
    geo[WOFDM_G_FBUF] = 0;                       // set by configure()
    geo[WOFDM_G_NACT] = g.N;
    geo[WOFDM_G_SPWR] = 0;                       // set by configure()
    PLAN_TRY(hipMalloc(&pl->d_geo, sizeof geo));
    PLAN_TRY(hipMemcpy(pl->d_geo, geo, sizeof geo, hipMemcpyHostToDevice));

    wofdm_kparams &kp = pl->base;
    kp.n_cells = pl->n_cells; kp.first_cell = 0; kp.inject_base_cell = 0;
    kp.seed_lo = (uint32_t)cfg->seed; kp.seed_hi = (uint32_t)(cfg->seed >> 32);

    hipDeviceProp_t prop;
    PLAN_TRY(hipGetDeviceProperties(&prop, device));
    pl->cus = prop.multiProcessorCount;
    PLAN_TRY(hipMalloc(&pl->d_status, sizeof(unsigned)));
    PLAN_TRY(hipMemset(pl->d_status, 0, sizeof(unsigned)));
    PLAN_TRY(hipMalloc(&pl->d_work, sizeof(unsigned long long)));
    PLAN_TRY(hipMemset(pl->d_work, 0, sizeof(unsigned long long)));
    if (const char *e = std::getenv("WOFDM_SPLIT_ALPHA")) {
        const double a = std::strtod(e, nullptr);
        if (!(a >= 0.0 && a < 1.0)) {
            wofdm_plan_destroy(pl);
            return fail(WOFDM_E_INVALID, "WOFDM_SPLIT_ALPHA=%s: a fraction in [0, 1)", e);
        }
        pl->split_alpha_256 = (uint32_t)(a * 256.0);
        pl->split_forced = true;
    }
    if (const char *e = std::getenv("WOFDM_SPLIT_CHUNK")) {
        const unsigned long c = std::strtoul(e, nullptr, 0);
        if (c < 1 || c > (1ul << 20)) {
            wofdm_plan_destroy(pl);
            return fail(WOFDM_E_INVALID, "WOFDM_SPLIT_CHUNK=%s: 1 ... 2^20 items", e);
        }
        pl->split_chunk = (uint32_t)c;
        pl->split_forced = true;
    }
    if ((rc = configure(pl)) != WOFDM_OK) {
        wofdm_plan_destroy(pl);
        return rc;
    }
    const int occ = pl->occ;
    if (const size_t row = wofdm_noise_scratch_len(g.N, pl->layout)) {
        pl->nscr_elems = (uint64_t)pl->cus * (uint64_t)occ * row;
        PLAN_TRY(hipMalloc(&pl->d_nscr, pl->nscr_elems * sizeof(float2)));
        PLAN_TRY(hipMemset(pl->d_nscr, 0, pl->nscr_elems * sizeof(float2)));
        PLAN_TRY(hipDeviceSynchronize());
    }
#undef PLAN_TRY
    *out = pl;
    return WOFDM_OK;
}

int wofdm_plan_destroy(wofdm_plan *pl)
{
    if (!pl) return WOFDM_OK;
    (void)hipSetDevice(pl->device);
    if (pl->d_wtx) (void)hipFree(pl->d_wtx);
    if (pl->d_wrx) (void)hipFree(pl->d_wrx);
    if (pl->d_h) (void)hipFree(pl->d_h);
    if (pl->d_nlin) (void)hipFree(pl->d_nlin);
    if (pl->d_geo) (void)hipFree(pl->d_geo);
    if (pl->d_nscr) (void)hipFree(pl->d_nscr);
    if (pl->d_amask) (void)hipFree(pl->d_amask);
    if (pl->d_tmask) (void)hipFree(pl->d_tmask);
    if (pl->d_tspec) (void)hipFree(pl->d_tspec);
    if (pl->d_tspec4) (void)hipFree(pl->d_tspec4);
    if (pl->d_status) (void)hipFree(pl->d_status);
    if (pl->d_work) (void)hipFree(pl->d_work);
    if (pl->d_fira) (void)hipFree(pl->d_fira);
    if (pl->d_dftc) (void)hipFree(pl->d_dftc);
    if (pl->d_rxs) (void)hipFree(pl->d_rxs);
    if (pl->ev0) (void)hipEventDestroy(pl->ev0);
    if (pl->ev1) (void)hipEventDestroy(pl->ev1);
    delete pl;
    return WOFDM_OK;
}

int wofdm_plan_set_allocation(wofdm_plan *pl, const uint8_t *active)
{
    if (!pl) return fail(WOFDM_E_INVALID, "plan is NULL");
    HIP_TRY(hipSetDevice(pl->device));
    HIP_TRY(hipDeviceSynchronize());           // no launch of this plan may still read the mask
    const int N = pl->g.N, NQ = N / 4;
    const size_t amask_words = wofdm_amask_words(N);
    int nact = N;
    if (active) {
        nact = 0;
        // [0, NQ): word j, byte r <-> subcarrier j + r NQ; [NQ, 2 NQ): the quarter-wave order of
        // the N = 256 kernels, word 16 q + l, byte r <-> subcarrier l + 16 (q + 4 r)
        // N >= 512, [NQ, NQ + 256): the input element order of layout 12, word lane + 64 j, byte c <-> subcarrier
        // N/16 (lane / 16 + 4 j) + NC (lane % 16) + c, NC = N / 256; N = 256: the same with NC = 1 (layout 15) in [2 NQ, 2 NQ + 256)
        std::vector<uint32_t> words(amask_words, 0u);
        for (int n = 0; n < N; ++n) {
            if (active[n]) { ++nact; continue; }
            words[(size_t)(n % NQ)] |= 0x80u << (8 * (n / NQ));
            if (N == 256) {
                const int l = n & 15, t = n >> 4;
                words[(size_t)(NQ + 16 * (t & 3) + l)] |= 0x80u << (8 * (t >> 2));
            }
            if (N <= 128) {
                // [NQ, NQ + 256): layouts 13 / 14, word 64 t + lane (set t), byte j <-> subcarrier N/16 (lane / 16 + 4 j) + c,
                // c = 4 (t % (N / 64)) + lane % 4
                const int sc = N / 16, scs = sc / 4;
                for (int t = 0; t < 4; ++t)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 4; ++j)
                            if (sc * (lane / 16 + 4 * j) + 4 * (t % scs) + (lane & 3) == n)
                                words[(size_t)(NQ + 64 * t + lane)] |= 0x80u << (8 * j);
            }
            if (N >= 512 || N == 256) {
                // (N = 256, layout 15: one set, behind the quarter-wave part)
                const int nc = N >= 512 ? N / 256 : 1, a = n / (N / 16), r = n % (N / 16), b = r / nc, c = r % nc;   // n = N/16 a + NC b + c
                const int lane = 16 * (a & 3) + b, j = a >> 2;                                         // a = g + 4 j
                words[(size_t)((N == 256 ? 2 * NQ : NQ) + lane + 64 * j)] |= 0x80u << (8 * c);
            }
        }
        if (nact == 0) return fail(WOFDM_E_INVALID, "allocation loads no subcarrier");
        if (!pl->d_amask) HIP_TRY(hipMalloc(&pl->d_amask, amask_words * sizeof(uint32_t)));
        HIP_TRY(hipMemcpy(pl->d_amask, words.data(), amask_words * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    if (!active && pl->d_amask) HIP_TRY(hipMemset(pl->d_amask, 0, amask_words * sizeof(uint32_t)));
    HIP_TRY(hipMemcpy(pl->d_geo + WOFDM_G_NACT, &nact, sizeof(int), hipMemcpyHostToDevice));
    pl->has_alloc = active && nact < N;
    return configure(pl);
}

int wofdm_plan_set_tx_mask(wofdm_plan *pl, const float *mask)
{
    if (!pl) return fail(WOFDM_E_INVALID, "plan is NULL");
    HIP_TRY(hipSetDevice(pl->device));
    HIP_TRY(hipDeviceSynchronize());
    if (!mask) {
        pl->has_mask = false;
        return configure(pl);
    }
    // impulse response of the mask: g = IDFT_{2P-1}(mask), in double on the host (complex in
    // general: main_channel_mask.m's centred raised cosine is not even around bin 0 when P is odd)
    const int Lm = 2 * pl->g.P - 1;
    std::vector<float2> gtd((size_t)Lm);
    for (int n = 0; n < Lm; ++n) {
        double re = 0.0, im = 0.0;
        for (int k = 0; k < Lm; ++k) {
            const double a = 2.0 * M_PI * (double)(((long long)k * n) % Lm) / (double)Lm;
            re += (double)mask[k] * std::cos(a);
            im += (double)mask[k] * std::sin(a);
        }
        gtd[(size_t)n] = make_float2((float)(re / Lm), (float)(im / Lm));
    }
    if (!pl->d_tmask) HIP_TRY(hipMalloc(&pl->d_tmask, (size_t)Lm * sizeof(float2)));
    HIP_TRY(hipMemcpy(pl->d_tmask, gtd.data(), (size_t)Lm * sizeof(float2), hipMemcpyHostToDevice));
    {
        // fast-convolution spectrum: FFT_MF of gt[t] = g[(t - (P-1)) mod (2P-1)], t < 3P-2, with the
        // 1/MF of the inverse transform folded in (wofdm_kernel.hip, TXFFT)
        const int MF = WOFDM_TXFFT_LEN, P = pl->g.P, G = 3 * P - 2;
        std::vector<float2> spec((size_t)MF, make_float2(0.f, 0.f));
        if (G <= MF) {
            std::vector<double> gr((size_t)G), gi((size_t)G), cw((size_t)MF), sw((size_t)MF);
            for (int t = 0; t < G; ++t) {
                const int kk = ((t - (P - 1)) % Lm + Lm) % Lm;
                double re = 0.0, im = 0.0;          // g in double again (gtd is rounded to float)
                for (int k = 0; k < Lm; ++k) {
                    const double a = 2.0 * M_PI * (double)(((long long)k * kk) % Lm) / (double)Lm;
                    re += (double)mask[k] * std::cos(a);
                    im += (double)mask[k] * std::sin(a);
                }
                gr[(size_t)t] = re / Lm; gi[(size_t)t] = im / Lm;
            }
            for (int q = 0; q < MF; ++q) {
                cw[(size_t)q] = std::cos(2.0 * M_PI * q / MF); sw[(size_t)q] = -std::sin(2.0 * M_PI * q / MF);
            }
            for (int f = 0; f < MF; ++f) {
                double re = 0.0, im = 0.0;
                for (int t = 0; t < G; ++t) {
                    const int q = (int)(((long long)f * t) % MF);
                    re += gr[(size_t)t] * cw[(size_t)q] - gi[(size_t)t] * sw[(size_t)q];
                    im += gr[(size_t)t] * sw[(size_t)q] + gi[(size_t)t] * cw[(size_t)q];
                }
                spec[(size_t)f] = make_float2((float)(re / MF), (float)(im / MF));
            }
        }
        if (!pl->d_tspec) HIP_TRY(hipMalloc(&pl->d_tspec, (size_t)MF * sizeof(float2)));
        HIP_TRY(hipMemcpy(pl->d_tspec, spec.data(), (size_t)MF * sizeof(float2), hipMemcpyHostToDevice));
        if (MF == 1024) {
            std::vector<float> spec4((size_t)2 * MF);
            for (int kc = 0; kc < 4; ++kc)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 4; ++j) {
                        const float2 v = spec[(size_t)(lane + 64 * j + 256 * kc)];
                        spec4[((size_t)(2 * kc + 0) * 64 + lane) * 4 + j] = 16.0f * v.x;
                        spec4[((size_t)(2 * kc + 1) * 64 + lane) * 4 + j] = 16.0f * v.y;
                    }
            if (!pl->d_tspec4) HIP_TRY(hipMalloc(&pl->d_tspec4, spec4.size() * sizeof(float)));
            HIP_TRY(hipMemcpy(pl->d_tspec4, spec4.data(), spec4.size() * sizeof(float), hipMemcpyHostToDevice));
        }
    }
    if (!pl->d_amask) {        // the mask kernels always read an allocation word
        const size_t amask_words = wofdm_amask_words(pl->g.N);
        HIP_TRY(hipMalloc(&pl->d_amask, amask_words * sizeof(uint32_t)));
        HIP_TRY(hipMemset(pl->d_amask, 0, amask_words * sizeof(uint32_t)));
    }
    const bool had = pl->has_mask;
    pl->has_mask = true;
    const int rc = configure(pl);
    if (rc != WOFDM_OK) pl->has_mask = had;
    return rc;
}

int wofdm_plan_set_option(wofdm_plan *pl, int32_t option, int32_t value)
{
    if (!pl) return fail(WOFDM_E_INVALID, "plan is NULL");
    HIP_TRY(hipSetDevice(pl->device));
    HIP_TRY(hipDeviceSynchronize());           // no launch of this plan may still be running on the old choice
    const bool direct = pl->force_direct_mask, valu = pl->fir_valu, dvalu = pl->dft_valu, ggeo = pl->generic_geo;
    const int cap = pl->max_spw;
    switch (option) {
    case WOFDM_OPT_FIR_VALU: pl->fir_valu = value != 0; break;
    case WOFDM_OPT_MAX_SPW:
        if (value != 0 && value != 1 && value != 2 && value != 4)
            return fail(WOFDM_E_INVALID, "WOFDM_OPT_MAX_SPW takes 0, 1, 2 or 4");
        pl->max_spw = value;
        break;
    case WOFDM_OPT_TXMASK_DIRECT: pl->force_direct_mask = value != 0; break;
    case WOFDM_OPT_DFT_VALU: pl->dft_valu = value != 0; break;
    case WOFDM_OPT_GENERIC_GEOMETRY: pl->generic_geo = value != 0; break;
    default: return fail(WOFDM_E_INVALID, "unknown option %d", (int)option);
    }
    const int rc = configure(pl);
    if (rc != WOFDM_OK) { pl->force_direct_mask = direct; pl->fir_valu = valu; pl->max_spw = cap; pl->dft_valu = dvalu; pl->generic_geo = ggeo; }
    // (the noise scratch rows are sized per layout: a forced grid in launch() regrows them, a new layout here)
    if (rc == WOFDM_OK) {
        const size_t row = wofdm_noise_scratch_len(pl->g.N, pl->layout);
        const uint64_t wgs = (uint64_t)pl->cus * (uint64_t)pl->occ;
        if (row && wgs * row > pl->nscr_elems) {
            if (pl->d_nscr) (void)hipFree(pl->d_nscr);
            pl->d_nscr = nullptr; pl->nscr_elems = 0;
            HIP_TRY(hipMalloc(&pl->d_nscr, wgs * row * sizeof(float2)));
            HIP_TRY(hipMemset(pl->d_nscr, 0, wgs * row * sizeof(float2)));
            pl->nscr_elems = wgs * row;
        }
    }
    return rc;
}

int wofdm_plan_status(wofdm_plan *pl)
{
    if (!pl) return fail(WOFDM_E_INVALID, "plan is NULL");
    HIP_TRY(hipSetDevice(pl->device));
    return check_status(pl);
}

int wofdm_plan_info(wofdm_plan *pl, int32_t info[5])
{
    if (!pl || !info) return fail(WOFDM_E_INVALID, "NULL argument");
    info[0] = wofdm_waves(pl->layout, pl->g.N, pl->g.S, pl->g.B);
    info[1] = (int32_t)pl->base.lds_bytes;
    info[2] = pl->cus * pl->occ;
    info[3] = pl->occ;
    info[4] = pl->cus;
    return WOFDM_OK;
}

#ifdef WOFDM_AUDIT
// developer build only: device buffer of [grid][items][16][8] words for the per-frame records
extern "C" int wofdm_plan_set_audit(wofdm_plan *pl, void *dev, uint32_t items)
{
    if (!pl) return WOFDM_E_INVALID;
    pl->audit = static_cast<uint32_t *>(dev); pl->audit_items = items;
    return WOFDM_OK;
}
#endif
int wofdm_plan_kernel_id(wofdm_plan *pl, int32_t id[2])
{
    if (!pl || !id) return fail(WOFDM_E_INVALID, "NULL argument");
    id[0] = pl->layout;
    id[1] = pl->var;
    return WOFDM_OK;
}

int wofdm_plan_kernel_geo(wofdm_plan *pl, int32_t *id)
{
    if (!pl || !id) return fail(WOFDM_E_INVALID, "NULL argument");
    *id = pl->geo;
    return WOFDM_OK;
}

int wofdm_cfg_geo_id(const wofdm_cfg *cfg)
{
    geom g;
    const int rc = check_cfg(cfg, &g);
    return rc != WOFDM_OK ? rc : geo_id_of(g);
}

int wofdm_plan_launch(wofdm_plan *pl, uint64_t frame_offset, uint64_t frames_per_cell,
                      uint64_t *counts_dev, void *stream)
{
    int rc = check_launch_args(pl, frames_per_cell);
    if (rc) return rc;
    if (!counts_dev) return fail(WOFDM_E_INVALID, "counts_dev is NULL");
    HIP_TRY(hipSetDevice(pl->device));
    wofdm_kparams kp = pl->base;
    kp.frames_per_cell = frames_per_cell; kp.frame_offset = frame_offset;
    kp.counts = reinterpret_cast<unsigned long long *>(counts_dev);
    return launch(pl, WOFDM_MODE_GEN, kp, frames_per_cell * pl->n_cells, 0,
                  static_cast<hipStream_t>(stream));
}

int wofdm_plan_launch_timed(wofdm_plan *pl, uint64_t frame_offset, uint64_t frames_per_cell,
                            uint64_t *counts_dev, void *stream, float *kernel_ms)
{
    if (!pl || !kernel_ms) return fail(WOFDM_E_INVALID, "NULL argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(pl->device));
    HIP_TRY(hipEventRecord(pl->ev0, st));
    int rc = wofdm_plan_launch(pl, frame_offset, frames_per_cell, counts_dev, stream);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(pl->ev1, st));
    HIP_TRY(hipEventSynchronize(pl->ev1));
    HIP_TRY(hipEventElapsedTime(kernel_ms, pl->ev0, pl->ev1));
    return check_status(pl);
}

int wofdm_plan_launch_injected(wofdm_plan *pl, uint64_t frames_per_cell, const uint8_t *labels_dev,
                               const float *unit_noise_dev, uint64_t *counts_dev, void *stream)
{
    int rc = check_launch_args(pl, frames_per_cell);
    if (rc) return rc;
    if (!counts_dev || !labels_dev || !unit_noise_dev) return fail(WOFDM_E_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(pl->device));
    wofdm_kparams kp = pl->base;
    kp.frames_per_cell = frames_per_cell; kp.frame_offset = 0;
    kp.counts = reinterpret_cast<unsigned long long *>(counts_dev);
    kp.labels = labels_dev;
    kp.unit_noise = reinterpret_cast<const float2 *>(unit_noise_dev);
    return launch(pl, WOFDM_MODE_INJECT, kp, frames_per_cell * pl->n_cells, 0,
                  static_cast<hipStream_t>(stream));
}

int wofdm_plan_dump_frame(wofdm_plan *pl, uint32_t cell, uint64_t frame, const uint8_t *labels,
                          const float *unit_noise, uint64_t *counts, wofdm_dump *out)
{
    if (!pl || !counts || !out) return fail(WOFDM_E_INVALID, "NULL argument");
    if (cell >= pl->n_cells) return fail(WOFDM_E_INVALID, "cell %u out of range", cell);
    if ((labels == nullptr) != (unit_noise == nullptr))
        return fail(WOFDM_E_INVALID, "inject both labels and unit_noise or neither");
    const geom &g = pl->g;
    HIP_TRY(hipSetDevice(pl->device));
    const size_t SN = (size_t)g.S * g.N, CL = (size_t)g.T + g.L - 1, SB = (size_t)g.S * g.B;
    // one device arena: [counts 4xu64][X][tx][conv][rx][Y][Xhat][noise] float2, gain, labels
    const size_t n_f2 = SN + g.T + CL + SB + SN + SN + (size_t)g.NL;
    const size_t bytes = 32 + n_f2 * sizeof(float2) + 16 + 2 * SN + (labels ? SN + (size_t)g.NL * 8 : 0) + 64;
    unsigned char *arena = nullptr;
    HIP_TRY(hipMalloc(&arena, bytes));
    int rc = WOFDM_OK;
    do {
        if (hipMemset(arena, 0, bytes) != hipSuccess) { rc = fail(WOFDM_E_HIP, "hipMemset failed"); break; }
        wofdm_kparams kp = pl->base;
        unsigned char *ptr = arena;
        kp.counts = reinterpret_cast<unsigned long long *>(ptr); ptr += 32;    // entry 0 = `cell` (inject_base_cell below)
        float2 *f2 = reinterpret_cast<float2 *>(ptr);
        kp.dump.X = f2; f2 += SN;
        kp.dump.tx = f2; f2 += g.T;
        kp.dump.conv = f2; f2 += CL;
        kp.dump.rx = f2; f2 += SB;
        kp.dump.Y = f2; f2 += SN;
        kp.dump.Xhat = f2; f2 += SN;
        kp.dump.unit_noise = f2; f2 += g.NL;
        kp.dump.gain = reinterpret_cast<float *>(f2);
        kp.dump.sink = f2 + 1;                     // inside the 16-byte pad behind the gain
        unsigned char *b = reinterpret_cast<unsigned char *>(f2) + 16;
        kp.dump.labels_tx = b; b += SN;
        kp.dump.labels_rx = b; b += SN;
        if (labels) {
            uint8_t *dl = b; b += SN;
            b = reinterpret_cast<unsigned char *>(((uintptr_t)b + 15) & ~(uintptr_t)15);
            float2 *dn = reinterpret_cast<float2 *>(b);
            if (hipMemcpy(dl, labels, SN, hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(dn, unit_noise, (size_t)g.NL * 8, hipMemcpyHostToDevice) != hipSuccess) {
                rc = fail(WOFDM_E_HIP, "hipMemcpy of injected inputs failed"); break;
            }
            kp.labels = dl; kp.unit_noise = dn;
        }
        kp.first_cell = cell; kp.n_cells = 1; kp.inject_base_cell = cell;
        kp.frames_per_cell = 1; kp.frame_offset = frame;
        rc = launch(pl, labels ? WOFDM_MODE_DUMP_INJECT : WOFDM_MODE_DUMP_GEN, kp, 1, 1, nullptr);
        if (rc) break;
        if (hipDeviceSynchronize() != hipSuccess) { rc = fail(WOFDM_E_HIP, "dump kernel failed: %s", hipGetErrorString(hipGetLastError())); break; }
        uint64_t c4[4];
        auto down = [&](void *dst, const void *src, size_t n) {
            return !dst || hipMemcpy(dst, src, n, hipMemcpyDeviceToHost) == hipSuccess;
        };
        bool ok = down(c4, arena, 32) && down(out->X, kp.dump.X, SN * 8) &&
                  down(out->tx, kp.dump.tx, (size_t)g.T * 8) && down(out->conv, kp.dump.conv, CL * 8) &&
                  down(out->rx, kp.dump.rx, SB * 8) && down(out->Y, kp.dump.Y, SN * 8) &&
                  down(out->Xhat, kp.dump.Xhat, (SN - g.N) * 8) &&
                  down(out->unit_noise, kp.dump.unit_noise, (size_t)g.NL * 8) &&
                  down(out->gain, kp.dump.gain, 4) && down(out->labels_tx, kp.dump.labels_tx, SN) &&
                  down(out->labels_rx, kp.dump.labels_rx, SN - g.N);
        if (!ok) { rc = fail(WOFDM_E_HIP, "hipMemcpy of dump failed"); break; }
        // The kernels (instrumented and production alike) leave the circular shift of the Rx chain (m:313-333) out:
        // their Y is the reference's times e^{-2 pi i (kappa + delta/2) n / N} on every symbol, which the one-tap
        // equaliser divides out.  The dump hands the reference's Y back: the ramp is undone here, on the host.
        if (out->Y && (g.kappa + g.delta / 2) % g.N != 0) {
            const int c = (g.kappa + g.delta / 2) % g.N;
            for (int n = 0; n < g.N; ++n) {
                const double a = 2.0 * M_PI * (double)(((long long)c * n) % g.N) / (double)g.N;
                const float cr = (float)std::cos(a), ci = (float)std::sin(a);
                for (int sy = 0; sy < g.S; ++sy) {
                    float *y = out->Y + 2 * ((size_t)sy * g.N + n);
                    const float re = y[0] * cr - y[1] * ci, im = y[0] * ci + y[1] * cr;
                    y[0] = re; y[1] = im;
                }
            }
        }
        for (int i = 0; i < 4; ++i) counts[i] += c4[i];
    } while (0);
    (void)hipFree(arena);
    return rc;
}

int wofdm_run(const wofdm_cfg *cfg, int device, const float *w_tx, const float *w_rx,
              const float *h, const float *snr_db, uint64_t *counts)
{
    if (!counts) return fail(WOFDM_E_INVALID, "counts is NULL");
    wofdm_plan *pl = nullptr;
    int rc = wofdm_plan_create(&pl, cfg, device, w_tx, w_rx, h, snr_db);
    if (rc) return rc;
    const size_t n = (size_t)pl->n_cells * 4;
    uint64_t *d = nullptr;
    std::vector<uint64_t> hc(n);
    do {
        if (hipMalloc(&d, n * 8) != hipSuccess || hipMemset(d, 0, n * 8) != hipSuccess) {
            rc = fail(WOFDM_E_NOMEM, "counter allocation failed"); break;
        }
        rc = wofdm_plan_launch(pl, cfg->frame_offset, cfg->frames_per_cell, d, nullptr);
        if (rc) break;
        if (hipDeviceSynchronize() != hipSuccess ||
            hipMemcpy(hc.data(), d, n * 8, hipMemcpyDeviceToHost) != hipSuccess) {
            rc = fail(WOFDM_E_HIP, "kernel or copy-back failed: %s", hipGetErrorString(hipGetLastError()));
            break;
        }
        if ((rc = check_status(pl)) != WOFDM_OK) break;
        for (size_t i = 0; i < n; ++i) counts[i] += hc[i];
    } while (0);
    if (d) (void)hipFree(d);
    wofdm_plan_destroy(pl);
    return rc;
}

int wofdm_run_injected(const wofdm_cfg *cfg, int device, const float *w_tx, const float *w_rx,
                       const float *h, const float *snr_db, const uint8_t *labels,
                       const float *unit_noise, uint64_t *counts)
{
    if (!counts || !labels || !unit_noise) return fail(WOFDM_E_INVALID, "NULL argument");
    wofdm_plan *pl = nullptr;
    int rc = wofdm_plan_create(&pl, cfg, device, w_tx, w_rx, h, snr_db);
    if (rc) return rc;
    const size_t n = (size_t)pl->n_cells * 4;
    const size_t frames = (size_t)pl->n_cells * cfg->frames_per_cell;
    const size_t lb = frames * pl->g.S * pl->g.N, nb = frames * (size_t)pl->g.NL * 8;
    uint64_t *d = nullptr;
    uint8_t *dl = nullptr;
    float *dn = nullptr;
    std::vector<uint64_t> hc(n);
    do {
        if (hipMalloc(&d, n * 8) != hipSuccess || hipMemset(d, 0, n * 8) != hipSuccess ||
            hipMalloc(&dl, lb ? lb : 1) != hipSuccess || hipMalloc(&dn, nb ? nb : 8) != hipSuccess) {
            rc = fail(WOFDM_E_NOMEM, "device allocation failed"); break;
        }
        if (hipMemcpy(dl, labels, lb, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(dn, unit_noise, nb, hipMemcpyHostToDevice) != hipSuccess) {
            rc = fail(WOFDM_E_HIP, "upload failed"); break;
        }
        rc = wofdm_plan_launch_injected(pl, cfg->frames_per_cell, dl, dn, d, nullptr);
        if (rc) break;
        if (hipDeviceSynchronize() != hipSuccess ||
            hipMemcpy(hc.data(), d, n * 8, hipMemcpyDeviceToHost) != hipSuccess) {
            rc = fail(WOFDM_E_HIP, "kernel or copy-back failed: %s", hipGetErrorString(hipGetLastError()));
            break;
        }
        if ((rc = check_status(pl)) != WOFDM_OK) break;
        for (size_t i = 0; i < n; ++i) counts[i] += hc[i];
    } while (0);
    if (d) (void)hipFree(d);
    if (dl) (void)hipFree(dl);
    if (dn) (void)hipFree(dn);
    wofdm_plan_destroy(pl);
    return rc;
}

int wofdm_interference(const wofdm_cfg *cfg, int device, const float *w_tx, const float *w_rx,
                       const float *h, float *power)
{
    if (!w_tx || !w_rx || !h || !power) return fail(WOFDM_E_INVALID, "NULL argument");
    geom g;
    int rc = check_cfg(cfg, &g);
    if (rc) return rc;
    if ((rc = use_device(device)) != WOFDM_OK) return rc;
    const int jobs = cfg->n_window_pairs * cfg->n_channels;
    const size_t n_wtx = (size_t)cfg->n_window_pairs * g.P, n_wrx = (size_t)cfg->n_window_pairs * (g.N + g.delta);
    const size_t n_out = (size_t)jobs * g.N;
    const std::vector<float2> hp = pack_taps(cfg, g, h);
    dev_buf<float> d_wtx, d_wrx, d_pow;
    dev_buf<float2> d_h;
    if (!d_wtx.alloc(n_wtx) || !d_wrx.alloc(n_wrx) || !d_h.alloc(hp.size()) || !d_pow.alloc(n_out))
        return fail(WOFDM_E_NOMEM, "device allocation failed");
    if (!d_wtx.upload(w_tx, n_wtx) || !d_wrx.upload(w_rx, n_wrx) || !d_h.upload(hp.data(), hp.size()))
        return fail(WOFDM_E_HIP, "upload failed");
    // (no frame kernel of this process beside these kernels: the gate of launch() is held until they have finished)
    std::lock_guard<std::mutex> gate(g_gate_mu);
    (void)hipDeviceSynchronize();
    const wofdm_aux_fns *ax = wofdm_aux(g.N);
    const hipError_t e = !ax ? hipErrorInvalidValue
                             : ax->interf(jobs, g.P, g.B, g.mu, g.delta, g.gamma, g.kappa, cfg->n_channels, d_wtx, d_wrx, d_h,
                                          d_pow, nullptr);
    if (e != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(power, d_pow, n_out * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(WOFDM_E_HIP, "interference kernel or copy-back failed: %s", hipGetErrorString(hipGetLastError()));
    return WOFDM_OK;
}

// Every argument is checked before the first HIP call.
int wofdm_interference_masked(const wofdm_cfg *cfg, int device, const float *w_tx, const float *w_rx,
                              const float *h, const uint8_t *active, const float *tx_mask, float *power,
                              float *wanted)
{
    if (!cfg || !w_tx || !w_rx || !h || !power) return fail(WOFDM_E_INVALID, "NULL argument");
    if (!active && !tx_mask && !wanted) return wofdm_interference(cfg, device, w_tx, w_rx, h, power);
    geom g;
    int rc = check_cfg(cfg, &g);
    if (rc) return rc;
    if (cfg->n_window_pairs > 65535) return fail(WOFDM_E_UNSUPPORTED, "more than 65535 window pairs");
    const int Lm = 2 * g.P - 1, J = g.B + g.P - 1, JP = (J + 1) & ~1;
    // (check_cfg leaves tail_tx <= 16 and n_taps <= 21 against B >= 64: the filtered pulse ends within three periods)
    if (J + WOFDM_LT - 1 > 3 * g.B)
        return fail(WOFDM_E_UNSUPPORTED, "the masked pulse with the channel exceeds three symbol periods");
    std::vector<uint8_t> hact;
    if (active) {
        hact.resize((size_t)g.N);
        int n_act = 0;
        for (int n = 0; n < g.N; ++n) n_act += (hact[(size_t)n] = active[n] ? 1 : 0);
        if (n_act == 0) return fail(WOFDM_E_INVALID, "the allocation loads no subcarrier");
    }
    if (tx_mask)
        for (int i = 0; i < Lm; ++i)
            if (!std::isfinite(tx_mask[i])) return fail(WOFDM_E_INVALID, "mask gains must be finite");
    if ((rc = use_device(device)) != WOFDM_OK) return rc;
    // impulse response of the mask, g = IDFT_{2P-1}(gains): host, double precision, stored in single
    std::vector<float2> hg;
    if (tx_mask) {
        const std::vector<cplx> gd = idft_any(tx_mask, Lm);
        hg.resize((size_t)Lm);
        for (int i = 0; i < Lm; ++i) hg[(size_t)i] = make_float2((float)gd[(size_t)i].real(), (float)gd[(size_t)i].imag());
    }
    const int pairs = cfg->n_window_pairs, jobs = pairs * cfg->n_channels;
    const size_t n_wtx = (size_t)pairs * g.P, n_wrx = (size_t)pairs * (g.N + g.delta);
    const size_t n_cols = (size_t)pairs * g.N * JP, n_out = (size_t)jobs * g.N;
    const std::vector<float2> hp = pack_taps(cfg, g, h);
    dev_buf<float> d_wtx, d_wrx, d_pow, d_want;
    dev_buf<float2> d_h, d_g, d_cols;
    dev_buf<uint8_t> d_act;
    if (!d_wtx.alloc(n_wtx) || !d_wrx.alloc(n_wrx) || !d_h.alloc(hp.size()) || !d_pow.alloc(n_out) ||
        (wanted && !d_want.alloc(n_out)) || !d_cols.alloc(n_cols) || (tx_mask && !d_g.alloc(hg.size())) ||
        (active && !d_act.alloc(hact.size())))
        return fail(WOFDM_E_NOMEM, "device allocation failed (the pulses of %d pairs take %lld bytes)", pairs,
                    (long long)(n_cols * 8));
    if (!d_wtx.upload(w_tx, n_wtx) || !d_wrx.upload(w_rx, n_wrx) || !d_h.upload(hp.data(), hp.size()) ||
        (tx_mask && !d_g.upload(hg.data(), hg.size())) || (active && !d_act.upload(hact.data(), hact.size())))
        return fail(WOFDM_E_HIP, "upload failed");
    // (no frame kernel of this process beside these kernels: the gate of launch() is held until they have finished)
    std::lock_guard<std::mutex> gate(g_gate_mu);
    (void)hipDeviceSynchronize();
    const wofdm_aux_fns *ax = wofdm_aux(g.N);
    const hipError_t e = !ax ? hipErrorInvalidValue
                             : ax->interf_masked(pairs, cfg->n_channels, g.P, g.B, g.mu, g.delta, g.gamma, g.kappa, JP, d_wtx,
                                                 d_wrx, d_h, d_g, d_act, d_cols, d_pow, d_want, nullptr);
    if (e != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(power, d_pow, n_out * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        (wanted && hipMemcpy(wanted, d_want, n_out * 4, hipMemcpyDeviceToHost) != hipSuccess))
        return fail(WOFDM_E_HIP, "masked interference kernels or copy-back failed: %s", hipGetErrorString(hipGetLastError()));
    return WOFDM_OK;
}

int wofdm_tx_psd(const wofdm_cfg *cfg, int device, const float *w_tx, const float *X, int no_symbols,
                 int overlap, float *psd)
{
    if (!cfg || !w_tx || !X || !psd) return fail(WOFDM_E_INVALID, "NULL argument");
    const int N = cfg->n_fft;
    if (N != 64 && N != 128 && N != 256)
        return fail(WOFDM_E_UNSUPPORTED, "wofdm_tx_psd is built for n_fft in {64,128,256} (transform length 8 n_fft)");
    const int P = N + cfg->cp + cfg->cs;
    if (cfg->cp < 0 || cfg->cs < 0 || cfg->cp > N || cfg->cs > N || overlap < 0 || 2 * overlap > P || no_symbols < 1)
        return fail(WOFDM_E_INVALID, "bad cp / cs / overlap / no_symbols");
    const int rc = use_device(device);
    if (rc != WOFDM_OK) return rc;
    const int FL = 8 * N, len = overlap + no_symbols * (P - overlap);
    const size_t n_X = (size_t)no_symbols * N;
    dev_buf<float> d_w, d_psd;
    dev_buf<float2> d_X, d_x;
    if (!d_w.alloc((size_t)P) || !d_X.alloc(n_X) || !d_x.alloc((size_t)len) || !d_psd.alloc((size_t)FL))
        return fail(WOFDM_E_NOMEM, "device allocation failed");
    if (!d_w.upload(w_tx, (size_t)P) || !d_X.upload(X, n_X) ||
        hipMemset(d_x, 0, (size_t)len * 8) != hipSuccess)
        return fail(WOFDM_E_HIP, "upload failed");
    // (no frame kernel of this process beside these kernels: the gate of launch() is held until they have finished)
    std::lock_guard<std::mutex> gate(g_gate_mu);
    (void)hipDeviceSynchronize();
    const wofdm_aux_fns *ax = wofdm_aux(N);
    const hipError_t e = !(ax && ax->psd) ? hipErrorInvalidValue
                                          : ax->psd(P, cfg->cp, cfg->cs, overlap, no_symbols, d_w, d_X, d_x, len, d_psd, nullptr);
    if (e != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(psd, d_psd, (size_t)FL * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(WOFDM_E_HIP, "PSD kernels or copy-back failed: %s", hipGetErrorString(hipGetLastError()));
    return WOFDM_OK;
}

// the amplifier table of wofdm_tx_psd_batch_pa and its output; a null pointer to it is wofdm_tx_psd_batch(_masked)
struct psd_pa_args {
    int32_t n_pa;
    const wofdm_pa_point *pa;
    const int32_t *job_pa;
    float *job_power;
};

// wofdm_tx_psd_batch (n_masks = 0, job_mask = NULL), wofdm_tx_psd_batch_masked and wofdm_tx_psd_batch_pa.  Every argument is
// checked before the first HIP call.
static int psd_batch(const char *who, int32_t n_fft, int device, int32_t n_jobs, const wofdm_psd_job *jobs, const float *w_tx,
                     int32_t n_masks, const int32_t *mask_len, const float *mask_gain, const int32_t *job_mask,
                     int32_t n_blocks, int32_t no_symbols, const float *X, float *psd, const psd_pa_args *amp = nullptr)
{
    if (!jobs || !w_tx || !X || !psd || (n_masks > 0 && (!mask_len || !mask_gain)))
        return fail(WOFDM_E_INVALID, "NULL argument");
    if (amp && amp->n_pa < 0) return fail(WOFDM_E_INVALID, "bad n_pa");
    if (amp && amp->n_pa > 0 && !amp->pa) return fail(WOFDM_E_INVALID, "NULL argument (pa)");
    const int N = n_fft;
    if (N != 64 && N != 128 && N != 256 && N != 512 && N != 1024)
        return fail(WOFDM_E_UNSUPPORTED, "%s is built for n_fft in {64,128,256,512,1024}", who);
    if (n_jobs < 1 || n_jobs > 65535 || n_blocks < 1 || no_symbols < 1)
        return fail(WOFDM_E_INVALID, "bad n_jobs / n_blocks / no_symbols");
    if (n_masks < 0 || n_masks > 65535) return fail(WOFDM_E_INVALID, "bad n_masks");
    std::vector<int64_t> gain_off((size_t)n_masks);
    int64_t n_gain = 0;
    for (int m = 0; m < n_masks; ++m) {
        if (mask_len[m] < 1) return fail(WOFDM_E_INVALID, "mask %d: length %d", m, mask_len[m]);
        gain_off[(size_t)m] = n_gain;
        n_gain += mask_len[m];
    }
    for (int64_t i = 0; i < n_gain; ++i)
        if (!std::isfinite(mask_gain[i])) return fail(WOFDM_E_INVALID, "mask gains must be finite");
    const int FL = 8 * N, per_item = wofdm_psd_batch_slices(N);
    std::vector<wofdm_bjob> hj((size_t)n_jobs), hplain;
    std::vector<wofdm_mjob> hm;
    std::vector<wofdm_bitem> hi;
    std::vector<int> spec_of((size_t)n_masks, -1), spec_mask;       // masks in use -> spectrum slot, and back
    int64_t n_w = 0, n_x = 0, n_y = 0;
    int max_len = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const wofdm_psd_job &q = jobs[j];
        const int P = N + q.cp + q.cs;
        if (q.block < 0 || q.block >= n_blocks || q.cp < 0 || q.cs < 0 || q.cp > N || q.cs > N || q.overlap < 0 ||
            2 * q.overlap > P)
            return fail(WOFDM_E_INVALID, "job %d: bad block / cp / cs / overlap", j);
        const int64_t len = q.overlap + (int64_t)no_symbols * (P - q.overlap);
        if (len > INT32_MAX - 2 * (int64_t)FL) return fail(WOFDM_E_INVALID, "job %d: waveform of %lld samples", j, (long long)len);
        wofdm_bjob &b = hj[(size_t)j];
        b.block = q.block; b.cp = q.cp; b.cs = q.cs; b.overlap = q.overlap;
        b.w_off = (int32_t)n_w; b.len = (int32_t)len; b.x_off = n_x;
        const int n_sl = (int)((len + FL - 1) / FL);
        b.item0 = (int32_t)hi.size();
        for (int s0 = 0; s0 < n_sl; s0 += per_item) hi.push_back({j, s0, std::min(per_item, n_sl - s0), 0});
        b.n_items = (int32_t)hi.size() - b.item0;
        n_w += P; n_x += len;
        if (n_w > INT32_MAX) return fail(WOFDM_E_INVALID, "windows too long");
        const int m = job_mask ? job_mask[j] : -1;
        if (m < -1 || m >= n_masks) return fail(WOFDM_E_INVALID, "job %d: mask index %d outside [-1, %d)", j, m, n_masks);
        if (m >= 0) {
            if (mask_len[m] != 2 * P - 1)
                return fail(WOFDM_E_INVALID, "job %d: mask %d has %d gains, the job needs 2 P - 1 = %d", j, m, mask_len[m], 2 * P - 1);
            if (P > wofdm_txmask_batch_pmax(N))
                return fail(WOFDM_E_UNSUPPORTED, "job %d: a masked job needs 3 P - 2 <= 8 n_fft, i.e. P = n_fft + cp + cs <= %d "
                            "at n_fft = %d (P = %d)", j, wofdm_txmask_batch_pmax(N), N, P);
            if (spec_of[(size_t)m] < 0) {
                spec_of[(size_t)m] = (int)spec_mask.size();
                spec_mask.push_back(m);
            }
            hm.push_back({j, spec_of[(size_t)m], n_y});
            n_y += (int64_t)no_symbols * (2 * P - 1);
            max_len = std::max(max_len, (int)len);
        }
    }
    for (int j = 0; j < n_jobs; ++j)
        if (!(job_mask && job_mask[j] >= 0)) hplain.push_back(hj[(size_t)j]);
    // the amplifier of every job: the table's checks, then model, 2 p, 1 / (2 p) and 10^(ibo / 10) per job (model -1: none)
    std::vector<wofdm_pajob> hpa;
    if (amp) {
        std::vector<wofdm_papoint> pts;
        const int prc = check_pa_points(amp->n_pa, amp->pa, &pts);
        if (prc != WOFDM_OK) return prc;
        hpa.assign((size_t)n_jobs, wofdm_pajob{-1, 2.f, 0.5f, 0, 1.0});
        for (int j = 0; j < n_jobs; ++j) {
            const int a = amp->job_pa ? amp->job_pa[j] : -1;
            if (a < -1 || a >= amp->n_pa)
                return fail(WOFDM_E_INVALID, "job %d: amplifier index %d outside [-1, %d)", j, a, amp->n_pa);
            if (a >= 0)
                hpa[(size_t)j] = {pts[(size_t)a].model, pts[(size_t)a].two_p, pts[(size_t)a].inv_two_p, 0,
                                  std::pow(10.0, 0.1 * (double)amp->pa[a].ibo_db)};
        }
    }
    const int rc = use_device(device);
    if (rc != WOFDM_OK) return rc;
    // one fast-convolution spectrum per mask in use (host, fp64, O(M log M)), whatever the number of jobs that share it
    std::vector<float2> hspec(spec_mask.size() * (size_t)FL);
    for (size_t k = 0; k < spec_mask.size(); ++k) {
        const int m = spec_mask[k];
        mask_fastconv_spectrum(mask_gain + gain_off[(size_t)m], mask_len[m], FL, hspec.data() + k * (size_t)FL);
    }
    const size_t n_X = (size_t)n_blocks * no_symbols * N, n_items = hi.size();
    const bool masked = !hm.empty();
    dev_buf<float> d_w, d_part, d_psd;
    dev_buf<float2> d_X, d_x, d_spec, d_Y;
    dev_buf<wofdm_bjob> d_jobs, d_plain;
    dev_buf<wofdm_mjob> d_mjobs;
    dev_buf<wofdm_bitem> d_items;
    if (!d_w.alloc((size_t)n_w) || !d_X.alloc(n_X) || !d_x.alloc((size_t)n_x) || !d_part.alloc(n_items * FL) ||
        !d_psd.alloc((size_t)n_jobs * FL) || !d_jobs.alloc(hj.size()) || !d_items.alloc(n_items))
        return fail(WOFDM_E_NOMEM, "device allocation failed");
    if (masked && (!d_spec.alloc(hspec.size()) || !d_Y.alloc((size_t)n_y) || !d_mjobs.alloc(hm.size()) ||
                   (!hplain.empty() && !d_plain.alloc(hplain.size()))))
        return fail(WOFDM_E_NOMEM, "device allocation failed (masked jobs keep %lld filtered samples)", (long long)n_y);
    if (!d_w.upload(w_tx, (size_t)n_w) || !d_X.upload(X, n_X) || !d_jobs.upload(hj.data(), hj.size()) ||
        !d_items.upload(hi.data(), n_items) || hipMemset(d_x, 0, (size_t)n_x * 8) != hipSuccess)
        return fail(WOFDM_E_HIP, "upload failed");
    if (masked && (!d_spec.upload(hspec.data(), hspec.size()) || !d_mjobs.upload(hm.data(), hm.size()) ||
                   (!hplain.empty() && !d_plain.upload(hplain.data(), hplain.size()))))
        return fail(WOFDM_E_HIP, "upload failed");
    dev_buf<wofdm_pajob> d_pa;
    dev_buf<float> d_jpow;
    if (amp) {
        if (!d_pa.alloc(hpa.size()) || !d_jpow.alloc(2 * (size_t)n_jobs)) return fail(WOFDM_E_NOMEM, "device allocation failed (amplifier)");
        if (!d_pa.upload(hpa.data(), hpa.size())) return fail(WOFDM_E_HIP, "upload failed");
    }
    // (no frame kernel of this process beside these kernels: the gate of launch() is held until they have finished)
    std::lock_guard<std::mutex> gate(g_gate_mu);
    (void)hipDeviceSynchronize();
    const wofdm_aux_fns *ax = wofdm_aux(N);
    const int ni = (int)n_items, np = (int)hplain.size(), nm = (int)hm.size();
    hipError_t e = hipErrorInvalidValue;
    std::vector<float> hjpow(amp ? 2 * (size_t)n_jobs : 0);
    const wofdm_pa_fns *axp = wofdm_aux_pa(N);
    if (amp) {
        // (without a masked job every job is a plain one: the job table itself)
        if (axp)
            e = axp->psd_batch_pa(n_jobs, no_symbols, ni, d_jobs, d_items, masked ? np : n_jobs, masked ? d_plain : d_jobs, nm,
                                  d_mjobs, max_len, d_spec, d_Y, d_w, d_X, d_x, d_part, d_psd, d_pa, d_jpow, nullptr);
    } else if (ax && !masked) {
        e = ax->psd_batch(n_jobs, no_symbols, ni, d_jobs, d_items, d_w, d_X, d_x, d_part, d_psd, nullptr);
    } else if (ax)
        e = ax->psd_batch_masked(n_jobs, no_symbols, ni, d_jobs, d_items, np, d_plain, nm, d_mjobs, max_len, d_spec, d_Y, d_w, d_X,
                                 d_x, d_part, d_psd, nullptr);
    if (e != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        (amp && hipMemcpy(hjpow.data(), d_jpow, hjpow.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) ||
        hipMemcpy(psd, d_psd, (size_t)n_jobs * FL * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(WOFDM_E_HIP, "PSD kernels or copy-back failed: %s", hipGetErrorString(hipGetLastError()));
    // the sums over a job's len samples -> mean powers
    if (amp && amp->job_power)
        for (int j = 0; j < n_jobs; ++j)
            for (int w = 0; w < 2; ++w)
                amp->job_power[2 * j + w] = (float)((double)hjpow[(size_t)(2 * j + w)] / (double)hj[(size_t)j].len);
    return WOFDM_OK;
}

int wofdm_tx_psd_batch(int32_t n_fft, int device, int32_t n_jobs, const wofdm_psd_job *jobs, const float *w_tx,
                       int32_t n_blocks, int32_t no_symbols, const float *X, float *psd)
{
    return psd_batch("wofdm_tx_psd_batch", n_fft, device, n_jobs, jobs, w_tx, 0, nullptr, nullptr, nullptr, n_blocks,
                     no_symbols, X, psd);
}

int wofdm_tx_psd_batch_masked(int32_t n_fft, int device, int32_t n_jobs, const wofdm_psd_job *jobs, const float *w_tx,
                              int32_t n_masks, const int32_t *mask_len, const float *mask_gain, const int32_t *job_mask,
                              int32_t n_blocks, int32_t no_symbols, const float *X, float *psd)
{
    return psd_batch("wofdm_tx_psd_batch_masked", n_fft, device, n_jobs, jobs, w_tx, n_masks, mask_len, mask_gain, job_mask,
                     n_blocks, no_symbols, X, psd);
}

int wofdm_tx_psd_batch_pa(int32_t n_fft, int device, int32_t n_jobs, const wofdm_psd_job *jobs, const float *w_tx,
                          int32_t n_masks, const int32_t *mask_len, const float *mask_gain, const int32_t *job_mask,
                          int32_t n_pa, const wofdm_pa_point *pa, const int32_t *job_pa, int32_t n_blocks, int32_t no_symbols,
                          const float *X, float *psd, float *job_power)
{
    const psd_pa_args amp = {n_pa, pa, job_pa, job_power};
    return psd_batch("wofdm_tx_psd_batch_pa", n_fft, device, n_jobs, jobs, w_tx, n_masks, mask_len, mask_gain, job_mask, n_blocks,
                     no_symbols, X, psd, &amp);
}

// Every argument is checked before the first HIP call; the caller's arrays are written only after everything has succeeded.
int wofdm_tx_papr(const wofdm_cfg *cfg, int device, const float *w_tx, const uint8_t *active, const float *tx_mask,
                  float lo_db, float step_db, int32_t n_bins, uint64_t *hist, float *max_papr, float *periods)
{
    if (!cfg || !w_tx || !hist) return fail(WOFDM_E_INVALID, "NULL argument");
    int rc = check_tx_grid(cfg);
    if (rc != WOFDM_OK) return rc;
    const tx_geom g = tx_geom_of(cfg);
    const int N = g.N, S = g.S, P = g.P;
    if (cfg->cp < 0 || cfg->cs < 0 || g.beta < 0 || !tx_symbol_fits(cfg, g)) return fail(WOFDM_E_INVALID, "bad cp / cs / tail_tx");
    if (cfg->n_window_pairs < 1) return fail(WOFDM_E_INVALID, "n_window_pairs must be >= 1");
    if (n_bins < 1) return fail(WOFDM_E_INVALID, "n_bins=%d", n_bins);
    if (!(step_db > 0.f) || !std::isfinite(step_db) || !std::isfinite(lo_db))
        return fail(WOFDM_E_INVALID, "step_db must be positive and finite, lo_db finite");
    const uint64_t pairs = (uint64_t)cfg->n_window_pairs, frames = cfg->frames_per_cell;
    // (the pair is the cell of the label stream and shares its counter word with the stream id; w_off of the job tables is 32-bit)
    if (pairs >= (1u << 28) || pairs * (uint64_t)P > (uint64_t)INT32_MAX)
        return fail(WOFDM_E_UNSUPPORTED, "too many window pairs (2^28 cells, 2^31 window samples)");
    if (n_bins > WOFDM_PAPR_MAX_BINS) return fail(WOFDM_E_UNSUPPORTED, "n_bins=%d exceeds %d", n_bins, WOFDM_PAPR_MAX_BINS);
    if (frames > (UINT64_MAX >> 6) / pairs) return fail(WOFDM_E_UNSUPPORTED, "pairs * frames_per_cell * syms_per_frame overflows");
    if ((rc = check_mask_length(tx_mask, g)) != WOFDM_OK) return rc;
    const uint64_t items = pairs * frames, n_periods = items * (uint64_t)S;
    if (periods && n_periods > WOFDM_TX_PAPR_MAX_PERIODS)
        return fail(WOFDM_E_UNSUPPORTED, "periods is a diagnostic output: at most %d periods (%llu asked for)",
                    WOFDM_TX_PAPR_MAX_PERIODS, (unsigned long long)n_periods);
    std::vector<uint8_t> hact;
    if ((rc = check_allocation(active, N, &hact)) != WOFDM_OK || (rc = check_mask_gains(tx_mask, g)) != WOFDM_OK) return rc;
    rc = use_device(device);
    if (rc != WOFDM_OK) return rc;
    g_papr_ms = 0.f;
    if (items == 0) return WOFDM_OK;
    // frames per chunk: what the budget holds (symbol grid + waveform + filtered symbols of a frame), as the header documents it
    const uint64_t job_bytes = 8ull * ((uint64_t)S * N + (uint64_t)g.T + (tx_mask ? (uint64_t)S * g.Lm : 0ull));
    const uint64_t chunk = chunk_frames(items, WOFDM_TX_PAPR_CHUNK_BYTES, job_bytes);
    const size_t n_hist = (size_t)pairs * n_bins;
    tx_shared sh;
    tx_chain tx;
    dev_buf<float2> d_per;
    dev_buf<unsigned long long> d_hist;
    dev_buf<uint32_t> d_max;
    if ((rc = sh.stage(w_tx, (size_t)pairs * P, tx_mask, g)) != WOFDM_OK ||
        (rc = tx.stage(g, S, (size_t)chunk, hact, tx_mask != nullptr, "")) != WOFDM_OK)
        return rc;
    if (!d_hist.alloc(n_hist) || !d_max.alloc((size_t)pairs) || (periods && !d_per.alloc((size_t)n_periods)))
        return fail(WOFDM_E_NOMEM, "device allocation failed");
    if (hipMemset(d_hist, 0, n_hist * 8) != hipSuccess || hipMemset(d_max, 0, (size_t)pairs * 4) != hipSuccess)
        return fail(WOFDM_E_HIP, "upload failed");
    wofdm_pparams pp = tx.params(cfg, g, S, 1, sh);
    pp.n_bins = n_bins; pp.lo_db = lo_db; pp.step_db = step_db;
    pp.hist = d_hist; pp.max_bits = d_max; pp.periods = d_per;
    std::vector<unsigned long long> hh(n_hist);
    std::vector<uint32_t> hmax((size_t)pairs);
    std::vector<float> hper(periods ? (size_t)n_periods * 2 : 0);
    float ms = 0.f;
    hipError_t e = hipSuccess;
    const wofdm_aux_fns *ax = wofdm_aux(N);
    rc = run_chunks(items, chunk, [&](uint64_t item0, int32_t n_jobs) {
        pp.item0 = item0;
        pp.n_jobs = n_jobs;
        return ax ? ax->papr(&pp, nullptr) : hipErrorInvalidValue;
    }, &e, &ms);
    if (rc != WOFDM_OK) return rc;
    if (e != hipSuccess || hipMemcpy(hh.data(), d_hist, n_hist * 8, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(hmax.data(), d_max, (size_t)pairs * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        (periods && hipMemcpy(hper.data(), d_per, (size_t)n_periods * 8, hipMemcpyDeviceToHost) != hipSuccess))
        return fail(WOFDM_E_HIP, "PAPR kernels or copy-back failed: %s", hipGetErrorString(e != hipSuccess ? e : hipGetLastError()));
    for (size_t i = 0; i < n_hist; ++i) hist[i] += hh[i];
    if (max_papr)
        for (size_t p = 0; p < (size_t)pairs; ++p) {
            float v;
            memcpy(&v, &hmax[p], 4);
            max_papr[p] = std::max(max_papr[p], v);
        }
    if (periods) memcpy(periods, hper.data(), hper.size() * 4);
    g_papr_ms = ms;
    return WOFDM_OK;
}

int wofdm_tx_papr_kernel_ms(float *ms)
{
    if (!ms) return fail(WOFDM_E_INVALID, "NULL argument");
    *ms = g_papr_ms;
    return WOFDM_OK;
}

}  // extern "C"

namespace {

// A receive-profile call, whichever of the entry points made it: what every call has, and the stages that are on, each
// with its own inputs and outputs.  The entry points fill it; rx_profile_run checks it, prepares the stages, runs the chunks
// and copies back.
struct rx_call {
    const wofdm_cfg *cfg;
    int device;
    const float *w_tx, *w_rx, *h, *snr_db;
    const uint8_t *active;
    const float *tx_mask;
    uint64_t *errs;
    double *err_power;
    int32_t arm;                      // RXP_* of wofdm_link.h: the receive kernel the chunks run
    int32_t n_points;                 // the points (tracks) of the arm's point loop; 1 where it has none
    bool per_symbol;                  // the arm has a point loop, and with it the per-symbol sums behind sym_errs, sym_power
    uint64_t *sym_errs;               // (either may be null)
    double *sym_power;
    // the adjacent-band neighbour; a link call's offset and level are its points'
    struct { bool on; const uint8_t *active; const float *h; int32_t delay; float level_db; } nb;
    // the receiver's timing and carrier offsets
    struct { bool on; const wofdm_sync_point *points; } sync;
    // the channels that move within the frame; static_track: the static channel h stands behind them as one more track (it is
    // then needed, and is the only track where on is false)
    struct { bool on, static_track; const float *h_track; int32_t n_tracks, n_knots, knot_step; } dop;
    // the power amplifier; ref_optional: no reference power is needed where every point is linear
    struct { bool on, ref_optional; const wofdm_pa_point *points; const float *ref_power; double *pa_power; } amp;
    // the oscillator's phase noise
    struct { bool on; const wofdm_pn_point *points; } pn;
    // the points of wofdm_rx_profile_link, which switch the five stages above per point; as_sync, as_pn, as_pa: what a point
    // says to each of them, in the form the stage takes (its points point here)
    struct {
        bool on;
        const wofdm_link_point *points;
        std::vector<wofdm_sync_point> as_sync;
        std::vector<wofdm_pn_point> as_pn;
        std::vector<wofdm_pa_point> as_pa;
    } link;
    // the soft demapper of wofdm_rx_profile_soft
    struct { bool on; int32_t n_scales; const float *scales; double *bit_penalty, *sym_penalty; } soft;
    // the tracking receiver of wofdm_rx_profile_tracking: the comb (may be null) and a tracking point per link point
    struct { bool on; const uint8_t *pilots; const wofdm_tracking_point *points; } trk;
    // the coded link of wofdm_rx_profile_coded: the quantiser's scale, the interleaver (may be null), the codes, the counters
    // and (may be null) the soft bits themselves
    struct {
        bool on; float llr_scale; const int32_t *perm; int32_t n_codes; const wofdm_code *codes; uint64_t *code_errs; int8_t *soft_bits;
    } code;
    // the frame-spanning code of wofdm_rx_profile_coded_frame: code is on with it (code_errs null) and gives the soft bits, the
    // interleaver within a symbol and the codes; the rotation from symbol to symbol and the counters
    struct { bool on; int32_t sym_rot; uint64_t *frame_errs; } frm;
    // the LDPC code of wofdm_rx_profile_ldpc: code and frm are on with it (codes, code_errs and frame_errs null) and give the soft
    // bits, the frame interleaver and n_codes; the codes and the counters
    struct { bool on; const wofdm_ldpc_code *codes; uint64_t *ldpc_errs; } ldpc;
    // the coset view of wofdm_rx_profile_coset: code is on with it (codes, code_errs null, n_codes 0) and gives the soft bits and the
    // interleaver within a symbol; frm and ldpc stay off -- both families' codes, the rotation and the counters are here
    struct {
        bool on; int32_t n_codes; const wofdm_code *codes; int32_t n_ldpc; const wofdm_ldpc_code *ldpc_codes; int32_t sym_rot;
        uint64_t *frame_errs, *ldpc_errs;
        // wofdm_rx_profile_harq: rounds > 0, no Viterbi code, and ldpc_errs is harq_errs with WOFDM_HARQ_FIELDS counters per code
        int32_t rounds, combine;
    } coset;
    bool harq;                        // wofdm_rx_profile_harq (coset is on with it)
};

// the receive side's geometry beside the Tx chain's, and the cells of the call
struct rx_geom : tx_geom {
    int L, delta, gam, NW;
    uint64_t pairs, cpp, cells, frames;   // cpp: cells per window pair
};

// A call on its way: the geometry, what the stages prepared on the host, their device side, and the chunk the launcher takes
struct rx_run {
    const rx_call &c;
    rx_geom g;
    // host: the allocations, whether a neighbour is on the air at all, the points as the kernels read them
    std::vector<uint8_t> act, nb_act;
    bool nb;
    int max_theta;                    // the largest timing offset, or 0
    std::vector<wofdm_spoint> pts;
    std::vector<float2> base, taps;
    std::vector<wofdm_pnpoint> pn;
    std::vector<wofdm_lpoint> lk;
    std::vector<wofdm_papoint> pa;
    std::vector<float> asat;
    std::vector<uint8_t> pil;         // the comb as 0 / 1, empty without one
    std::vector<wofdm_tpoint> tp;
    std::vector<int32_t> gather;      // the coded link: byte 8 n + i of coded-stream index c in a symbol's soft bits
    int32_t csteps[WOFDM_CODE_CODES];
    // the frame-spanning code: per variant (0: the points without post, S_d = S - 1; 1: those with, S_d = S - 2; wofdm_link.h)
    // whether a point uses it, the codeword's positions, the gather table, per code the steps (0: unused), and the history's blocks
    bool fuse[2];
    int32_t fnc[2], fsteps[WOFDM_CODE_CODES][2], hist_blocks;
    std::vector<int32_t> fgather[2];
    // the LDPC code: per variant the words of a frame and their positions (0: unused), per code and variant the lift
    int32_t lW[2], ln[2], lZ[WOFDM_CODE_CODES][2];
    size_t n_lerr;
    dev_buf<unsigned long long> d_lerrs;
    int n_knots, knot_step;
    // device
    size_t chunk, n_out, n_sym, n_ptot, n_bpen, n_spen, n_cerr, n_ferr;
    dev_buf<int32_t> d_fgather[2];
    dev_buf<unsigned long long> d_hist, d_ferrs;
    dev_buf<int8_t> d_sbits;
    dev_buf<int32_t> d_gather;
    dev_buf<unsigned long long> d_cerrs;
    tx_shared sh;
    tx_chain tx, nbtx;
    dev_buf<float> d_wr, d_nlin, d_ppow, d_spow, d_asat, d_pwr, d_w2, d_bpart, d_spart;
    dev_buf<float2> d_h, d_hi, d_base, d_y;
    dev_buf<uint32_t> d_pcnt, d_scnt;
    dev_buf<unsigned long long> d_errs, d_serrs;
    dev_buf<double> d_pow, d_stot, d_ptot, d_walk, d_btot, d_sptot;
    dev_buf<wofdm_spoint> d_pts;
    dev_buf<wofdm_papoint> d_papts;
    dev_buf<wofdm_pnpoint> d_pnpts;
    dev_buf<wofdm_lpoint> d_lkpts;
    dev_buf<uint8_t> d_pil;
    dev_buf<wofdm_tpoint> d_tp;
    wofdm_rxchunk ck;
    int n_tracks() const { return c.dop.on ? c.dop.n_tracks : 0; }
};

bool all_finite(const float *a, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(a[i])) return false;
    return true;
}

// ---- the checks, in the order a caller meets them: the NULL arguments and the stages' counts, the geometry, the finiteness ----

int check_rx_args(const rx_call &c)
{
    if (!c.cfg || !c.w_tx || !c.w_rx || ((!c.dop.on || c.dop.static_track) && !c.h) || (c.dop.on && !c.dop.h_track) || !c.snr_db ||
        !c.errs)
        return fail(WOFDM_E_INVALID, "NULL argument");
    if (c.amp.on) {
        bool needs_ref = !c.amp.ref_optional;
        for (int i = 0; c.amp.ref_optional && c.amp.points && i < c.n_points; ++i)
            needs_ref |= c.amp.points[i].model != WOFDM_PA_LINEAR;
        if (!c.amp.points || (!c.amp.ref_power && needs_ref)) return fail(WOFDM_E_INVALID, "NULL argument (points or ref_power)");
        if (c.n_points < 1) return fail(WOFDM_E_INVALID, "n_points=%d must be >= 1", c.n_points);
    }
    if (c.nb.on && !c.nb.active) return fail(WOFDM_E_INVALID, "NULL argument (aci_active)");
    // (where both stages are on their points are the link call's, which has checked them)
    if ((c.sync.on && !c.sync.points) || (c.pn.on && !c.pn.points)) return fail(WOFDM_E_INVALID, "NULL argument (points)");
    if ((c.sync.on || c.pn.on) && c.n_points < 1) return fail(WOFDM_E_INVALID, "n_points=%d must be >= 1", c.n_points);
    if (c.dop.on && (c.dop.n_tracks < 1 || c.dop.n_knots < 2 || c.dop.knot_step < 1))
        return fail(WOFDM_E_INVALID, "n_tracks=%d must be >= 1, n_knots=%d >= 2, knot_step=%d >= 1", c.dop.n_tracks, c.dop.n_knots,
                    c.dop.knot_step);
    return WOFDM_OK;
}

int check_rx_geometry(const rx_call &c, rx_geom *out)
{
    const wofdm_cfg *cfg = c.cfg;
    int rc = check_tx_grid(cfg);
    if (rc != WOFDM_OK) return rc;
    const int N = cfg->n_fft, L = cfg->n_taps;
    if (cfg->n_channels < 1 || cfg->n_snr < 1 || cfg->n_window_pairs < 1)
        return fail(WOFDM_E_INVALID, "n_channels, n_snr, n_window_pairs must be >= 1");
    if (cfg->cp < 0 || cfg->cs < 0 || cfg->tail_tx < 0 || cfg->tail_rx < 0 || cfg->prefix_rm < 0 || cfg->circ_shift < 0 ||
        cfg->circ_shift >= N || L < 1)
        return fail(WOFDM_E_INVALID, "negative length, n_taps < 1 or circ_shift >= n_fft");
    if (L > WOFDM_MAX_TAPS) return fail(WOFDM_E_UNSUPPORTED, "n_taps=%d exceeds %d", L, WOFDM_MAX_TAPS);
    rx_geom &g = *out;
    static_cast<tx_geom &>(g) = tx_geom_of(cfg);
    g.L = L; g.delta = cfg->tail_rx; g.gam = cfg->prefix_rm; g.NW = N + g.delta;
    if ((g.delta & 1) || g.delta > 64) return fail(WOFDM_E_UNSUPPORTED, "tail_rx=%d must be even and <= 64", g.delta);
    if (!tx_symbol_fits(cfg, g)) return fail(WOFDM_E_UNSUPPORTED, "cp, cs <= n_fft and 2 tail_tx <= P required");
    if (N + g.delta + g.gam != g.B)
        return fail(WOFDM_E_UNSUPPORTED, "n_fft+tail_rx+prefix_rm (%d) != n_fft+cp+cs-tail_tx (%d)", N + g.delta + g.gam, g.B);
    if ((rc = check_mask_length(c.tx_mask, g)) != WOFDM_OK) return rc;
    g.pairs = (uint64_t)cfg->n_window_pairs; g.cpp = (uint64_t)cfg->n_snr * (uint64_t)cfg->n_channels;
    g.cells = g.pairs * g.cpp; g.frames = cfg->frames_per_cell;
    // (the cell shares its counter word with the stream id; w_off of the job tables is 32-bit)
    if (g.cells >= (1u << 28) || g.pairs * (uint64_t)g.P > (uint64_t)INT32_MAX)
        return fail(WOFDM_E_UNSUPPORTED, "too many cells (2^28) or window samples (2^31)");
    if (g.frames > (UINT64_MAX >> 6) / g.cells) return fail(WOFDM_E_UNSUPPORTED, "cells * frames_per_cell * syms_per_frame overflows");
    return WOFDM_OK;
}

int check_rx_finite(const rx_call &c, const rx_geom &g)
{
    if (!all_finite(c.w_tx, (size_t)g.pairs * g.P) || !all_finite(c.w_rx, (size_t)g.pairs * g.NW))
        return fail(WOFDM_E_INVALID, "windows must be finite");
    if ((!c.dop.on || c.dop.static_track) && !all_finite(c.h, (size_t)c.cfg->n_channels * g.L * 2))
        return fail(WOFDM_E_INVALID, "channel taps must be finite");
    if (!all_finite(c.snr_db, (size_t)c.cfg->n_snr)) return fail(WOFDM_E_INVALID, "SNR points must be finite");
    return check_mask_gains(c.tx_mask, g);
}

// ---- the stages' host side: a stage's points checked, and turned into what the kernels read ----

// the neighbour: an allocation that loads no bin is "no neighbour" (nb stays false), and the call takes the route without one
int prep_nb(rx_run &r)
{
    const auto &nb = r.c.nb;
    if (!nb.on) return WOFDM_OK;
    if (!std::isfinite(nb.level_db) || !std::isfinite((float)std::pow(10.0, 0.05 * (double)nb.level_db)))
        return fail(WOFDM_E_INVALID, "aci_level_db must be finite, and so the amplitude 10^(level / 20) in single precision");
    if (nb.delay < 0) return fail(WOFDM_E_INVALID, "aci_delay=%d is negative", nb.delay);
    if (nb.delay >= r.g.B)
        return fail(WOFDM_E_UNSUPPORTED, "aci_delay=%d must be below the symbol stride B = %d", nb.delay, r.g.B);
    if (nb.h && !all_finite(nb.h, (size_t)r.c.cfg->n_channels * r.g.L * 2)) return fail(WOFDM_E_INVALID, "aci_h taps must be finite");
    r.nb_act.resize((size_t)r.g.N);
    for (int n = 0; n < r.g.N; ++n) r.nb |= (r.nb_act[(size_t)n] = nb.active[n] ? 1 : 0) != 0;
    return WOFDM_OK;
}

// the receiver offsets: the base phasor of every (point, symbol) in double precision, from cfo as stored
int prep_sync(rx_run &r)
{
    if (!r.c.sync.on) return WOFDM_OK;
    const int NP = r.c.n_points, S = r.g.S, B = r.g.B;
    if (NP > WOFDM_SYNC_MAX_POINTS) return fail(WOFDM_E_UNSUPPORTED, "n_points=%d exceeds %d", NP, WOFDM_SYNC_MAX_POINTS);
    for (int i = 0; i < NP; ++i) {
        const wofdm_sync_point &q = r.c.sync.points[i];
        if (!std::isfinite(q.cfo)) return fail(WOFDM_E_INVALID, "points[%d].cfo must be finite", i);
        if (q.reserved != 0) return fail(WOFDM_E_INVALID, "points[%d].reserved=%d must be 0", i, q.reserved);
        if (q.cfo_tracked != 0 && q.cfo_tracked != 1)
            return fail(WOFDM_E_INVALID, "points[%d].cfo_tracked=%d must be 0 or 1", i, q.cfo_tracked);
    }
    r.pts.resize((size_t)NP);
    r.base.resize((size_t)NP * S);
    for (int i = 0; i < NP; ++i) {
        const wofdm_sync_point &q = r.c.sync.points[i];
        if ((int64_t)q.timing >= (int64_t)B || (int64_t)q.timing <= -(int64_t)B)
            return fail(WOFDM_E_UNSUPPORTED, "points[%d].timing=%d must lie inside (-B, B), B = %d", i, q.timing, B);
        if (std::fabs(q.cfo) > 4.0f)
            return fail(WOFDM_E_UNSUPPORTED, "points[%d].cfo=%g exceeds 4 subcarrier spacings", i, (double)q.cfo);
        r.pts[(size_t)i].theta = q.timing;
        r.max_theta = std::max(r.max_theta, (int)q.timing);
        r.pts[(size_t)i].eps = q.cfo;
        for (int s = 0; s < S; ++s) {
            // eps (s B + gam + theta) / N is exact in double: 24 bits times less than 2^16, over a power of two
            const double turns = (double)q.cfo * (double)(s * B + r.g.gam + q.timing) / (double)r.g.N;
            const double ph = 2.0 * 3.14159265358979323846 * (turns - std::nearbyint(turns));
            r.base[(size_t)i * S + s] = q.cfo_tracked ? make_float2(1.f, 0.f) : make_float2((float)std::cos(ph), (float)std::sin(ph));
        }
    }
    return WOFDM_OK;
}

// the phase noise: sigma / (2 pi) = sqrt(beta / (2 pi n_fft)) of every point in double precision, from beta as stored
int prep_pn(rx_run &r)
{
    if (!r.c.pn.on) return WOFDM_OK;
    const int NP = r.c.n_points;
    if (NP > WOFDM_PN_MAX_POINTS) return fail(WOFDM_E_UNSUPPORTED, "n_points=%d exceeds %d", NP, WOFDM_PN_MAX_POINTS);
    for (int i = 0; i < NP; ++i) {
        const wofdm_pn_point &q = r.c.pn.points[i];
        if (!std::isfinite(q.linewidth) || q.linewidth < 0.f)
            return fail(WOFDM_E_INVALID, "points[%d].linewidth must be finite and >= 0", i);
        if (q.cpe_tracked != 0 && q.cpe_tracked != 1)
            return fail(WOFDM_E_INVALID, "points[%d].cpe_tracked=%d must be 0 or 1", i, q.cpe_tracked);
        if (q.reserved[0] != 0 || q.reserved[1] != 0) return fail(WOFDM_E_INVALID, "points[%d].reserved must be 0", i);
    }
    r.pn.resize((size_t)NP);
    for (int i = 0; i < NP; ++i) {
        const wofdm_pn_point &q = r.c.pn.points[i];
        if (q.linewidth > 1.0f)
            return fail(WOFDM_E_UNSUPPORTED, "points[%d].linewidth=%g exceeds 1 subcarrier spacing", i, (double)q.linewidth);
        r.pn[(size_t)i].turn = std::sqrt((double)q.linewidth / (2.0 * 3.14159265358979323846 * (double)r.g.N));
        r.pn[(size_t)i].tracked = q.cpe_tracked;
        r.pn[(size_t)i].pad = 0;
    }
    return WOFDM_OK;
}

// the moving channels: every knot finite, and the knots reach the last sample of conv, index T + L - 2 -- under receiver
// offsets a late window takes taps max_theta samples further on
int check_knots(const rx_run &r)
{
    const auto &dop = r.c.dop;
    if (!dop.on) return WOFDM_OK;
    if (dop.n_tracks > WOFDM_DOPPLER_MAX_TRACKS)
        return fail(WOFDM_E_UNSUPPORTED, "n_tracks=%d exceeds %d", dop.n_tracks, WOFDM_DOPPLER_MAX_TRACKS);
    if (dop.n_knots > WOFDM_DOPPLER_MAX_KNOTS) return fail(WOFDM_E_UNSUPPORTED, "n_knots=%d exceeds %d", dop.n_knots, WOFDM_DOPPLER_MAX_KNOTS);
    if (!all_finite(dop.h_track, (size_t)dop.n_tracks * r.c.cfg->n_channels * dop.n_knots * r.g.L * 2))
        return fail(WOFDM_E_INVALID, "channel knots must be finite");
    const int last = r.g.T + r.g.L - 2 + r.max_theta;
    if ((int64_t)(dop.n_knots - 1) * (int64_t)dop.knot_step < (int64_t)last)
        return fail(WOFDM_E_INVALID, "the knots end at sample %lld, the frame's last at %d: (n_knots - 1) knot_step >= "
                    "tail_tx + S B + n_taps - 2%s required", (long long)(dop.n_knots - 1) * dop.knot_step, last,
                    r.c.sync.on ? " + the largest positive timing" : "");
    return WOFDM_OK;
}

// the link points' own part: the track and the neighbour of every point; a neighbour no point switches on is no neighbour
int prep_link(rx_run &r)
{
    if (!r.c.link.on) return WOFDM_OK;
    const int NP = r.c.n_points, NTR = r.n_tracks(), B = r.g.B;
    for (int i = 0; i < NP; ++i) {
        const wofdm_link_point &q = r.c.link.points[i];
        if (q.track < -1 || q.track >= NTR) return fail(WOFDM_E_INVALID, "points[%d].track=%d must be -1 or below n_tracks=%d", i, q.track, NTR);
        if (q.aci_on != 0 && q.aci_on != 1) return fail(WOFDM_E_INVALID, "points[%d].aci_on=%d must be 0 or 1", i, q.aci_on);
        if (q.reserved[0] != 0 || q.reserved[1] != 0 || q.reserved[2] != 0 || q.reserved[3] != 0)
            return fail(WOFDM_E_INVALID, "points[%d].reserved must be 0", i);
        if (!std::isfinite(q.aci_level_db) || !std::isfinite((float)std::pow(10.0, 0.05 * (double)q.aci_level_db)))
            return fail(WOFDM_E_INVALID, "points[%d].aci_level_db must be finite, and so the amplitude 10^(level / 20)", i);
        if (q.aci_delay < 0) return fail(WOFDM_E_INVALID, "points[%d].aci_delay=%d is negative", i, q.aci_delay);
    }
    r.lk.resize((size_t)NP);
    bool any_nb = false;
    for (int i = 0; i < NP; ++i) {
        const wofdm_link_point &q = r.c.link.points[i];
        if (q.aci_delay >= B)
            return fail(WOFDM_E_UNSUPPORTED, "points[%d].aci_delay=%d must be below the symbol stride B = %d", i, q.aci_delay, B);
        // (an allocation that loads no bin is "no neighbour", as in wofdm_rx_profile_aci; the static track is the last)
        r.lk[(size_t)i] = {q.track < 0 ? NTR : q.track, q.aci_on && r.nb ? 1 : 0, B - q.aci_delay,
                           (float)std::pow(10.0, 0.05 * (double)q.aci_level_db)};
        any_nb |= r.lk[(size_t)i].aci_on != 0;
    }
    r.nb = any_nb;
    return WOFDM_OK;
}

// the amplifier: the points, and the saturation amplitude of every (point, pair) in double precision, stored in single
int prep_amp(rx_run &r)
{
    const auto &amp = r.c.amp;
    if (!amp.on) return WOFDM_OK;
    const int NP = r.c.n_points;
    const uint64_t pairs = r.g.pairs;
    const int prc = check_pa_points(NP, amp.points, &r.pa);
    if (prc != WOFDM_OK) return prc;
    r.asat.assign((size_t)NP * pairs, 1.f);                           // (every point linear and no ref_power: never read)
    for (uint64_t p = 0; amp.ref_power && p < pairs; ++p)
        if (!std::isfinite(amp.ref_power[p]) || !(amp.ref_power[p] > 0.f))
            return fail(WOFDM_E_INVALID, "ref_power[%llu] must be finite and positive", (unsigned long long)p);
    for (int i = 0; amp.ref_power && i < NP; ++i)
        for (uint64_t p = 0; p < pairs; ++p) {
            // (the root of a positive single-precision number times 10^-4 ... 10^6 is a normal single-precision number)
            r.asat[(size_t)i * pairs + p] = (float)std::sqrt((double)amp.ref_power[p] * std::pow(10.0, 0.1 * (double)amp.points[i].ibo_db));
        }
    return WOFDM_OK;
}

// the tracking receiver, in the order include/wofdm.h documents: the comb -- every pilot on a loaded bin, a data bin left --, then
// point by point the flags, reserved, post against S, cpe against the comb
int prep_track(rx_run &r)
{
    const auto &trk = r.c.trk;
    if (!trk.on) return WOFDM_OK;
    const int N = r.g.N, NP = r.c.n_points;
    int n_pil = 0, n_data = 0;
    const auto loaded = [&](int n) { return r.act.empty() || r.act[(size_t)n] != 0; };   // (no allocation: every bin)
    if (trk.pilots) {
        r.pil.resize((size_t)N);
        for (int n = 0; n < N; ++n) {
            r.pil[(size_t)n] = trk.pilots[n] ? 1 : 0;
            if (trk.pilots[n] && !loaded(n)) return fail(WOFDM_E_INVALID, "pilots[%d] is set on a bin that is not loaded", n);
            n_pil += trk.pilots[n] ? 1 : 0;
        }
    }
    for (int n = 0; n < N; ++n) n_data += loaded(n) && !(trk.pilots && trk.pilots[n]) ? 1 : 0;
    if (n_data < 1) return fail(WOFDM_E_INVALID, "the comb leaves no data bin");
    r.tp.resize((size_t)NP);
    for (int i = 0; i < NP; ++i) {
        const wofdm_tracking_point &q = trk.points[i];
        if ((q.cpe != 0 && q.cpe != 1) || (q.post != 0 && q.post != 1))
            return fail(WOFDM_E_INVALID, "tracking[%d]: cpe=%d and post=%d must be 0 or 1", i, q.cpe, q.post);
        if (q.reserved[0] != 0 || q.reserved[1] != 0) return fail(WOFDM_E_INVALID, "tracking[%d].reserved must be 0", i);
        if (q.post && r.g.S < 3) return fail(WOFDM_E_INVALID, "tracking[%d].post needs syms_per_frame >= 3, not %d", i, r.g.S);
        if (q.cpe && n_pil < 1) return fail(WOFDM_E_INVALID, "tracking[%d].cpe needs at least one pilot bin", i);
        r.tp[(size_t)i] = {q.cpe, q.post};
    }
    return WOFDM_OK;
}

// the largest T whose kept outputs number at most n_c (include/wofdm.h): rate 1/2 keeps 2 per step; 2/3 (A 1 1, B 1 0) 3 per
// period of 2, 2 in its first step; 3/4 (A 1 1 0, B 1 0 1) 4 per period of 3, 2 in its first step and 1 in its second
int32_t code_steps(int32_t rate, int64_t n_c)
{
    if (rate == 0) return (int32_t)(n_c / 2);
    if (rate == 1) return (int32_t)(2 * (n_c / 3) + (n_c % 3 == 2 ? 1 : 0));
    const int64_t rem = n_c % 4;
    return (int32_t)(3 * (n_c / 4) + (rem >= 3 ? 2 : (rem == 2 ? 1 : 0)));
}

bool is_permutation(const int32_t *perm, int64_t n)
{
    std::vector<uint8_t> seen((size_t)n, 0);
    for (int64_t c = 0; c < n; ++c) {
        if (perm[c] < 0 || perm[c] >= n || seen[(size_t)perm[c]]) return false;
        seen[(size_t)perm[c]] = 1;
    }
    return true;
}

// the coded link, in the order include/wofdm.h documents; leaves the gather table of a symbol's soft bits: coded-stream index c
// reads position j = perm[c] = r k + i, bit i of the r-th data bin n, at byte 8 n + i
int prep_code(rx_run &r)
{
    const auto &cd = r.c.code;
    if (!cd.on) return WOFDM_OK;
    const bool frame = r.c.frm.on;                                     // (its counters and lengths: prep_frame)
    const bool ldpc = r.c.ldpc.on;                                     // (its codes are checked behind the frame's: prep_frame)
    const bool coset = r.c.coset.on;                                   // (its counts and codes come behind perm: prep_coset)
    if (!coset && (ldpc ? !r.c.ldpc.codes : (!cd.codes || (!frame && !cd.code_errs))))
        return fail(WOFDM_E_INVALID, "NULL argument (codes or code_errs)");
    if (!std::isfinite(cd.llr_scale) || !(cd.llr_scale > 0.f)) return fail(WOFDM_E_INVALID, "llr_scale must be finite and positive");
    if (!coset && cd.n_codes < 1) return fail(WOFDM_E_INVALID, "n_codes=%d must be >= 1", cd.n_codes);
    if (!coset && cd.n_codes > WOFDM_CODE_MAX) return fail(WOFDM_E_UNSUPPORTED, "n_codes=%d exceeds %d", cd.n_codes, WOFDM_CODE_MAX);
    const int N = r.g.N, k = r.g.k;
    std::vector<int32_t> bins;
    for (int n = 0; n < N; ++n)
        if ((r.act.empty() || r.act[(size_t)n] != 0) && (r.pil.empty() || r.pil[(size_t)n] == 0)) bins.push_back(n);
    const int32_t n_c = k * (int32_t)bins.size();
    for (int i = 0; !ldpc && i < cd.n_codes; ++i) {
        const wofdm_code &q = cd.codes[i];
        if (q.rate < 0 || q.rate > 2) return fail(WOFDM_E_INVALID, "codes[%d].rate=%d must be 0, 1 or 2", i, q.rate);
        if (q.reserved[0] != 0 || q.reserved[1] != 0 || q.reserved[2] != 0) return fail(WOFDM_E_INVALID, "codes[%d].reserved must be 0", i);
        r.csteps[i] = code_steps(q.rate, n_c);
        if (!frame && r.csteps[i] < 7)
            return fail(WOFDM_E_INVALID, "codes[%d]: %d coded bits per symbol give %d steps, at least 7 are needed", i, n_c, r.csteps[i]);
    }
    if (cd.perm && !is_permutation(cd.perm, n_c)) return fail(WOFDM_E_INVALID, "perm is not a permutation of 0 ... %d", n_c - 1);
    const uint64_t bytes = r.g.cells * r.g.frames * (uint64_t)r.c.n_points * (uint64_t)(r.g.S - 1) * (uint64_t)N * 8;
    if (cd.soft_bits && bytes > (1ull << 30))
        return fail(WOFDM_E_UNSUPPORTED, "soft_bits of %llu bytes exceed 2^30", (unsigned long long)bytes);
    r.gather.resize((size_t)n_c);
    for (int32_t c = 0; c < n_c; ++c) {
        const int32_t j = cd.perm ? cd.perm[c] : c;
        r.gather[(size_t)c] = 8 * bins[(size_t)(j / k)] + j % k;
    }
    return WOFDM_OK;
}

// The lift of the (J, L) code over n positions (include/wofdm.h): the smallest prime Z >= max(L, ceil(n / L)) whose
// multiplicative order of 2 is at least L; the caller has checked the ranges
int32_t ldpc_lift(int32_t J, int32_t L, int32_t n)
{
    (void)J;
    for (int32_t Z = std::max(L, (n + L - 1) / L);; ++Z) {
        bool ok = Z >= 3;
        for (int32_t d = 2; ok && d * d <= Z; ++d) ok = Z % d != 0;
        int32_t p = 2 % Z;
        for (int32_t k = 1; ok && k < L; ++k) {                          // 2^k != 1 for 0 < k < L
            ok = p != 1;
            p = (2 * p) % Z;
        }
        if (ok) return Z;
    }
}
bool ldpc_ranges_ok(int32_t J, int32_t L) { return J >= 3 && J <= 6 && L > J && L <= 24; }

// the LDPC codes of wofdm_rx_profile_ldpc, behind prep_frame's sym_rot and ldpc_errs, code by code in the order include/wofdm.h
// documents: a frame of n_f positions carries W = ceil(n_f / WOFDM_LDPC_MAX_BITS) words of n = floor(n_f / W) positions
// (the coset view's codes likewise, behind prep_coset's; its decoder keeps the transmitted word in LDS as well)
int prep_ldpc(rx_run &r, const wofdm_ldpc_code *codes, int32_t n_codes, bool coset)
{
    for (int v = 0; v < 2; ++v) {
        r.lW[v] = r.fnc[v] > 0 ? (r.fnc[v] + WOFDM_LDPC_MAX_BITS - 1) / WOFDM_LDPC_MAX_BITS : 0;
        r.ln[v] = r.lW[v] > 0 ? r.fnc[v] / r.lW[v] : 0;
    }
    for (int i = 0; i < n_codes; ++i) {
        const wofdm_ldpc_code &q = codes[i];
        const char *name = coset ? "ldpc_codes" : "codes";
        if (q.J < 3 || q.J > 6) return fail(WOFDM_E_INVALID, "%s[%d].J=%d must be 3 ... 6", name, i, q.J);
        if (q.L <= q.J || q.L > 24) return fail(WOFDM_E_INVALID, "%s[%d].L=%d must be J + 1 ... 24", name, i, q.L);
        if (q.max_iter < 1 || q.max_iter > 64) return fail(WOFDM_E_INVALID, "%s[%d].max_iter=%d must be 1 ... 64", name, i, q.max_iter);
        if (q.reserved != 0) return fail(WOFDM_E_INVALID, "%s[%d].reserved must be 0", name, i);
        for (int v = 0; v < 2; ++v) {
            r.lZ[i][v] = r.lW[v] > 0 ? ldpc_lift(q.J, q.L, r.ln[v]) : 0;
            if (r.lW[v] > 0 && (int64_t)(q.L - q.J) * r.lZ[i][v] - ((int64_t)q.L * r.lZ[i][v] - r.ln[v]) < 1)
                return fail(WOFDM_E_INVALID, "%s[%d]: (%d, %d) over %d positions has no information bit", name, i, q.J, q.L, r.ln[v]);
            if (r.lW[v] > 0 &&
                (coset ? wofdm_ldpc_coset_lds(q.J, q.L, r.lZ[i][v]) : wofdm_ldpc_lds(q.J, q.L, r.lZ[i][v])) > WOFDM_LDPC_LDS_MAX)
                return fail(WOFDM_E_UNSUPPORTED, "%s[%d]: the decoder's LDS exceeds %d bytes", name, i, WOFDM_LDPC_LDS_MAX);
        }
    }
    return WOFDM_OK;
}

// wofdm_viterbi_decode_long and the frame-spanning code: the history is 512 bytes per block of 64 steps
int32_t hist_blocks_of(int32_t steps) { return (steps + 63) / 64; }

// the variants a call's points use and their coded-stream lengths
void frame_lengths(rx_run &r)
{
    const int32_t n_c = (int32_t)r.gather.size(), S = r.g.S;
    r.fuse[0] = r.fuse[1] = false;
    for (int i = 0; i < r.c.n_points; ++i) r.fuse[r.tp[(size_t)i].post ? 1 : 0] = true;
    r.hist_blocks = 1;
    for (int v = 0; v < 2; ++v) {
        const int64_t s_d = S - 1 - v;
        r.fnc[v] = r.fuse[v] && s_d >= 1 ? (int32_t)((int64_t)n_c * s_d) : 0;       // (n_c <= 6 * 1024, S <= 64)
    }
}
// the Viterbi codes' steps per variant, and the history's blocks
int frame_steps(rx_run &r, const wofdm_code *codes, int32_t n_codes)
{
    for (int pass = 0; pass < 2; ++pass)                                 // (every T < 7 before any T beyond the limit)
        for (int i = 0; i < n_codes; ++i)
            for (int v = 0; v < 2; ++v) {
                const int32_t T = r.fnc[v] > 0 ? code_steps(codes[i].rate, r.fnc[v]) : 0;
                r.fsteps[i][v] = T;
                if (r.fnc[v] == 0) continue;
                if (pass == 0 && T < 7)
                    return fail(WOFDM_E_INVALID, "codes[%d]: %d coded bits per frame give %d steps, at least 7 are needed", i, r.fnc[v], T);
                if (pass == 1 && T > WOFDM_CODE_LONG_MAX_STEPS)
                    return fail(WOFDM_E_UNSUPPORTED, "codes[%d]: %d steps, more than %d", i, T, WOFDM_CODE_LONG_MAX_STEPS);
                r.hist_blocks = std::max(r.hist_blocks, hist_blocks_of(T));
            }
    return WOFDM_OK;
}
// the frame's gather tables per variant
void frame_gathers(rx_run &r, int32_t sym_rot)
{
    const int32_t n_c = (int32_t)r.gather.size(), S = r.g.S, N = r.g.N;
    for (int v = 0; v < 2; ++v) {
        const int32_t s_d = S - 1 - v;
        r.fgather[v].resize((size_t)r.fnc[v]);
        for (int32_t c = 0; c < r.fnc[v]; ++c) {
            const int32_t j = c % s_d, q = c / s_d;
            r.fgather[v][(size_t)c] = 8 * N * j + r.gather[(size_t)(((int64_t)q + (int64_t)j * sym_rot) % n_c)];
        }
    }
}

// the frame-spanning code, in the order include/wofdm.h documents, behind prep_code (which leaves the gather table of one symbol);
// leaves per variant the gather table of the frame: coded-stream index c sits in data symbol 1 + j, j = c mod S_d, at the
// symbol's position perm[(c div S_d + j sym_rot) mod n_c], which is byte 8 N j + gather[(c div S_d + j sym_rot) mod n_c] of the
// (frame, point)'s soft bits [S - 1][N][8]
int prep_frame(rx_run &r)
{
    const auto &fm = r.c.frm;
    if (!fm.on) return WOFDM_OK;
    const int32_t n_c = (int32_t)r.gather.size();
    if (fm.sym_rot < 0 || fm.sym_rot >= n_c) return fail(WOFDM_E_INVALID, "sym_rot=%d outside [0, %d)", fm.sym_rot, n_c);
    const bool ldpc = r.c.ldpc.on;
    if (ldpc ? !r.c.ldpc.ldpc_errs : !fm.frame_errs) return fail(WOFDM_E_INVALID, "NULL argument (%s)", ldpc ? "ldpc_errs" : "frame_errs");
    frame_lengths(r);
    const int rc = ldpc ? WOFDM_OK : frame_steps(r, r.c.code.codes, r.c.code.n_codes);
    if (rc != WOFDM_OK) return rc;
    frame_gathers(r, fm.sym_rot);
    return ldpc ? prep_ldpc(r, r.c.ldpc.codes, r.c.code.n_codes, false) : WOFDM_OK;
}

// the coset view (wofdm_rx_profile_coset), behind prep_code's llr_scale, perm and soft_bits, in the order include/wofdm.h
// documents: the counts, the code arrays, sym_rot, the counters, the Viterbi codes as wofdm_rx_profile_coded_frame checks them,
// the LDPC codes as wofdm_rx_profile_ldpc does
int prep_coset(rx_run &r)
{
    const auto &cs = r.c.coset;
    if (!cs.on) return WOFDM_OK;
    const bool harq = r.c.harq;
    if (cs.n_codes < 0 || cs.n_ldpc < 0) return fail(WOFDM_E_INVALID, "n_codes=%d and n_ldpc=%d must be >= 0", cs.n_codes, cs.n_ldpc);
    if (cs.n_codes > WOFDM_CODE_MAX || cs.n_ldpc > WOFDM_CODE_MAX)
        return fail(WOFDM_E_UNSUPPORTED, "n_codes=%d or n_ldpc=%d exceeds %d", cs.n_codes, cs.n_ldpc, WOFDM_CODE_MAX);
    if (cs.n_codes + cs.n_ldpc < 1) return fail(WOFDM_E_INVALID, harq ? "n_ldpc must be >= 1" : "n_codes + n_ldpc must be >= 1");
    if ((cs.n_codes > 0 && !cs.codes) || (cs.n_ldpc > 0 && !cs.ldpc_codes)) return fail(WOFDM_E_INVALID, "NULL argument (codes or ldpc_codes)");
    const int32_t n_c = (int32_t)r.gather.size();
    if (cs.sym_rot < 0 || cs.sym_rot >= n_c) return fail(WOFDM_E_INVALID, "sym_rot=%d outside [0, %d)", cs.sym_rot, n_c);
    if ((cs.n_codes > 0 && !cs.frame_errs) || (cs.n_ldpc > 0 && !cs.ldpc_errs))
        return fail(WOFDM_E_INVALID, harq ? "NULL argument (harq_errs)" : "NULL argument (frame_errs or ldpc_errs)");
    if (harq) {
        // wofdm_rx_profile_harq: the rounds, the combining rule, then the groups -- whole groups per cell, on the global frame index
        if (cs.rounds < 1 || cs.rounds > WOFDM_HARQ_MAX_ROUNDS)
            return fail(WOFDM_E_INVALID, "rounds=%d must be 1 ... %d", cs.rounds, WOFDM_HARQ_MAX_ROUNDS);
        if (cs.combine != 0 && cs.combine != 1) return fail(WOFDM_E_INVALID, "combine=%d must be 0 or 1", cs.combine);
        if (r.c.cfg->frames_per_cell % (uint64_t)cs.rounds != 0)
            return fail(WOFDM_E_INVALID, "frames_per_cell=%llu is no multiple of rounds=%d", (unsigned long long)r.c.cfg->frames_per_cell, cs.rounds);
        if (r.c.cfg->frame_offset % (uint64_t)cs.rounds != 0)
            return fail(WOFDM_E_INVALID, "frame_offset=%llu is no multiple of rounds=%d", (unsigned long long)r.c.cfg->frame_offset, cs.rounds);
    }
    for (int i = 0; i < cs.n_codes; ++i) {
        const wofdm_code &q = cs.codes[i];
        if (q.rate < 0 || q.rate > 2) return fail(WOFDM_E_INVALID, "codes[%d].rate=%d must be 0, 1 or 2", i, q.rate);
        if (q.reserved[0] != 0 || q.reserved[1] != 0 || q.reserved[2] != 0) return fail(WOFDM_E_INVALID, "codes[%d].reserved must be 0", i);
    }
    frame_lengths(r);
    const int rc = frame_steps(r, cs.codes, cs.n_codes);
    if (rc != WOFDM_OK) return rc;
    frame_gathers(r, cs.sym_rot);
    return prep_ldpc(r, cs.ldpc_codes, cs.n_ldpc, true);
}

// The taps as the kernels read them.  Of moving channels the knots, [n_tracks][n_channels][n_knots][WOFDM_LT], zero padded, and
// behind them the static track where the call has one: h at every knot (without a track of the caller's, two knots that cover
// every sample).  Without either, h as it is -- the static track of one knot.
void pack_channel(rx_run &r)
{
    const rx_call &c = r.c;
    const int L = r.g.L;
    r.n_knots = c.dop.on ? c.dop.n_knots : 2;
    r.knot_step = c.dop.on ? c.dop.knot_step : r.g.T + L + r.g.B;
    const size_t rows = c.dop.on ? (size_t)c.dop.n_tracks * c.cfg->n_channels * c.dop.n_knots : 0;
    r.taps.assign(rows * WOFDM_LT, make_float2(0.f, 0.f));
    for (size_t row = 0; row < rows; ++row)
        for (int l = 0; l < L; ++l)
            r.taps[row * WOFDM_LT + l] = make_float2(c.dop.h_track[2 * (row * L + l)], c.dop.h_track[2 * (row * L + l) + 1]);
    if (c.dop.on && !c.dop.static_track) return;
    geom gl{};
    gl.L = L;
    const std::vector<float2> hs = pack_taps(c.cfg, gl, c.h);
    for (int ch = 0; ch < c.cfg->n_channels; ++ch)
        for (int q = 0; q < (c.dop.static_track ? r.n_knots : 1); ++q)
            r.taps.insert(r.taps.end(), hs.begin() + (size_t)ch * WOFDM_LT, hs.begin() + (size_t)(ch + 1) * WOFDM_LT);
}

// Bytes of scratch per frame, the sum of the stages' terms as the header documents them: 8-byte words but for the demapper's
uint64_t rx_job_bytes(const rx_run &r)
{
    const rx_call &c = r.c;
    const uint64_t S = (uint64_t)r.g.S, N = (uint64_t)r.g.N, T = (uint64_t)r.g.T, B = (uint64_t)r.g.B, NP = (uint64_t)c.n_points;
    const uint64_t Lm = c.tx_mask ? (uint64_t)r.g.Lm : 0;                  // filtered symbols only under a mask
    uint64_t words = S * N + T + S * Lm;                                  // symbol grid, waveform, filtered symbols
    words += NP * N;                                                      // the partials per bin, of every point
    if (c.per_symbol) words += NP * S;                                    // the partials per symbol
    if (c.amp.on) words += NP * T;                                        // every point's amplified waveform
    if (c.pn.on) words += S * B;                                          // the unit phase walk
    if (r.nb) words += (S + 1) * N + (T + B) + (S + 1) * Lm;              // the neighbour's chain of S + 1 symbols
    // the demapper: per point and scale the penalties of every data symbol's bins and the symbols' sums, fp32
    // the coded link: 8 bytes of soft bits per point, data symbol and bin (the decoder's survivors are in LDS)
    // the frame-spanning code: 512 bytes of survivor history per point and block of 64 steps of the longest codeword, which the
    // codes' launches share
    return 8 * words + (c.soft.on ? 4 * NP * (uint64_t)c.soft.n_scales * ((S - 1) * N + S) : 0) + (c.code.on ? 8 * NP * (S - 1) * N : 0) +
           ((c.frm.on && !c.ldpc.on) || (c.coset.on && c.coset.n_codes > 0) ? 512 * NP * (uint64_t)r.hist_blocks : 0);
}

// ---- the stages' device side: allocation, upload, and the stage's parameters in the chunk ----

// the Tx chain, the receive kernel's constants, the partials per bin and the totals
int stage_base(rx_run &r)
{
    const rx_call &c = r.c;
    const rx_geom &g = r.g;
    const size_t NP = (size_t)c.n_points, n_wr = (size_t)g.pairs * g.NW, n_part = r.chunk * NP * g.N;
    std::vector<float> nlin((size_t)c.cfg->n_snr);
    for (int i = 0; i < c.cfg->n_snr; ++i) nlin[(size_t)i] = (float)std::pow(10.0, -0.1 * (double)c.snr_db[i]);
    int rc = r.sh.stage(c.w_tx, (size_t)g.pairs * g.P, c.tx_mask, g);
    if (rc == WOFDM_OK) rc = r.tx.stage(g, g.S, r.chunk, r.act, c.tx_mask != nullptr, "");
    if (rc != WOFDM_OK) return rc;
    if (!r.d_wr.alloc(n_wr) || !r.d_nlin.alloc(nlin.size()) || !r.d_h.alloc(r.taps.size()) || !r.d_ppow.alloc(n_part) ||
        !r.d_pcnt.alloc(n_part) || !r.d_errs.alloc(2 * r.n_out) || !r.d_pow.alloc(r.n_out))
        return fail(WOFDM_E_NOMEM, "device allocation failed");
    if (!r.d_wr.upload(c.w_rx, n_wr) || !r.d_nlin.upload(nlin.data(), nlin.size()) || !r.d_h.upload(r.taps.data(), r.taps.size()) ||
        hipMemset(r.d_errs, 0, 2 * r.n_out * 8) != hipSuccess || hipMemset(r.d_pow, 0, r.n_out * 8) != hipSuccess)
        return fail(WOFDM_E_HIP, "upload failed");
    r.ck.tx = r.tx.params(c.cfg, g, g.S, (uint32_t)g.cpp, r.sh);
    wofdm_rparams &rp = r.ck.r;
    rp.S = g.S; rp.k = g.k; rp.B = g.B; rp.T = g.T; rp.NL = c.cfg->noise_before_truncate ? g.T + g.L - 1 : g.S * g.B;
    rp.delta = g.delta; rp.gam = g.gam; rp.kap = c.cfg->circ_shift; rp.n_ch = c.cfg->n_channels; rp.n_snr = c.cfg->n_snr;
    rp.seed_lo = r.ck.tx.seed_lo; rp.seed_hi = r.ck.tx.seed_hi; rp.frames = g.frames; rp.frame_offset = c.cfg->frame_offset;
    rp.X = r.tx.X; rp.x = r.tx.x; rp.wrx = r.d_wr; rp.h = r.d_h; rp.nlin = r.d_nlin; rp.amask = r.tx.act;
    rp.part_pow = r.d_ppow; rp.part_cnt = r.d_pcnt; rp.errs = r.d_errs; rp.pow = r.d_pow;
    if (c.dop.on || c.dop.static_track) {
        r.ck.dp.knots = r.d_h; r.ck.dp.n_knots = r.n_knots; r.ck.dp.knot_step = r.knot_step;
    }
    r.ck.n_tracks = r.n_tracks() + 1; r.ck.max_theta = r.max_theta;
    return WOFDM_OK;
}

// the point loop's side: the receiver offsets' points and base phasors, and the per-symbol partials and totals
int stage_points(rx_run &r)
{
    wofdm_sparams &sp = r.ck.sp;
    sp.n_points = r.c.n_points; sp.cells = r.g.cells;
    if (!r.c.per_symbol) return WOFDM_OK;
    const size_t n_part = r.chunk * (size_t)r.c.n_points * r.g.S;
    const bool sync = r.c.sync.on;
    if ((sync && (!r.d_pts.alloc(r.pts.size()) || !r.d_base.alloc(r.base.size()))) || !r.d_spow.alloc(n_part) || !r.d_scnt.alloc(n_part) ||
        !r.d_serrs.alloc(2 * r.n_sym) || !r.d_stot.alloc(r.n_sym))
        return fail(WOFDM_E_NOMEM, "device allocation failed (receiver offsets or tracks)");
    if ((sync && (!r.d_pts.upload(r.pts.data(), r.pts.size()) || !r.d_base.upload(r.base.data(), r.base.size()))) ||
        hipMemset(r.d_serrs, 0, 2 * r.n_sym * 8) != hipSuccess || hipMemset(r.d_stot, 0, r.n_sym * 8) != hipSuccess)
        return fail(WOFDM_E_HIP, "upload failed");
    sp.pts = r.d_pts; sp.base = r.d_base; sp.sym_pow = r.d_spow; sp.sym_cnt = r.d_scnt; sp.sym_errs = r.d_serrs; sp.sym_tot = r.d_stot;
    return WOFDM_OK;
}

// the amplifier's side: points, saturation amplitudes, the points' waveforms and power sums of the chunk, the power totals
int stage_amp(rx_run &r)
{
    if (!r.c.amp.on) return WOFDM_OK;
    const size_t NP = (size_t)r.c.n_points;
    if (!r.d_papts.alloc(r.pa.size()) || !r.d_asat.alloc(r.asat.size()) || !r.d_y.alloc(r.chunk * NP * r.g.T) ||
        !r.d_pwr.alloc(r.chunk * NP * 2) || !r.d_ptot.alloc(r.n_ptot))
        return fail(WOFDM_E_NOMEM, "device allocation failed (amplifier)");
    if (!r.d_papts.upload(r.pa.data(), r.pa.size()) || !r.d_asat.upload(r.asat.data(), r.asat.size()) ||
        hipMemset(r.d_ptot, 0, r.n_ptot * 8) != hipSuccess)
        return fail(WOFDM_E_HIP, "upload failed");
    wofdm_paparams &pa = r.ck.pa;
    pa.n_points = (int32_t)NP; pa.pairs = (int32_t)r.g.pairs; pa.pts = r.d_papts; pa.asat = r.d_asat; pa.y = r.d_y;
    pa.pwr = r.d_pwr; pa.pwr_tot = r.d_ptot;
    return WOFDM_OK;
}

// the phase noise's side: the points and the unit walks of the chunk's items
int stage_pn(rx_run &r)
{
    if (!r.c.pn.on) return WOFDM_OK;
    if (!r.d_pnpts.alloc(r.pn.size()) || !r.d_walk.alloc(r.chunk * r.g.S * r.g.B)) return fail(WOFDM_E_NOMEM, "device allocation failed (phase noise)");
    if (!r.d_pnpts.upload(r.pn.data(), r.pn.size())) return fail(WOFDM_E_HIP, "upload failed");
    r.ck.pn.pts = r.d_pnpts; r.ck.pn.walk = r.d_walk;
    return WOFDM_OK;
}

int stage_link(rx_run &r)
{
    if (!r.c.link.on) return WOFDM_OK;
    if (!r.d_lkpts.alloc(r.lk.size())) return fail(WOFDM_E_NOMEM, "device allocation failed (link points)");
    if (!r.d_lkpts.upload(r.lk.data(), r.lk.size())) return fail(WOFDM_E_HIP, "upload failed");
    r.ck.lk.pts = r.d_lkpts;
    return WOFDM_OK;
}

// the demapper's side: the pairs' W2 = sum w_rx^2 (double, stored in single), the scales as c_j log2(e), the chunk's penalties,
// the totals
int stage_soft(rx_run &r)
{
    const auto &soft = r.c.soft;
    if (!soft.on) return WOFDM_OK;
    const rx_geom &g = r.g;
    const size_t NP = (size_t)r.c.n_points, NSC = (size_t)soft.n_scales;
    std::vector<float> hw2((size_t)g.pairs);
    for (uint64_t p = 0; p < g.pairs; ++p) {
        double acc = 0.0;
        for (int m = 0; m < g.NW; ++m) acc += (double)r.c.w_rx[p * g.NW + m] * (double)r.c.w_rx[p * g.NW + m];
        hw2[(size_t)p] = (float)acc;
    }
    if (!r.d_w2.alloc(hw2.size()) || !r.d_bpart.alloc(r.chunk * NP * (g.S - 1) * NSC * g.N) || !r.d_spart.alloc(r.chunk * NP * NSC * g.S) ||
        !r.d_btot.alloc(r.n_bpen) || !r.d_sptot.alloc(r.n_spen))
        return fail(WOFDM_E_NOMEM, "device allocation failed (soft outputs)");
    if (!r.d_w2.upload(hw2.data(), hw2.size()) || hipMemset(r.d_btot, 0, r.n_bpen * 8) != hipSuccess ||
        hipMemset(r.d_sptot, 0, r.n_spen * 8) != hipSuccess)
        return fail(WOFDM_E_HIP, "upload failed");
    wofdm_softparams &so = r.ck.soft;
    so.n_scales = soft.n_scales;
    for (int j = 0; j < soft.n_scales; ++j) so.cs[j] = (float)((double)soft.scales[j] * 1.4426950408889634074);
    so.w2 = r.d_w2; so.bit_part = r.d_bpart; so.sym_part = r.d_spart; so.bit_tot = r.d_btot; so.sym_tot = r.d_sptot;
    r.ck.soft_on = true;
    return WOFDM_OK;
}

// the tracking receiver's side: the comb and the points
int stage_track(rx_run &r)
{
    if (!r.c.trk.on) return WOFDM_OK;
    if ((!r.pil.empty() && !r.d_pil.alloc(r.pil.size())) || !r.d_tp.alloc(r.tp.size()))
        return fail(WOFDM_E_NOMEM, "device allocation failed (tracking receiver)");
    if ((!r.pil.empty() && !r.d_pil.upload(r.pil.data(), r.pil.size())) || !r.d_tp.upload(r.tp.data(), r.tp.size()))
        return fail(WOFDM_E_HIP, "upload failed");
    r.ck.tk.pilots = r.pil.empty() ? nullptr : (const uint8_t *)r.d_pil;
    r.ck.tk.pts = r.d_tp;
    r.ck.track_on = true;
    return WOFDM_OK;
}

// the coded link's side: the chunk's soft bits, the gather table, the counters
int stage_code(rx_run &r)
{
    const auto &cd = r.c.code;
    if (!cd.on) return WOFDM_OK;
    const rx_geom &g = r.g;
    // (the frame-spanning code has counters and gather tables of its own: stage_frame)
    const bool sym = !r.c.frm.on && !r.c.coset.on;
    if (!r.d_sbits.alloc(r.chunk * (size_t)r.c.n_points * (g.S - 1) * g.N * 8) || !r.d_gather.alloc(r.gather.size()) ||
        (sym && !r.d_cerrs.alloc(r.n_cerr)))
        return fail(WOFDM_E_NOMEM, "device allocation failed (coded link)");
    if (!r.d_gather.upload(r.gather.data(), r.gather.size()) || (sym && hipMemset(r.d_cerrs, 0, r.n_cerr * 8) != hipSuccess))
        return fail(WOFDM_E_HIP, "upload failed");
    wofdm_codeparams &k = r.ck.cd;
    k.llr_scale = cd.llr_scale; k.soft = r.d_sbits; k.gather = r.d_gather; k.n_c = (int32_t)r.gather.size(); k.n_codes = cd.n_codes;
    for (int i = 0; !r.c.ldpc.on && i < cd.n_codes; ++i) {
        k.rate[i] = cd.codes[i].rate;
        k.steps[i] = r.csteps[i];
    }
    k.errs = r.d_cerrs;
    r.ck.code_on = true;
    return WOFDM_OK;
}

// the frame's gather tables in use, on the device
int stage_fgather(rx_run &r, const char *what)
{
    for (int v = 0; v < 2; ++v) {
        if (r.fnc[v] == 0) continue;
        if (!r.d_fgather[v].alloc(r.fgather[v].size())) return fail(WOFDM_E_NOMEM, "device allocation failed (%s)", what);
        if (!r.d_fgather[v].upload(r.fgather[v].data(), r.fgather[v].size())) return fail(WOFDM_E_HIP, "upload failed");
    }
    return WOFDM_OK;
}

// the LDPC codes' side: the words per variant, the counters, the codes and their lifts
int stage_ldpc_codes(rx_run &r, const wofdm_ldpc_code *codes, int32_t n_codes)
{
    wofdm_ldpcparams &k = r.ck.ld;
    k = wofdm_ldpcparams{};
    for (int v = 0; v < 2; ++v) {
        if (r.fnc[v] == 0) continue;
        k.gather[v] = r.d_fgather[v];
        k.n[v] = r.ln[v];
        k.W[v] = r.lW[v];
    }
    if (!r.d_lerrs.alloc(r.n_lerr)) return fail(WOFDM_E_NOMEM, "device allocation failed (LDPC code)");
    if (hipMemset(r.d_lerrs, 0, r.n_lerr * 8) != hipSuccess) return fail(WOFDM_E_HIP, "upload failed");
    k.errs = r.d_lerrs;
    for (int i = 0; i < n_codes; ++i) {
        const wofdm_ldpc_code &q = codes[i];
        r.ck.ld_code[i][0] = q.J; r.ck.ld_code[i][1] = q.L; r.ck.ld_code[i][2] = q.max_iter;
        r.ck.ld_Z[i][0] = r.lZ[i][0]; r.ck.ld_Z[i][1] = r.lZ[i][1];
    }
    return WOFDM_OK;
}

// the Viterbi codes' side: the codeword lengths per variant, the chunk's history, the counters, the codes' steps
int stage_frame_codes(rx_run &r, int32_t n_codes)
{
    wofdm_longparams &k = r.ck.fr;
    k = wofdm_longparams{};
    for (int v = 0; v < 2; ++v) {
        if (r.fnc[v] == 0) continue;
        k.gather[v] = r.d_fgather[v];
        k.n_c[v] = r.fnc[v];
    }
    if (!r.d_hist.alloc(r.chunk * (size_t)r.c.n_points * (size_t)r.hist_blocks * 64) || !r.d_ferrs.alloc(r.n_ferr))
        return fail(WOFDM_E_NOMEM, "device allocation failed (frame code)");
    if (hipMemset(r.d_ferrs, 0, r.n_ferr * 8) != hipSuccess) return fail(WOFDM_E_HIP, "upload failed");
    k.hist = r.d_hist; k.hist_blocks = r.hist_blocks; k.errs = r.d_ferrs;
    for (int i = 0; i < n_codes; ++i)
        for (int v = 0; v < 2; ++v) r.ck.fr_steps[i][v] = r.fsteps[i][v];
    return WOFDM_OK;
}

// the frame-spanning code's side (behind stage_code), or in its place the LDPC code's
int stage_frame(rx_run &r)
{
    if (!r.c.frm.on) return WOFDM_OK;
    const bool ldpc = r.c.ldpc.on;
    int rc = stage_fgather(r, ldpc ? "LDPC code" : "frame code");
    if (rc == WOFDM_OK) rc = ldpc ? stage_ldpc_codes(r, r.c.ldpc.codes, r.c.code.n_codes) : stage_frame_codes(r, r.c.code.n_codes);
    if (rc != WOFDM_OK) return rc;
    (ldpc ? r.ck.ldpc_on : r.ck.frame_on) = true;
    return WOFDM_OK;
}

// the coset view's side (behind stage_code): both families over the same gather tables, the rates, the stream's key
int stage_coset(rx_run &r)
{
    const auto &cs = r.c.coset;
    if (!cs.on) return WOFDM_OK;
    int rc = stage_fgather(r, "coset view");
    if (rc == WOFDM_OK && cs.n_codes > 0) rc = stage_frame_codes(r, cs.n_codes);
    if (rc == WOFDM_OK && cs.n_ldpc > 0) rc = stage_ldpc_codes(r, cs.ldpc_codes, cs.n_ldpc);
    if (rc != WOFDM_OK) return rc;
    for (int i = 0; i < cs.n_codes; ++i) r.ck.cd.rate[i] = cs.codes[i].rate;
    r.ck.cs_nv = cs.n_codes; r.ck.cs_nl = cs.n_ldpc;
    r.ck.cs = {(uint32_t)r.c.cfg->seed, (uint32_t)(r.c.cfg->seed >> 32), r.c.cfg->frame_offset};
    r.ck.coset_on = true;
    if (r.c.harq) {
        r.ck.hq_rounds = cs.rounds;
        r.ck.hq_combine = cs.combine;
    }
    return WOFDM_OK;
}

// the neighbour's side of the chunk: allocation, channels, and the Tx chain of its S + 1 symbols on the victim's windows and mask
int stage_nb(rx_run &r)
{
    if (!r.nb) return WOFDM_OK;
    const rx_call &c = r.c;
    const rx_geom &g = r.g;
    geom gl{};
    gl.L = g.L;
    const std::vector<float2> hpi = pack_taps(c.cfg, gl, c.nb.h ? c.nb.h : c.h);
    const int rc = r.nbtx.stage(g, g.S + 1, r.chunk, r.nb_act, c.tx_mask != nullptr, " (neighbour)");
    if (rc != WOFDM_OK) return rc;
    if (!r.d_hi.alloc(hpi.size())) return fail(WOFDM_E_NOMEM, "device allocation failed (neighbour)");
    if (!r.d_hi.upload(hpi.data(), hpi.size())) return fail(WOFDM_E_HIP, "upload failed");
    r.ck.nb = r.nbtx.params(c.cfg, g, g.S + 1, (uint32_t)g.cpp, r.sh);
    r.ck.nb.stream = WOFDM_STREAM_ACI;
    wofdm_aparams &a = r.ck.a;
    a.xi = r.nbtx.x; a.hi = r.d_hi; a.Ti = g.T + g.B; a.ioff = g.B - c.nb.delay;
    a.a_lvl = (float)std::pow(10.0, 0.05 * (double)c.nb.level_db);
    r.ck.nb_on = true;
    return WOFDM_OK;
}

template <typename T> bool fetch(std::vector<T> &host, const T *dev)
{
    return host.empty() || hipMemcpy(host.data(), dev, host.size() * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess;
}
template <typename T, typename U> void add_to(T *out, const std::vector<U> &host)
{
    for (size_t i = 0; out && i < host.size(); ++i) out[i] += host[i];
}

// The receive profiles.  Every argument is checked before the first HIP call -- the NULL arguments and the stages' counts,
// the geometry, the finiteness, then the stages' points: sync, pn, doppler, link, amplifier, tracking --; the caller's arrays are
// written only after everything has succeeded.
int rx_profile_run(const rx_call &c)
{
    int rc = check_rx_args(c);
    if (rc != WOFDM_OK) return rc;
    rx_run r{c};
    if ((rc = check_rx_geometry(c, &r.g)) != WOFDM_OK || (rc = check_rx_finite(c, r.g)) != WOFDM_OK ||
        (rc = check_allocation(c.active, r.g.N, &r.act)) != WOFDM_OK || (rc = prep_nb(r)) != WOFDM_OK ||
        (rc = prep_sync(r)) != WOFDM_OK || (rc = prep_pn(r)) != WOFDM_OK || (rc = check_knots(r)) != WOFDM_OK ||
        (rc = prep_link(r)) != WOFDM_OK || (rc = prep_amp(r)) != WOFDM_OK || (rc = prep_track(r)) != WOFDM_OK ||
        (rc = prep_code(r)) != WOFDM_OK || (rc = prep_frame(r)) != WOFDM_OK || (rc = prep_coset(r)) != WOFDM_OK ||
        (rc = use_device(c.device)) != WOFDM_OK)
        return rc;
    g_rxprof_ms = 0.f;
    const rx_geom &g = r.g;
    const uint64_t items = g.cells * g.frames;
    if (items == 0) return WOFDM_OK;
    r.chunk = (size_t)chunk_frames(items, WOFDM_RX_PROFILE_CHUNK_BYTES, rx_job_bytes(r));
    // (retransmissions: whole groups per chunk -- the formula rounded down to a multiple of the rounds, one group at least)
    if (c.harq) r.chunk = std::max<size_t>(r.chunk / (size_t)c.coset.rounds, 1) * (size_t)c.coset.rounds;
    pack_channel(r);
    const size_t NP = (size_t)c.n_points, NSC = c.soft.on ? (size_t)c.soft.n_scales : 0;
    r.n_out = NP * g.cells * g.N;
    r.n_sym = c.per_symbol ? NP * g.cells * (g.S - 1) : 0;
    r.n_ptot = c.amp.on ? NP * g.cells * 2 : 0;
    r.n_bpen = NP * g.cells * NSC * g.N;
    r.n_spen = NP * g.cells * NSC * (g.S - 1);
    r.n_cerr = c.code.on ? NP * g.cells * (size_t)c.code.n_codes * (g.S - 1) * 2 : 0;
    r.n_ferr = c.frm.on && !c.ldpc.on ? NP * g.cells * (size_t)c.code.n_codes * 2 : 0;
    r.n_lerr = c.ldpc.on ? NP * g.cells * (size_t)c.code.n_codes * 4 : 0;
    if (c.frm.on) r.n_cerr = 0;
    if (c.coset.on) {
        r.n_ferr = NP * g.cells * (size_t)c.coset.n_codes * 2;
        r.n_lerr = NP * g.cells * (size_t)c.coset.n_ldpc * (c.harq ? WOFDM_HARQ_FIELDS : 4);
    }
    if ((rc = stage_base(r)) != WOFDM_OK || (rc = stage_points(r)) != WOFDM_OK || (rc = stage_amp(r)) != WOFDM_OK ||
        (rc = stage_pn(r)) != WOFDM_OK || (rc = stage_link(r)) != WOFDM_OK || (rc = stage_soft(r)) != WOFDM_OK ||
        (rc = stage_track(r)) != WOFDM_OK || (rc = stage_code(r)) != WOFDM_OK || (rc = stage_frame(r)) != WOFDM_OK ||
        (rc = stage_coset(r)) != WOFDM_OK || (rc = stage_nb(r)) != WOFDM_OK)
        return rc;
    // (a neighbour that loads no bin: the plain kernel)
    r.ck.arm = c.arm == RXP_ACI && !r.nb ? RXP_PLAIN : c.arm;
    std::vector<unsigned long long> herr(2 * r.n_out), hserr(2 * r.n_sym);
    std::vector<unsigned long long> hcerr(r.n_cerr), hferr(r.n_ferr), hlerr(r.n_lerr);
    std::vector<double> hpow(r.n_out), hspow(r.n_sym), hptot(r.n_ptot), hbpen(r.n_bpen), hspen(r.n_spen);
    float ms = 0.f;
    hipError_t e = hipSuccess;
    const wofdm_link_fns *ax = wofdm_aux_link(g.N);
    // (the coded link's soft bits, where the caller wants them: the items are [cell][frame], so a chunk's block is contiguous
    // in the caller's array, and its copy waits for the chunk)
    const size_t item_bytes = c.code.on ? NP * (size_t)(g.S - 1) * g.N * 8 : 0;
    rc = run_chunks(items, r.chunk, [&](uint64_t item0, int32_t n_jobs) {
        r.ck.tx.item0 = r.ck.nb.item0 = r.ck.r.item0 = item0;
        r.ck.tx.n_jobs = r.ck.nb.n_jobs = r.ck.r.n_jobs = n_jobs;
        hipError_t le = ax ? ax->rx_profile_chunk(&r.ck, nullptr) : hipErrorInvalidValue;
        if (le == hipSuccess && c.code.on && c.code.soft_bits)
            le = hipMemcpy(c.code.soft_bits + item0 * item_bytes, r.d_sbits.p, (size_t)n_jobs * item_bytes, hipMemcpyDeviceToHost);
        return le;
    }, &e, &ms);
    if (rc != WOFDM_OK) return rc;
    if (e != hipSuccess || !fetch(herr, r.d_errs.p) || !fetch(hpow, r.d_pow.p) || !fetch(hserr, r.d_serrs.p) || !fetch(hspow, r.d_stot.p) ||
        !fetch(hptot, r.d_ptot.p) || !fetch(hbpen, r.d_btot.p) || !fetch(hspen, r.d_sptot.p) || !fetch(hcerr, r.d_cerrs.p) || !fetch(hferr, r.d_ferrs.p) ||
        !fetch(hlerr, r.d_lerrs.p))
        return fail(WOFDM_E_HIP, "receive-profile kernels or copy-back failed: %s",
                    hipGetErrorString(e != hipSuccess ? e : hipGetLastError()));
    add_to(c.errs, herr);
    add_to(c.err_power, hpow);
    add_to(c.sym_errs, hserr);
    add_to(c.sym_power, hspow);
    add_to(c.amp.pa_power, hptot);
    add_to(c.soft.bit_penalty, hbpen);
    add_to(c.soft.sym_penalty, hspen);
    add_to(c.code.code_errs, hcerr);
    add_to(c.frm.frame_errs, hferr);
    add_to(c.ldpc.ldpc_errs, hlerr);
    if (c.coset.on) {
        add_to(c.coset.frame_errs, hferr);
        add_to(c.coset.ldpc_errs, hlerr);
    }
    g_rxprof_ms = ms;
    return WOFDM_OK;
}

// what every call has; the arm and the stages are the entry point's to add
rx_call rx_base(const wofdm_cfg *cfg, int device, const float *w_tx, const float *w_rx, const float *h, const float *snr_db,
                const uint8_t *active, const float *tx_mask)
{
    rx_call c{};
    c.cfg = cfg; c.device = device; c.w_tx = w_tx; c.w_rx = w_rx; c.h = h; c.snr_db = snr_db; c.active = active; c.tx_mask = tx_mask;
    c.arm = RXP_PLAIN; c.n_points = 1;
    return c;
}
// an arm with a point loop: its points, and the outputs every call and every such arm has
void rx_outputs(rx_call &c, int32_t arm, int32_t n_points, uint64_t *errs, double *err_power, uint64_t *sym_errs = nullptr,
                double *sym_power = nullptr)
{
    c.arm = arm; c.n_points = n_points; c.per_symbol = arm != RXP_PLAIN && arm != RXP_ACI;
    c.errs = errs; c.err_power = err_power; c.sym_errs = sym_errs; c.sym_power = sym_power;
}

// wofdm_rx_profile_link and wofdm_rx_profile_soft: the points switch the five stages, each of which takes what a point says to
// it in its own arm's form, so that its own arm's code checks and prepares it
int rx_link_stages(rx_call &c, int32_t n_points, const wofdm_link_point *points)
{
    if (!points) return fail(WOFDM_E_INVALID, "NULL argument (points)");
    if (n_points < 1) return fail(WOFDM_E_INVALID, "n_points=%d must be >= 1", n_points);
    if (n_points > WOFDM_LINK_MAX_POINTS) return fail(WOFDM_E_UNSUPPORTED, "n_points=%d exceeds %d", n_points, WOFDM_LINK_MAX_POINTS);
    bool any_track = false, any_nb = false;
    for (int i = 0; i < n_points; ++i) {
        const wofdm_link_point &q = points[i];
        c.link.as_sync.push_back({q.timing, q.cfo, q.cfo_tracked, 0});
        c.link.as_pn.push_back({q.linewidth, q.cpe_tracked, {0, 0}});
        c.link.as_pa.push_back({q.pa_model, q.pa_ibo_db, q.pa_smooth, 0});
        any_track |= q.track >= 0;
        any_nb |= q.aci_on != 0;
    }
    if (any_track && !c.dop.h_track) return fail(WOFDM_E_INVALID, "NULL argument (h_track, and a point names a track)");
    if (any_nb && !c.nb.active) return fail(WOFDM_E_INVALID, "NULL argument (aci_active, and a point has aci_on)");
    c.link.on = true; c.link.points = points;
    c.sync.on = c.amp.on = c.pn.on = true;
    c.sync.points = c.link.as_sync.data(); c.pn.points = c.link.as_pn.data(); c.amp.points = c.link.as_pa.data();
    // (the tracks and the neighbour are on where a point wants them; the static channel is behind the tracks either way, and
    // a linear point needs no reference power)
    c.dop.on = any_track; c.dop.static_track = true; c.nb.on = any_nb; c.amp.ref_optional = true;
    return WOFDM_OK;
}

}  // namespace

extern "C" {

int wofdm_rx_profile(const wofdm_cfg *cfg, int device, const float *w_tx, const float *w_rx, const float *h,
                     const float *snr_db, const uint8_t *active, const float *tx_mask, uint64_t *errs, double *err_power)
{
    rx_call c = rx_base(cfg, device, w_tx, w_rx, h, snr_db, active, tx_mask);
    rx_outputs(c, RXP_PLAIN, 1, errs, err_power);
    return rx_profile_run(c);
}

int wofdm_rx_profile_aci(const wofdm_cfg *cfg, int device, const float *w_tx, const float *w_rx, const float *h,
                         const float *snr_db, const uint8_t *active, const float *tx_mask, const uint8_t *aci_active,
                         const float *aci_h, int32_t aci_delay, float aci_level_db, uint64_t *errs, double *err_power)
{
    rx_call c = rx_base(cfg, device, w_tx, w_rx, h, snr_db, active, tx_mask);
    rx_outputs(c, RXP_ACI, 1, errs, err_power);
    c.nb = {true, aci_active, aci_h, aci_delay, aci_level_db};
    return rx_profile_run(c);
}

int wofdm_rx_profile_sync(const wofdm_cfg *cfg, int device, const float *w_tx, const float *w_rx, const float *h,
                          const float *snr_db, const uint8_t *active, const float *tx_mask, int32_t n_points,
                          const wofdm_sync_point *points, uint64_t *errs, double *err_power, uint64_t *sym_errs, double *sym_power)
{
    rx_call c = rx_base(cfg, device, w_tx, w_rx, h, snr_db, active, tx_mask);
    rx_outputs(c, RXP_SYNC, n_points, errs, err_power, sym_errs, sym_power);
    c.sync = {true, points};
    return rx_profile_run(c);
}

int wofdm_rx_profile_doppler(const wofdm_cfg *cfg, int device, const float *w_tx, const float *w_rx, const float *h_track,
                             int32_t n_tracks, int32_t n_knots, int32_t knot_step, const float *snr_db, const uint8_t *active,
                             const float *tx_mask, uint64_t *errs, double *err_power, uint64_t *sym_errs, double *sym_power)
{
    rx_call c = rx_base(cfg, device, w_tx, w_rx, nullptr, snr_db, active, tx_mask);
    rx_outputs(c, RXP_DOPPLER, n_tracks, errs, err_power, sym_errs, sym_power);
    c.dop = {true, false, h_track, n_tracks, n_knots, knot_step};
    return rx_profile_run(c);
}

int wofdm_rx_profile_pa(const wofdm_cfg *cfg, int device, const float *w_tx, const float *w_rx, const float *h, const float *snr_db,
                        const uint8_t *active, const float *tx_mask, int32_t n_points, const wofdm_pa_point *points,
                        const float *ref_power, uint64_t *errs, double *err_power, uint64_t *sym_errs, double *sym_power,
                        double *pa_power)
{
    rx_call c = rx_base(cfg, device, w_tx, w_rx, h, snr_db, active, tx_mask);
    rx_outputs(c, RXP_PA, n_points, errs, err_power, sym_errs, sym_power);
    c.amp = {true, false, points, ref_power, pa_power};
    return rx_profile_run(c);
}

int wofdm_rx_profile_pn(const wofdm_cfg *cfg, int device, const float *w_tx, const float *w_rx, const float *h, const float *snr_db,
                        const uint8_t *active, const float *tx_mask, int32_t n_points, const wofdm_pn_point *points, uint64_t *errs,
                        double *err_power, uint64_t *sym_errs, double *sym_power)
{
    rx_call c = rx_base(cfg, device, w_tx, w_rx, h, snr_db, active, tx_mask);
    rx_outputs(c, RXP_PN, n_points, errs, err_power, sym_errs, sym_power);
    c.pn = {true, points};
    return rx_profile_run(c);
}

int wofdm_rx_profile_link(const wofdm_cfg *cfg, int device, const float *w_tx, const float *w_rx, const float *h, const float *snr_db,
                          const uint8_t *active, const float *tx_mask, const float *h_track, int32_t n_tracks, int32_t n_knots,
                          int32_t knot_step, const uint8_t *aci_active, const float *aci_h, const float *ref_power, int32_t n_points,
                          const wofdm_link_point *points, uint64_t *errs, double *err_power, uint64_t *sym_errs, double *sym_power,
                          double *pa_power)
{
    rx_call c = rx_base(cfg, device, w_tx, w_rx, h, snr_db, active, tx_mask);
    rx_outputs(c, RXP_LINK, n_points, errs, err_power, sym_errs, sym_power);
    c.dop = {false, false, h_track, n_tracks, n_knots, knot_step};
    c.nb = {false, aci_active, aci_h, 0, 0.f};
    c.amp = {false, false, nullptr, ref_power, pa_power};
    const int rc = rx_link_stages(c, n_points, points);
    return rc != WOFDM_OK ? rc : rx_profile_run(c);
}

int wofdm_rx_profile_soft(const wofdm_cfg *cfg, int device, const float *w_tx, const float *w_rx, const float *h, const float *snr_db,
                          const uint8_t *active, const float *tx_mask, const float *h_track, int32_t n_tracks, int32_t n_knots,
                          int32_t knot_step, const uint8_t *aci_active, const float *aci_h, const float *ref_power, int32_t n_points,
                          const wofdm_link_point *points, int32_t n_scales, const float *scales, uint64_t *errs, double *err_power,
                          uint64_t *sym_errs, double *sym_power, double *pa_power, double *bit_penalty, double *sym_penalty)
{
    if (!scales || !bit_penalty) return fail(WOFDM_E_INVALID, "NULL argument (scales or bit_penalty)");
    if (n_scales < 1) return fail(WOFDM_E_INVALID, "n_scales=%d must be >= 1", n_scales);
    if (n_scales > WOFDM_SOFT_MAX_SCALES) return fail(WOFDM_E_UNSUPPORTED, "n_scales=%d exceeds %d", n_scales, WOFDM_SOFT_MAX_SCALES);
    for (int j = 0; j < n_scales; ++j)
        if (!std::isfinite(scales[j]) || !(scales[j] > 0.f))
            return fail(WOFDM_E_INVALID, "scales[%d] must be finite and positive", j);
    rx_call c = rx_base(cfg, device, w_tx, w_rx, h, snr_db, active, tx_mask);
    rx_outputs(c, RXP_LINK, n_points, errs, err_power, sym_errs, sym_power);
    c.dop = {false, false, h_track, n_tracks, n_knots, knot_step};
    c.nb = {false, aci_active, aci_h, 0, 0.f};
    c.amp = {false, false, nullptr, ref_power, pa_power};
    c.soft = {true, n_scales, scales, bit_penalty, sym_penalty};
    const int rc = rx_link_stages(c, n_points, points);
    return rc != WOFDM_OK ? rc : rx_profile_run(c);
}

// wofdm_rx_profile_tracking and, with the coded link behind it (code, or null), wofdm_rx_profile_coded: one call, filled once
static int rx_tracking_call(const wofdm_cfg *cfg, int device, const float *w_tx, const float *w_rx, const float *h, const float *snr_db,
                            const uint8_t *active, const float *tx_mask, const float *h_track, int32_t n_tracks, int32_t n_knots,
                            int32_t knot_step, const uint8_t *aci_active, const float *aci_h, const float *ref_power, int32_t n_points,
                            const wofdm_link_point *points, int32_t n_scales, const float *scales, const uint8_t *pilots,
                            const wofdm_tracking_point *tracking, uint64_t *errs, double *err_power, uint64_t *sym_errs,
                            double *sym_power, double *pa_power, double *bit_penalty, double *sym_penalty,
                            const decltype(rx_call::code) *code, const decltype(rx_call::frm) *frm = nullptr,
                            const decltype(rx_call::ldpc) *ldpc = nullptr, const decltype(rx_call::coset) *coset = nullptr,
                            bool harq = false)
{
    if (!scales || !bit_penalty || !tracking) return fail(WOFDM_E_INVALID, "NULL argument (scales, bit_penalty or tracking)");
    if (n_scales < 1) return fail(WOFDM_E_INVALID, "n_scales=%d must be >= 1", n_scales);
    if (n_scales > WOFDM_SOFT_MAX_SCALES) return fail(WOFDM_E_UNSUPPORTED, "n_scales=%d exceeds %d", n_scales, WOFDM_SOFT_MAX_SCALES);
    for (int j = 0; j < n_scales; ++j)
        if (!std::isfinite(scales[j]) || !(scales[j] > 0.f))
            return fail(WOFDM_E_INVALID, "scales[%d] must be finite and positive", j);
    rx_call c = rx_base(cfg, device, w_tx, w_rx, h, snr_db, active, tx_mask);
    rx_outputs(c, RXP_LINK, n_points, errs, err_power, sym_errs, sym_power);
    c.dop = {false, false, h_track, n_tracks, n_knots, knot_step};
    c.nb = {false, aci_active, aci_h, 0, 0.f};
    c.amp = {false, false, nullptr, ref_power, pa_power};
    c.soft = {true, n_scales, scales, bit_penalty, sym_penalty};
    c.trk = {true, pilots, tracking};
    if (code) c.code = *code;
    if (frm) c.frm = *frm;
    if (ldpc) c.ldpc = *ldpc;
    if (coset) c.coset = *coset;
    c.harq = harq;
    const int rc = rx_link_stages(c, n_points, points);
    return rc != WOFDM_OK ? rc : rx_profile_run(c);
}

int wofdm_rx_profile_tracking(const wofdm_cfg *cfg, int device, const float *w_tx, const float *w_rx, const float *h, const float *snr_db,
                              const uint8_t *active, const float *tx_mask, const float *h_track, int32_t n_tracks, int32_t n_knots,
                              int32_t knot_step, const uint8_t *aci_active, const float *aci_h, const float *ref_power, int32_t n_points,
                              const wofdm_link_point *points, int32_t n_scales, const float *scales, const uint8_t *pilots,
                              const wofdm_tracking_point *tracking, uint64_t *errs, double *err_power, uint64_t *sym_errs,
                              double *sym_power, double *pa_power, double *bit_penalty, double *sym_penalty)
{
    return rx_tracking_call(cfg, device, w_tx, w_rx, h, snr_db, active, tx_mask, h_track, n_tracks, n_knots, knot_step, aci_active, aci_h,
                            ref_power, n_points, points, n_scales, scales, pilots, tracking, errs, err_power, sym_errs, sym_power,
                            pa_power, bit_penalty, sym_penalty, nullptr);
}

int wofdm_rx_profile_coded(const wofdm_cfg *cfg, int device, const float *w_tx, const float *w_rx, const float *h, const float *snr_db,
                           const uint8_t *active, const float *tx_mask, const float *h_track, int32_t n_tracks, int32_t n_knots,
                           int32_t knot_step, const uint8_t *aci_active, const float *aci_h, const float *ref_power, int32_t n_points,
                           const wofdm_link_point *points, int32_t n_scales, const float *scales, const uint8_t *pilots,
                           const wofdm_tracking_point *tracking, float llr_scale, const int32_t *perm, int32_t n_codes,
                           const wofdm_code *codes, uint64_t *errs, double *err_power, uint64_t *sym_errs, double *sym_power,
                           double *pa_power, double *bit_penalty, double *sym_penalty, uint64_t *code_errs, int8_t *soft_bits)
{
    const decltype(rx_call::code) code = {true, llr_scale, perm, n_codes, codes, code_errs, soft_bits};
    return rx_tracking_call(cfg, device, w_tx, w_rx, h, snr_db, active, tx_mask, h_track, n_tracks, n_knots, knot_step, aci_active, aci_h,
                            ref_power, n_points, points, n_scales, scales, pilots, tracking, errs, err_power, sym_errs, sym_power,
                            pa_power, bit_penalty, sym_penalty, &code);
}

int wofdm_rx_profile_coded_frame(const wofdm_cfg *cfg, int device, const float *w_tx, const float *w_rx, const float *h,
                                 const float *snr_db, const uint8_t *active, const float *tx_mask, const float *h_track, int32_t n_tracks,
                                 int32_t n_knots, int32_t knot_step, const uint8_t *aci_active, const float *aci_h, const float *ref_power,
                                 int32_t n_points, const wofdm_link_point *points, int32_t n_scales, const float *scales,
                                 const uint8_t *pilots, const wofdm_tracking_point *tracking, float llr_scale, const int32_t *perm,
                                 int32_t n_codes, const wofdm_code *codes, int32_t sym_rot, uint64_t *errs, double *err_power,
                                 uint64_t *sym_errs, double *sym_power, double *pa_power, double *bit_penalty, double *sym_penalty,
                                 uint64_t *frame_errs, int8_t *soft_bits)
{
    const decltype(rx_call::code) code = {true, llr_scale, perm, n_codes, codes, nullptr, soft_bits};
    const decltype(rx_call::frm) frm = {true, sym_rot, frame_errs};
    return rx_tracking_call(cfg, device, w_tx, w_rx, h, snr_db, active, tx_mask, h_track, n_tracks, n_knots, knot_step, aci_active, aci_h,
                            ref_power, n_points, points, n_scales, scales, pilots, tracking, errs, err_power, sym_errs, sym_power,
                            pa_power, bit_penalty, sym_penalty, &code, &frm);
}

int wofdm_rx_profile_ldpc(const wofdm_cfg *cfg, int device, const float *w_tx, const float *w_rx, const float *h, const float *snr_db,
                          const uint8_t *active, const float *tx_mask, const float *h_track, int32_t n_tracks, int32_t n_knots,
                          int32_t knot_step, const uint8_t *aci_active, const float *aci_h, const float *ref_power, int32_t n_points,
                          const wofdm_link_point *points, int32_t n_scales, const float *scales, const uint8_t *pilots,
                          const wofdm_tracking_point *tracking, float llr_scale, const int32_t *perm, int32_t n_codes,
                          const wofdm_ldpc_code *codes, int32_t sym_rot, uint64_t *errs, double *err_power, uint64_t *sym_errs,
                          double *sym_power, double *pa_power, double *bit_penalty, double *sym_penalty, uint64_t *ldpc_errs,
                          int8_t *soft_bits)
{
    const decltype(rx_call::code) code = {true, llr_scale, perm, n_codes, nullptr, nullptr, soft_bits};
    const decltype(rx_call::frm) frm = {true, sym_rot, nullptr};
    const decltype(rx_call::ldpc) ldpc = {true, codes, ldpc_errs};
    return rx_tracking_call(cfg, device, w_tx, w_rx, h, snr_db, active, tx_mask, h_track, n_tracks, n_knots, knot_step, aci_active, aci_h,
                            ref_power, n_points, points, n_scales, scales, pilots, tracking, errs, err_power, sym_errs, sym_power,
                            pa_power, bit_penalty, sym_penalty, &code, &frm, &ldpc);
}

int wofdm_rx_profile_coset(const wofdm_cfg *cfg, int device, const float *w_tx, const float *w_rx, const float *h, const float *snr_db,
                           const uint8_t *active, const float *tx_mask, const float *h_track, int32_t n_tracks, int32_t n_knots,
                           int32_t knot_step, const uint8_t *aci_active, const float *aci_h, const float *ref_power, int32_t n_points,
                           const wofdm_link_point *points, int32_t n_scales, const float *scales, const uint8_t *pilots,
                           const wofdm_tracking_point *tracking, float llr_scale, const int32_t *perm, int32_t n_codes,
                           const wofdm_code *codes, int32_t n_ldpc, const wofdm_ldpc_code *ldpc_codes, int32_t sym_rot, uint64_t *errs,
                           double *err_power, uint64_t *sym_errs, double *sym_power, double *pa_power, double *bit_penalty,
                           double *sym_penalty, uint64_t *frame_errs, uint64_t *ldpc_errs, int8_t *soft_bits)
{
    const decltype(rx_call::code) code = {true, llr_scale, perm, 0, nullptr, nullptr, soft_bits};
    const decltype(rx_call::coset) coset = {true, n_codes, codes, n_ldpc, ldpc_codes, sym_rot, frame_errs, ldpc_errs, 0, 0};
    return rx_tracking_call(cfg, device, w_tx, w_rx, h, snr_db, active, tx_mask, h_track, n_tracks, n_knots, knot_step, aci_active, aci_h,
                            ref_power, n_points, points, n_scales, scales, pilots, tracking, errs, err_power, sym_errs, sym_power,
                            pa_power, bit_penalty, sym_penalty, &code, nullptr, nullptr, &coset);
}

int wofdm_rx_profile_harq(const wofdm_cfg *cfg, int device, const float *w_tx, const float *w_rx, const float *h, const float *snr_db,
                          const uint8_t *active, const float *tx_mask, const float *h_track, int32_t n_tracks, int32_t n_knots,
                          int32_t knot_step, const uint8_t *aci_active, const float *aci_h, const float *ref_power, int32_t n_points,
                          const wofdm_link_point *points, int32_t n_scales, const float *scales, const uint8_t *pilots,
                          const wofdm_tracking_point *tracking, float llr_scale, const int32_t *perm, int32_t n_ldpc,
                          const wofdm_ldpc_code *ldpc_codes, int32_t sym_rot, int32_t rounds, int32_t combine, uint64_t *errs,
                          double *err_power, uint64_t *sym_errs, double *sym_power, double *pa_power, double *bit_penalty,
                          double *sym_penalty, uint64_t *harq_errs, int8_t *soft_bits)
{
    const decltype(rx_call::code) code = {true, llr_scale, perm, 0, nullptr, nullptr, soft_bits};
    const decltype(rx_call::coset) coset = {true, 0, nullptr, n_ldpc, ldpc_codes, sym_rot, nullptr, harq_errs, rounds, combine};
    return rx_tracking_call(cfg, device, w_tx, w_rx, h, snr_db, active, tx_mask, h_track, n_tracks, n_knots, knot_step, aci_active, aci_h,
                            ref_power, n_points, points, n_scales, scales, pilots, tracking, errs, err_power, sym_errs, sym_power,
                            pa_power, bit_penalty, sym_penalty, &code, nullptr, nullptr, &coset, true);
}

int wofdm_ldpc_lift(int32_t J, int32_t L, int32_t n)
{
    if (!ldpc_ranges_ok(J, L)) return fail(WOFDM_E_INVALID, "J=%d must be 3 ... 6 and L=%d in J + 1 ... 24", J, L);
    if (n < 1 || n > (1 << 24)) return fail(WOFDM_E_INVALID, "n=%d must be 1 ... 2^24", n);
    const int32_t Z = ldpc_lift(J, L, n);
    if ((int64_t)(L - J) * Z - ((int64_t)L * Z - n) < 1)
        return fail(WOFDM_E_INVALID, "(%d, %d) over %d positions has no information bit", J, L, n);
    return Z;
}

int wofdm_code_steps(int32_t rate, int32_t n_c)
{
    if (rate < 0 || rate > 2 || n_c < 0) return fail(WOFDM_E_INVALID, "rate=%d must be 0, 1 or 2 and n_c=%d >= 0", rate, n_c);
    return code_steps(rate, n_c);
}

int wofdm_viterbi_decode(int device, int32_t rate, int32_t n_c, const int32_t *perm, int32_t n_cw, const int8_t *soft, uint8_t *bits,
                         int32_t *metric)
{
    if (!soft || !bits) return fail(WOFDM_E_INVALID, "NULL argument (soft or bits)");
    if (rate < 0 || rate > 2) return fail(WOFDM_E_INVALID, "rate=%d must be 0, 1 or 2", rate);
    if (n_c < 1 || n_cw < 1) return fail(WOFDM_E_INVALID, "n_c=%d and n_cw=%d must be >= 1", n_c, n_cw);
    const int32_t T = code_steps(rate, n_c);
    if (T < 7) return fail(WOFDM_E_INVALID, "n_c=%d gives %d steps, at least 7 are needed", n_c, T);
    if (T > WOFDM_CODE_MAX_STEPS) return fail(WOFDM_E_UNSUPPORTED, "n_c=%d gives %d steps, more than %d", n_c, T, WOFDM_CODE_MAX_STEPS);
    if (perm && !is_permutation(perm, n_c)) return fail(WOFDM_E_INVALID, "perm is not a permutation of 0 ... %d", n_c - 1);
    int rc = use_device(device);
    if (rc != WOFDM_OK) return rc;
    std::vector<int32_t> gather((size_t)n_c);
    for (int32_t c = 0; c < n_c; ++c) gather[(size_t)c] = perm ? perm[c] : c;
    const size_t n_soft = (size_t)n_cw * (size_t)n_c, n_bits = (size_t)n_cw * (size_t)T;
    dev_buf<int8_t> d_soft;
    dev_buf<int32_t> d_gather, d_metric;
    dev_buf<uint8_t> d_bits;
    if (!d_soft.alloc(n_soft) || !d_gather.alloc(gather.size()) || !d_bits.alloc(n_bits) || !d_metric.alloc((size_t)n_cw))
        return fail(WOFDM_E_NOMEM, "device allocation failed (decoder)");
    if (!d_soft.upload(soft, n_soft) || !d_gather.upload(gather.data(), gather.size())) return fail(WOFDM_E_HIP, "upload failed");
    wofdm_codeparams cd{};
    cd.soft = d_soft; cd.gather = d_gather; cd.n_c = n_c; cd.n_codes = 1; cd.rate[0] = rate; cd.steps[0] = T; cd.cw_stride = n_c;
    cd.bits = d_bits; cd.metric = d_metric; cd.n_cw = (uint32_t)n_cw;
    std::vector<uint8_t> hbits(n_bits);
    std::vector<int32_t> hmetric((size_t)n_cw);
    hipError_t e;
    {
        std::lock_guard<std::mutex> gate(g_gate_mu);
        e = wofdm_viterbi_launch(&cd, nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    if (e != hipSuccess || !fetch(hbits, d_bits.p) || !fetch(hmetric, d_metric.p))
        return fail(WOFDM_E_HIP, "decoder kernel or copy-back failed: %s", hipGetErrorString(e != hipSuccess ? e : hipGetLastError()));
    std::memcpy(bits, hbits.data(), n_bits);
    if (metric) std::memcpy(metric, hmetric.data(), hmetric.size() * sizeof(int32_t));
    return WOFDM_OK;
}

int wofdm_viterbi_decode_long(int device, int32_t rate, int32_t n_c, const int32_t *perm, int32_t n_cw, const int8_t *soft, uint8_t *bits,
                              int32_t *metric)
{
    if (!soft || !bits) return fail(WOFDM_E_INVALID, "NULL argument (soft or bits)");
    if (rate < 0 || rate > 2) return fail(WOFDM_E_INVALID, "rate=%d must be 0, 1 or 2", rate);
    if (n_c < 1 || n_cw < 1) return fail(WOFDM_E_INVALID, "n_c=%d and n_cw=%d must be >= 1", n_c, n_cw);
    const int32_t T = code_steps(rate, n_c);
    if (T < 7) return fail(WOFDM_E_INVALID, "n_c=%d gives %d steps, at least 7 are needed", n_c, T);
    if (T > WOFDM_CODE_LONG_MAX_STEPS)
        return fail(WOFDM_E_UNSUPPORTED, "n_c=%d gives %d steps, more than %d", n_c, T, WOFDM_CODE_LONG_MAX_STEPS);
    if (perm && !is_permutation(perm, n_c)) return fail(WOFDM_E_INVALID, "perm is not a permutation of 0 ... %d", n_c - 1);
    int rc = use_device(device);
    if (rc != WOFDM_OK) return rc;
    std::vector<int32_t> gather((size_t)n_c);
    for (int32_t c = 0; c < n_c; ++c) gather[(size_t)c] = perm ? perm[c] : c;
    // the codewords in groups whose history stays within the receive profiles' chunk budget (one codeword: at most 8 MiB)
    const int32_t blocks = hist_blocks_of(T);
    const size_t group = (size_t)std::min<uint64_t>((uint64_t)n_cw, std::max<uint64_t>(1, WOFDM_RX_PROFILE_CHUNK_BYTES / (512ull * (uint64_t)blocks)));
    const size_t n_soft = (size_t)n_cw * (size_t)n_c, n_bits = (size_t)n_cw * (size_t)T;
    dev_buf<int8_t> d_soft;
    dev_buf<int32_t> d_gather, d_metric;
    dev_buf<uint8_t> d_bits;
    dev_buf<unsigned long long> d_hist;
    if (!d_soft.alloc(n_soft) || !d_gather.alloc(gather.size()) || !d_bits.alloc(n_bits) || !d_metric.alloc((size_t)n_cw) ||
        !d_hist.alloc(group * (size_t)blocks * 64))
        return fail(WOFDM_E_NOMEM, "device allocation failed (decoder)");
    if (!d_soft.upload(soft, n_soft) || !d_gather.upload(gather.data(), gather.size())) return fail(WOFDM_E_HIP, "upload failed");
    wofdm_longparams lp{};
    lp.hist = d_hist; lp.gather[0] = d_gather; lp.n_c[0] = n_c; lp.steps[0] = T; lp.rate = rate; lp.hist_blocks = blocks;
    lp.cw_stride = n_c;
    std::vector<uint8_t> hbits(n_bits);
    std::vector<int32_t> hmetric((size_t)n_cw);
    hipError_t e = hipSuccess;
    {
        std::lock_guard<std::mutex> gate(g_gate_mu);
        for (size_t w0 = 0; e == hipSuccess && w0 < (size_t)n_cw; w0 += group) {
            lp.soft = d_soft.p + w0 * (size_t)n_c; lp.bits = d_bits.p + w0 * (size_t)T; lp.metric = d_metric.p + w0;
            lp.n_cw = (uint32_t)std::min(group, (size_t)n_cw - w0);
            e = wofdm_viterbi_long_launch(&lp, nullptr);
        }
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    if (e != hipSuccess || !fetch(hbits, d_bits.p) || !fetch(hmetric, d_metric.p))
        return fail(WOFDM_E_HIP, "decoder kernel or copy-back failed: %s", hipGetErrorString(e != hipSuccess ? e : hipGetLastError()));
    std::memcpy(bits, hbits.data(), n_bits);
    if (metric) std::memcpy(metric, hmetric.data(), hmetric.size() * sizeof(int32_t));
    return WOFDM_OK;
}

int wofdm_ldpc_decode(int device, int32_t J, int32_t L, int32_t max_iter, int32_t n, const int32_t *perm, int32_t n_cw, const int8_t *soft,
                      uint8_t *bits, int32_t *iters, uint8_t *converged)
{
    if (!soft || !bits) return fail(WOFDM_E_INVALID, "NULL argument (soft or bits)");
    if (!ldpc_ranges_ok(J, L)) return fail(WOFDM_E_INVALID, "J=%d must be 3 ... 6 and L=%d in J + 1 ... 24", J, L);
    if (max_iter < 1 || max_iter > 64) return fail(WOFDM_E_INVALID, "max_iter=%d must be 1 ... 64", max_iter);
    if (n < 1 || n_cw < 1) return fail(WOFDM_E_INVALID, "n=%d and n_cw=%d must be >= 1", n, n_cw);
    if (n > WOFDM_LDPC_MAX_BITS) return fail(WOFDM_E_UNSUPPORTED, "n=%d exceeds %d", n, WOFDM_LDPC_MAX_BITS);
    const int32_t Z = ldpc_lift(J, L, n);
    if ((int64_t)(L - J) * Z - ((int64_t)L * Z - n) < 1)
        return fail(WOFDM_E_INVALID, "(%d, %d) over %d positions has no information bit", J, L, n);
    if (wofdm_ldpc_lds(J, L, Z) > WOFDM_LDPC_LDS_MAX) return fail(WOFDM_E_UNSUPPORTED, "the decoder's LDS exceeds %d bytes", WOFDM_LDPC_LDS_MAX);
    if (perm && !is_permutation(perm, n)) return fail(WOFDM_E_INVALID, "perm is not a permutation of 0 ... %d", n - 1);
    int rc = use_device(device);
    if (rc != WOFDM_OK) return rc;
    std::vector<int32_t> gather((size_t)n);
    for (int32_t c = 0; c < n; ++c) gather[(size_t)c] = perm ? perm[c] : c;
    const size_t n_soft = (size_t)n_cw * (size_t)n;
    dev_buf<int8_t> d_soft;
    dev_buf<int32_t> d_gather, d_iters;
    dev_buf<uint8_t> d_bits, d_conv;
    if (!d_soft.alloc(n_soft) || !d_gather.alloc(gather.size()) || !d_bits.alloc(n_soft) || !d_iters.alloc((size_t)n_cw) ||
        !d_conv.alloc((size_t)n_cw))
        return fail(WOFDM_E_NOMEM, "device allocation failed (decoder)");
    if (!d_soft.upload(soft, n_soft) || !d_gather.upload(gather.data(), gather.size())) return fail(WOFDM_E_HIP, "upload failed");
    wofdm_ldpcparams lp{};
    lp.soft = d_soft; lp.gather[0] = d_gather; lp.n[0] = n; lp.W[0] = 1; lp.Z[0] = Z; lp.J = J; lp.L = L; lp.max_iter = max_iter;
    lp.cw_stride = n; lp.n_cw = (uint32_t)n_cw; lp.bits = d_bits; lp.iters = d_iters; lp.conv = d_conv;
    std::vector<uint8_t> hbits(n_soft), hconv((size_t)n_cw);
    std::vector<int32_t> hiters((size_t)n_cw);
    hipError_t e = hipSuccess;
    {
        std::lock_guard<std::mutex> gate(g_gate_mu);
        e = wofdm_ldpc_launch(&lp, nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    if (e != hipSuccess || !fetch(hbits, d_bits.p) || !fetch(hiters, d_iters.p) || !fetch(hconv, d_conv.p))
        return fail(WOFDM_E_HIP, "decoder kernel or copy-back failed: %s", hipGetErrorString(e != hipSuccess ? e : hipGetLastError()));
    std::memcpy(bits, hbits.data(), n_soft);
    if (iters) std::memcpy(iters, hiters.data(), hiters.size() * sizeof(int32_t));
    if (converged) std::memcpy(converged, hconv.data(), hconv.size());
    return WOFDM_OK;
}

int wofdm_ldpc_harq_decode(int device, int32_t J, int32_t L, int32_t max_iter, int32_t n, const int32_t *perm, int32_t n_cw, int32_t rounds,
                           int32_t combine, const int8_t *soft, uint8_t *bits, int32_t *round, int32_t *iters, uint8_t *converged)
{
    if (!soft || !bits) return fail(WOFDM_E_INVALID, "NULL argument (soft or bits)");
    if (!ldpc_ranges_ok(J, L)) return fail(WOFDM_E_INVALID, "J=%d must be 3 ... 6 and L=%d in J + 1 ... 24", J, L);
    if (max_iter < 1 || max_iter > 64) return fail(WOFDM_E_INVALID, "max_iter=%d must be 1 ... 64", max_iter);
    if (rounds < 1 || rounds > WOFDM_HARQ_MAX_ROUNDS) return fail(WOFDM_E_INVALID, "rounds=%d must be 1 ... %d", rounds, WOFDM_HARQ_MAX_ROUNDS);
    if (combine != 0 && combine != 1) return fail(WOFDM_E_INVALID, "combine=%d must be 0 or 1", combine);
    if (n < 1 || n_cw < 1) return fail(WOFDM_E_INVALID, "n=%d and n_cw=%d must be >= 1", n, n_cw);
    if (n > WOFDM_LDPC_MAX_BITS) return fail(WOFDM_E_UNSUPPORTED, "n=%d exceeds %d", n, WOFDM_LDPC_MAX_BITS);
    const int32_t Z = ldpc_lift(J, L, n);
    if ((int64_t)(L - J) * Z - ((int64_t)L * Z - n) < 1)
        return fail(WOFDM_E_INVALID, "(%d, %d) over %d positions has no information bit", J, L, n);
    if (wofdm_ldpc_coset_lds(J, L, Z) > WOFDM_LDPC_LDS_MAX)
        return fail(WOFDM_E_UNSUPPORTED, "the decoder's LDS exceeds %d bytes", WOFDM_LDPC_LDS_MAX);
    if (perm && !is_permutation(perm, n)) return fail(WOFDM_E_INVALID, "perm is not a permutation of 0 ... %d", n - 1);
    int rc = use_device(device);
    if (rc != WOFDM_OK) return rc;
    std::vector<int32_t> gather((size_t)n);
    for (int32_t c = 0; c < n; ++c) gather[(size_t)c] = perm ? perm[c] : c;
    const size_t n_bits = (size_t)n_cw * (size_t)n, n_soft = n_bits * (size_t)rounds;
    dev_buf<int8_t> d_soft;
    dev_buf<int32_t> d_gather, d_iters, d_round;
    dev_buf<uint8_t> d_bits, d_conv;
    if (!d_soft.alloc(n_soft) || !d_gather.alloc(gather.size()) || !d_bits.alloc(n_bits) || !d_iters.alloc((size_t)n_cw) ||
        !d_round.alloc((size_t)n_cw) || !d_conv.alloc((size_t)n_cw))
        return fail(WOFDM_E_NOMEM, "device allocation failed (decoder)");
    if (!d_soft.upload(soft, n_soft) || !d_gather.upload(gather.data(), gather.size())) return fail(WOFDM_E_HIP, "upload failed");
    wofdm_ldpcparams lp{};
    lp.soft = d_soft; lp.gather[0] = d_gather; lp.n[0] = n; lp.W[0] = 1; lp.Z[0] = Z; lp.J = J; lp.L = L; lp.max_iter = max_iter;
    lp.cw_stride = n; lp.n_cw = (uint32_t)n_cw; lp.bits = d_bits; lp.iters = d_iters; lp.conv = d_conv;
    const wofdm_harqparams hq = {rounds, combine, d_round};
    std::vector<uint8_t> hbits(n_bits), hconv((size_t)n_cw);
    std::vector<int32_t> hiters((size_t)n_cw), hround((size_t)n_cw);
    hipError_t e = hipSuccess;
    {
        std::lock_guard<std::mutex> gate(g_gate_mu);
        e = wofdm_ldpc_harq_launch(&lp, &hq, nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    if (e != hipSuccess || !fetch(hbits, d_bits.p) || !fetch(hiters, d_iters.p) || !fetch(hconv, d_conv.p) || !fetch(hround, d_round.p))
        return fail(WOFDM_E_HIP, "decoder kernel or copy-back failed: %s", hipGetErrorString(e != hipSuccess ? e : hipGetLastError()));
    std::memcpy(bits, hbits.data(), n_bits);
    if (round) std::memcpy(round, hround.data(), hround.size() * sizeof(int32_t));
    if (iters) std::memcpy(iters, hiters.data(), hiters.size() * sizeof(int32_t));
    if (converged) std::memcpy(converged, hconv.data(), hconv.size());
    return WOFDM_OK;
}

int wofdm_coset_info(uint64_t seed, uint32_t cell, uint64_t frame, int32_t n_bits, uint8_t *bits)
{
    if (!bits) return fail(WOFDM_E_INVALID, "NULL argument (bits)");
    if (n_bits < 0) return fail(WOFDM_E_INVALID, "n_bits=%d must be >= 0", n_bits);
    if (cell >= (1u << 28)) return fail(WOFDM_E_INVALID, "cell=%u must be below 2^28", cell);
    uint32_t word = 0;
    for (int32_t i = 0; i < n_bits; ++i) {
        if ((i & 31) == 0) word = wofdm_info_word((uint32_t)seed, (uint32_t)(seed >> 32), cell, frame, (uint32_t)i >> 5);
        bits[i] = (uint8_t)((word >> (i & 31)) & 1u);
    }
    return WOFDM_OK;
}

int wofdm_conv_encode(int device, int32_t rate, int32_t n_c, int32_t n_cw, const uint8_t *info, uint8_t *coded)
{
    if (!info || !coded) return fail(WOFDM_E_INVALID, "NULL argument (info or coded)");
    if (rate < 0 || rate > 2) return fail(WOFDM_E_INVALID, "rate=%d must be 0, 1 or 2", rate);
    if (n_c < 1 || n_cw < 1) return fail(WOFDM_E_INVALID, "n_c=%d and n_cw=%d must be >= 1", n_c, n_cw);
    const int32_t T = code_steps(rate, n_c);
    if (T < 7) return fail(WOFDM_E_INVALID, "n_c=%d gives %d steps, at least 7 are needed", n_c, T);
    if (T > WOFDM_CODE_LONG_MAX_STEPS)
        return fail(WOFDM_E_UNSUPPORTED, "n_c=%d gives %d steps, more than %d", n_c, T, WOFDM_CODE_LONG_MAX_STEPS);
    int rc = use_device(device);
    if (rc != WOFDM_OK) return rc;
    const size_t n_info = (size_t)n_cw * (size_t)(T - 6), n_coded = (size_t)n_cw * (size_t)n_c;
    dev_buf<uint8_t> d_info, d_coded;
    // (T = 7 at one codeword: one information bit; the buffers are never empty)
    if (!d_info.alloc(n_info) || !d_coded.alloc(n_coded)) return fail(WOFDM_E_NOMEM, "device allocation failed (encoder)");
    if (!d_info.upload(info, n_info)) return fail(WOFDM_E_HIP, "upload failed");
    wofdm_convencparams ep{};
    ep.info = d_info; ep.coded = d_coded; ep.rate = rate; ep.n_c = n_c; ep.steps = T; ep.n_cw = (uint32_t)n_cw;
    std::vector<uint8_t> hcoded(n_coded);
    hipError_t e;
    {
        std::lock_guard<std::mutex> gate(g_gate_mu);
        e = wofdm_conv_encode_launch(&ep, nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    if (e != hipSuccess || !fetch(hcoded, d_coded.p))
        return fail(WOFDM_E_HIP, "encoder kernel or copy-back failed: %s", hipGetErrorString(e != hipSuccess ? e : hipGetLastError()));
    std::memcpy(coded, hcoded.data(), n_coded);
    return WOFDM_OK;
}

int wofdm_ldpc_encode(int device, int32_t J, int32_t L, int32_t n, int32_t n_cw, const uint8_t *info, uint8_t *word)
{
    if (!info || !word) return fail(WOFDM_E_INVALID, "NULL argument (info or word)");
    if (!ldpc_ranges_ok(J, L)) return fail(WOFDM_E_INVALID, "J=%d must be 3 ... 6 and L=%d in J + 1 ... 24", J, L);
    if (n < 1 || n_cw < 1) return fail(WOFDM_E_INVALID, "n=%d and n_cw=%d must be >= 1", n, n_cw);
    if (n > WOFDM_LDPC_MAX_BITS) return fail(WOFDM_E_UNSUPPORTED, "n=%d exceeds %d", n, WOFDM_LDPC_MAX_BITS);
    const int32_t Z = ldpc_lift(J, L, n);
    if ((int64_t)(L - J) * Z - ((int64_t)L * Z - n) < 1)
        return fail(WOFDM_E_INVALID, "(%d, %d) over %d positions has no information bit", J, L, n);
    if (wofdm_ldpc_lds(J, L, Z) > WOFDM_LDPC_LDS_MAX) return fail(WOFDM_E_UNSUPPORTED, "the decoder's LDS exceeds %d bytes", WOFDM_LDPC_LDS_MAX);
    int rc = use_device(device);
    if (rc != WOFDM_OK) return rc;
    const size_t n_info = (size_t)n_cw * (size_t)(n - J * Z), n_word = (size_t)n_cw * (size_t)n;
    dev_buf<uint8_t> d_info, d_word;
    if (!d_info.alloc(n_info) || !d_word.alloc(n_word)) return fail(WOFDM_E_NOMEM, "device allocation failed (encoder)");
    if (!d_info.upload(info, n_info)) return fail(WOFDM_E_HIP, "upload failed");
    wofdm_ldpcencparams ep{};
    ep.info = d_info; ep.word = d_word; ep.J = J; ep.L = L; ep.n = n; ep.Z = Z; ep.n_cw = (uint32_t)n_cw;
    std::vector<uint8_t> hword(n_word);
    hipError_t e;
    {
        std::lock_guard<std::mutex> gate(g_gate_mu);
        e = wofdm_ldpc_encode_launch(&ep, nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    if (e != hipSuccess || !fetch(hword, d_word.p))
        return fail(WOFDM_E_HIP, "encoder kernel or copy-back failed: %s", hipGetErrorString(e != hipSuccess ? e : hipGetLastError()));
    std::memcpy(word, hword.data(), n_word);
    return WOFDM_OK;
}

int wofdm_rx_profile_kernel_ms(float *ms)
{
    if (!ms) return fail(WOFDM_E_INVALID, "NULL argument");
    *ms = g_rxprof_ms;
    return WOFDM_OK;
}

int wofdm_philox_kat(int device, const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4])
{
    if (!ctr || !key || !out) return fail(WOFDM_E_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(device));
    uint32_t hbuf[6] = {ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]};
    uint32_t *d = nullptr;
    HIP_TRY(hipMalloc(&d, 10 * sizeof(uint32_t)));
    int rc = WOFDM_OK;
    if (hipMemcpy(d, hbuf, sizeof hbuf, hipMemcpyHostToDevice) != hipSuccess ||
        wofdm_philox_kat_launch(d, d + 6, nullptr) != hipSuccess ||
        hipMemcpy(out, d + 6, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail(WOFDM_E_HIP, "philox KAT failed: %s", hipGetErrorString(hipGetLastError()));
    (void)hipFree(d);
    return rc;
}

}  // extern "C"
