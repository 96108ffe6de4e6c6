// wofdm_aux.hip -- the auxiliary kernels beside the frame kernel: closed-form ICI/ISI power (wofdm_interference,
// wofdm_interference_masked) and Tx waveform + averaged periodogram (wofdm_tx_psd, wofdm_tx_psd_batch,
// wofdm_tx_psd_batch_masked), the Tx PAPR (wofdm_tx_papr) and the per-subcarrier receive profile (wofdm_rx_profile; beside an adjacent-band neighbour: wofdm_rx_profile_aci; under receiver timing and carrier offsets: wofdm_rx_profile_sync; over channels that move within the frame: wofdm_rx_profile_doppler; behind a nonlinear power amplifier: wofdm_rx_profile_pa, wofdm_tx_psd_batch_pa; under oscillator phase noise: wofdm_rx_profile_pn).  Compiled once per DFT length (-DWOFDM_TU_N=<N>, see the Makefile); wofdm_kernel.h dispatches
// on n_fft through the unit's table of launchers (wofdm_aux_fns).  The coded link's decoders and encoders do not know the DFT
// length and live in a unit of their own, wofdm_code.hip: the receive kernel here writes the soft bits (wofdm_rxprof_coded_kernel),
// rx_profile_chunk decides which decoder runs behind it and calls that unit's wofdm_*_enqueue functions (wofdm_link.h).
#include "wofdm_kernel.h"
#include "wofdm_link.h"
#include "wofdm_device.h"
#include "philox.h"
#include <type_traits>

#if !defined(WOFDM_TU_N)
#error "compile with -DWOFDM_TU_N=<64|128|256|512|1024>"
#endif
#define WOFDM_CAT2(a, b) a##b
#define WOFDM_CAT(a, b) WOFDM_CAT2(a, b)

namespace {

// ---------------------------------------------------------------------------------------------
// Closed-form ICI + ISI power of a structure:
//   calculate_interference  matlab/main_interference_calculation.m:177-225
//   interf_power            python/ofdm_utils/interf_calc.py:20-113
//     A_m = W K P V_rx R  H_m  V_tx Gamma W^-1,   H_m[b, c] = h[m B + b - c],   m = 0, 1
//     P[n] = sum_{n' != n} |A_0[n, n']|^2 + sum_{n'} |A_1[n, n']|^2
// Column n' of A_m is the frame pipeline's own answer to a unit symbol on subcarrier n': the windowed,
// CP/CS-extended complex exponential x (the Tx matrix applied to e_n'), the 21-tap convolution over two
// symbol periods, and per period the Rx window / fold / shift + DFT of the frame kernel -- no dense
// matrices, no RNG.  One workgroup per (window pair, channel) job; a wave takes the columns
// n' = wave, wave + W, ... and keeps |A|^2 row sums of its subcarriers (FFT output layout) in registers;
// one LDS reduction over the waves at the end.  (M = 1 + ceil((L - 1 + beta) / B) = 2 for every
// supported structure: B >= 64 > 36.)
struct wofdm_iparams {
    int P, B, mu, delta, gam, kap, n_ch, rowlen;   // rowlen: float2 per wave row (24 + 2B + 24 rounded up)
    float *power;                                  // [pairs][n_ch][N]
};
template <int N> struct interf_geo {
    static constexpr int WAVES = N <= 256 ? 16 : (N == 512 ? 8 : 4);
    static constexpr int RB2 = 2 * (N / 64 + 1);                      // FIR outputs per lane over 2B samples
    static constexpr int CH = RB2 % 6 == 0 ? 6 : (RB2 % 5 == 0 ? 5 : (RB2 % 4 == 0 ? 4 : 2));
};

template <int N>
__global__ void __launch_bounds__(interf_geo<N>::WAVES * 64)
wofdm_interf_kernel(const wofdm_iparams p, const float *__restrict__ g_wtx, const float *__restrict__ g_wrx,
                    const float2 *__restrict__ g_h_)
{
    constexpr int WAVES = interf_geo<N>::WAVES, RB2 = interf_geo<N>::RB2, LT = WOFDM_LT;
    constexpr int BPL = geo<N>::BPL, NQ = geo<N>::NQ;
    constexpr bool FULL = geo<N>::FULL;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // LDS: FFT stage twiddles [N] | e^{+2 pi i k / N} [N] | w_rx [N + 64] | per wave: row [rowlen] + scratch [N]
    v2f *tw = reinterpret_cast<v2f *>(smem);
    v2f *wn = tw + N;
    float *wrx = reinterpret_cast<float *>(wn + N);
    v2f *rows = reinterpret_cast<v2f *>(wrx + N + 64);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int job = blockIdx.x, pair = job / p.n_ch, ch = job - pair * p.n_ch;
    const int P = p.P, B = p.B;
    fill_twiddles<N>(tw, tid, WAVES * 64);
    for (int i = tid; i < N; i += WAVES * 64) {
        float sv, cv;
        sincospif(2.0f * (float)i / (float)N, &sv, &cv);
        wn[i] = mk(cv, sv);
    }
    for (int i = tid; i < N + p.delta; i += WAVES * 64) wrx[i] = g_wrx[(size_t)pair * (N + p.delta) + i];
    v2f *row = rows + (size_t)wv * (p.rowlen + N);
    v2f *scr = row + p.rowlen;
    for (int i = lane; i < p.rowlen; i += 64) row[i] = mk(0.f, 0.f);
    __syncthreads();
    const v2f *__restrict__ taps = reinterpret_cast<const v2f *>(g_h_) + (size_t)ch * LT;
    const float *__restrict__ wtx = g_wtx + (size_t)pair * P;
    float pw[BPL][4];
#pragma unroll
    for (int q = 0; q < BPL; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) pw[q][r] = 0.f;
    const int h2 = p.delta >> 1;
    for (int np = wv; np < N; np += WAVES) {
        // x[c] = w_tx[c] e^{2 pi i ((c - mu) mod N) n' / N} / N at row[24 + c]  (tx matrix column, m:358-376)
        for (int c = lane; c < P; c += 64) {
            const int t = (c - p.mu) & (N - 1);
            row[24 + c] = wn[(t * np) & (N - 1)] * (wtx[c] * (1.0f / (float)N));
        }
        for (int c = P + lane; c < 2 * B + 24; c += 64) row[24 + c] = mk(0.f, 0.f);
        wave_sync();
        // z = conv(h, x) over two symbol periods (m:260): lane -> RB2 consecutive outputs from j0
        v2f acc[RB2];
        const int j0 = lane * RB2;
        fir_lane<RB2, interf_geo<N>::CH>(row + 24 - (LT - 1) + j0, taps, acc);
        wave_sync();
#pragma unroll
        for (int r = 0; r < RB2; ++r)
            if (j0 + r < 2 * B) row[24 + j0 + r] = acc[r];
        wave_sync();
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            // Rx window, fold, circular shift (m:297-355) of period m, then the DFT
            const v2f *fb = row + 24 + m * B;
            v2f v[1][BPL][4];
#pragma unroll
            for (int q = 0; q < BPL; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    v[0][q][r] = mk(0.f, 0.f);
                    if (!(FULL || lane + 64 * q < NQ)) continue;
                    const int m0 = (lane + 64 * q + r * NQ + p.kap + h2) & (N - 1);
                    v2f z = fb[p.gam + m0] * wrx[m0];
                    if (m0 < p.delta) {
                        const float w2 = wrx[m0 + N];
                        z = __builtin_elementwise_fma(mk(w2, w2), fb[p.gam + m0 + N], z);
                    }
                    v[0][q][r] = z;
                }
            fft_wave<N, -1, 1>(v, scr, 0, tw, lane);
#pragma unroll
            for (int q = 0; q < BPL; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int n = lane + 64 * q + r * NQ;
                    const float e = v[0][q][r].x * v[0][q][r].x + v[0][q][r].y * v[0][q][r].y;
                    if (FULL || lane + 64 * q < NQ)
                        pw[q][r] += (m == 0 && n == np) ? 0.f : e;    // the wanted term A_0[n, n] is no interference
                }
        }
        wave_sync();
    }
    // sum over the waves (each wave's row is free now): float [WAVES][N] in the rows area
    __syncthreads();
    float *red = reinterpret_cast<float *>(rows);
#pragma unroll
    for (int q = 0; q < BPL; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (FULL || lane + 64 * q < NQ) red[wv * N + lane + 64 * q + r * NQ] = pw[q][r];
    __syncthreads();
    for (int n = tid; n < N; n += WAVES * 64) {
        float t = 0.f;
        for (int w = 0; w < WAVES; ++w) t += red[w * N + n];
        p.power[(size_t)job * N + n] = t;
    }
}

// ---------------------------------------------------------------------------------------------
// Tx-side spectrum estimate: the transmitted waveform of a long run of symbols
// and its averaged periodogram,
//   wOFDMSystem.estimate_obr   python/ofdm_utils/timefreq_simulation.py:216-296 (Tx chain 242-258)
//   psd_estimate               timefreq_simulation.py:101-123
// The waveform kernel is phase A of the frame kernel fed with given symbols X[s][n] (any complex values,
// zeros on unloaded bins): IDFT, CP/CS copy, Tx window, overlap-add of the `overlap` tail samples --
// one wave per symbol, the overlapping samples by float atomics (two addends: order-independent).
struct wofdm_wparams {
    int P, mu, rho, overlap, no_symbols;
    float2 *x;                         // [overlap + no_symbols * (P - overlap)], zeroed by the host
};
// The symbol of both waveform kernels: X -> IDFT -> CP / CS copy x Tx window onto the waveform row `out` (the symbol's first
// sample); Bo = P - overlap samples further the next symbol starts.
template <int N>
__device__ __forceinline__ void txwave_symbol(const float2 *Xs, const float *wtx, float2 *out, int cp, int cs, int overlap,
                                              int Bo, int lane, v2f *scr, const v2f *tw)
{
    constexpr int BPL = geo<N>::BPL, NQ = geo<N>::NQ;
    constexpr bool FULL = geo<N>::FULL;
    v2f v[1][BPL][4];
#pragma unroll
    for (int q = 0; q < BPL; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            v[0][q][r] = mk(0.f, 0.f);
            if (FULL || lane + 64 * q < NQ) v[0][q][r] = ldg2(Xs + lane + 64 * q + r * NQ);
        }
    fft_wave<N, +1, 1>(v, scr, 0, tw, lane);                    // N x[t]
    auto put = [&](int i, v2f val) {
        val = val * (wtx[i] * (1.0f / (float)N));
        if (i < overlap || i >= Bo) {                            // shared with a neighbour symbol
            atomicAdd(&out[i].x, val.x);
            atomicAdd(&out[i].y, val.y);
        } else {
            out[i] = make_float2(val.x, val.y);
        }
    };
#pragma unroll
    for (int q = 0; q < BPL; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (!(FULL || lane + 64 * q < NQ)) continue;
            const int t = lane + 64 * q + r * NQ;
            put(t + cp, v[0][q][r]);
            if (t >= N - cp) put(t + cp - N, v[0][q][r]);
            if (t < cs) put(t + cp + N, v[0][q][r]);
        }
}
template <int N>
__global__ void __launch_bounds__(1024) wofdm_txwave_kernel(const wofdm_wparams p, const float *__restrict__ g_wtx,
                                                            const float2 *__restrict__ X)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    v2f *tw = reinterpret_cast<v2f *>(smem);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    v2f *scr = tw + N + (size_t)wv * N;
    fill_twiddles<N>(tw, tid, 1024);
    __syncthreads();
    const int s = blockIdx.x * 16 + wv;
    if (s >= p.no_symbols) return;
    const int Bo = p.P - p.overlap;
    txwave_symbol<N>(X + (size_t)s * N, g_wtx, p.x + (size_t)s * Bo, p.mu, p.rho, p.overlap, Bo, lane, scr, tw);
}

// Sum over consecutive FL-sample slices of x (the zero-padded remainder included) of |FFT_FL|^2, written
// fftshift-ed; the caller divides by the reference's slice count.  FL = 2048 runs as two 1024-point
// transforms of the even and odd samples and one radix-2 combination in registers.
template <int FL>
__global__ void __launch_bounds__(512) wofdm_psd_kernel(const float2 *__restrict__ x, int len, int n_slices,
                                                        float *__restrict__ psd)
{
    constexpr int M = FL == 2048 ? 1024 : FL, H = FL / M;        // transform length, transforms per slice
    constexpr int BPL = geo<M>::BPL, NQ = geo<M>::NQ, WAVES = 8;
    static_assert(geo<M>::FULL, "at least 256 points");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    v2f *tw = reinterpret_cast<v2f *>(smem);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    v2f *scr = tw + M + (size_t)wv * M;
    fill_twiddles<M>(tw, tid, WAVES * 64);
    __syncthreads();
    float acc[H][BPL][4];
#pragma unroll
    for (int h = 0; h < H; ++h)
#pragma unroll
        for (int q = 0; q < BPL; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[h][q][r] = 0.f;
    for (int sl = wv; sl < n_slices; sl += WAVES) {
        v2f e[1][BPL][4], o[1][BPL][4];
#pragma unroll
        for (int h = 0; h < H; ++h) {
            v2f (&dst)[1][BPL][4] = h == 0 ? e : o;
#pragma unroll
            for (int q = 0; q < BPL; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int idx = sl * FL + H * (lane + 64 * q + r * NQ) + h;       // even / odd samples
                    dst[0][q][r] = idx < len ? ldg2(x + idx) : mk(0.f, 0.f);
                }
            fft_wave<M, -1, 1>(dst, scr, 0, tw, lane);
        }
#pragma unroll
        for (int q = 0; q < BPL; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if constexpr (H == 2) {
                    const int k = lane + 64 * q + r * NQ;
                    float sv, cv;
                    sincospif(-2.0f * (float)k / (float)FL, &sv, &cv);
                    const v2f wo = cmul(o[0][q][r], mk(cv, sv));
                    const v2f a = e[0][q][r] + wo, b = e[0][q][r] - wo;
                    acc[0][q][r] += a.x * a.x + a.y * a.y;
                    acc[1][q][r] += b.x * b.x + b.y * b.y;
                } else {
                    acc[0][q][r] += e[0][q][r].x * e[0][q][r].x + e[0][q][r].y * e[0][q][r].y;
                }
            }
    }
    __syncthreads();
    float *red = reinterpret_cast<float *>(tw + M);                 // [WAVES][FL] over the scratch rows
#pragma unroll
    for (int h = 0; h < H; ++h)
#pragma unroll
        for (int q = 0; q < BPL; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[wv * FL + h * M + lane + 64 * q + r * NQ] = acc[h][q][r];
    __syncthreads();
    for (int k = tid; k < FL; k += WAVES * 64) {
        float t = 0.f;
        for (int w = 0; w < WAVES; ++w) t += red[w * FL + k];
        psd[(k + FL / 2) & (FL - 1)] = t;
    }
}

// The same two steps for a batch of jobs at every N (wofdm_tx_psd_batch).  The waveform kernel: grid (symbol groups,
// jobs), one wave per symbol of the job's block, each job with its own cp, cs, overlap, window and waveform row; the
// overlapping samples as above (two addends onto a zeroed row).  LDS: twiddles [N] + one scratch row [N] per wave
// (N = 1024: 9 x 8 KB).
template <int N> struct bwave_geo {
    static constexpr int WAVES = N >= 512 ? 8 : 16;
};
template <int N>
__global__ void __launch_bounds__(bwave_geo<N>::WAVES * 64)
wofdm_txwave_batch_kernel(const wofdm_bjob *__restrict__ jobs, int no_symbols, const float *__restrict__ g_wtx,
                          const float2 *__restrict__ X, float2 *__restrict__ x)
{
    constexpr int WAVES = bwave_geo<N>::WAVES;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    v2f *tw = reinterpret_cast<v2f *>(smem);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    v2f *scr = tw + N + (size_t)wv * N;
    fill_twiddles<N>(tw, tid, WAVES * 64);
    __syncthreads();
    const wofdm_bjob jb = jobs[blockIdx.y];
    const int s = blockIdx.x * WAVES + wv;
    if (s >= no_symbols) return;
    const int Bo = N + jb.cp + jb.cs - jb.overlap;
    txwave_symbol<N>(X + ((size_t)jb.block * no_symbols + s) * N, g_wtx + jb.w_off, x + jb.x_off + (size_t)s * Bo, jb.cp, jb.cs,
                     jb.overlap, Bo, lane, scr, tw);
}

// Periodogram of a batch: one workgroup (8 waves) per work item, i.e. up to wofdm_psd_batch_slices(N) consecutive
// FL-sample slices of one job.  FL <= 1024 (R = 1): a wave transforms a whole slice, 8 slices at a time.  FL = 1024 R,
// R = 2, 4, 8: the R waves of a group transform the decimated sub-sequences x[R m + h] of one slice (1024 points each,
// E_h), put E_h into their scratch rows and, behind a barrier, combine them:  X[k' + 1024 c] = sum_h W_R^(h c)
// (W_FL^(h k') E_h[k']).  Wave h of the group owns k' = h 1024 / R + lane + 64 j (j < 16 / R), i.e. 16 outputs per lane,
// whose twiddles it keeps in registers; its loads of the R rows are consecutive 8-byte words across the lanes, as are the
// stores of E_h (ds_read_b64 / ds_write_b64 without bank conflicts).  Every lane adds |X|^2 over its slices in a fixed
// order, the groups' sums are added in group order, and the workgroup writes one unshifted partial spectrum [FL];
// wofdm_psd_reduce_kernel adds a job's partials in item order -- no atomics: bitwise repeatable.
template <int FL>
__global__ void __launch_bounds__(512) wofdm_psd_batch_kernel(const wofdm_bjob *__restrict__ jobs,
                                                              const wofdm_bitem *__restrict__ items,
                                                              const float2 *__restrict__ x, float *__restrict__ partial)
{
    constexpr int R = wofdm_psd_batch_r(FL / 8), M = FL / R, G = 8 / R, ROUNDS = wofdm_psd_batch_slices(FL / 8) / G;
    constexpr int BPL = geo<M>::BPL, NQ = geo<M>::NQ, JJ = M / (64 * R), NACC = R > 1 ? JJ * R : 4 * BPL;
    static_assert(geo<M>::FULL && (R == 1 || M == 1024), "512- or 1024-point transforms");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    v2f *tw = reinterpret_cast<v2f *>(smem);
    v2f *rows = tw + M;                                           // [8][M]: scratch of wave w = E_h of group w / R
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = wv / R, h = wv % R;
    fill_twiddles<M>(tw, tid, 512);
    const wofdm_bitem it = items[blockIdx.x];
    const wofdm_bjob jb = jobs[it.job];
    const float2 *xj = x + jb.x_off;
    v2f cw[JJ][R > 1 ? R - 1 : 1];                                // W_FL^(t k'), t = 1 .. R-1
    if constexpr (R > 1) {
#pragma unroll
        for (int j = 0; j < JJ; ++j)
#pragma unroll
            for (int t = 1; t < R; ++t) {
                const int kp = h * (M / R) + lane + 64 * j;
                float sv, cv;
                sincospif(-2.0f * (float)(t * kp) / (float)FL, &sv, &cv);
                cw[j][t - 1] = mk(cv, sv);
            }
    }
    float acc[NACC];
#pragma unroll
    for (int a = 0; a < NACC; ++a) acc[a] = 0.f;
    __syncthreads();
    v2f *own = rows + (size_t)wv * M;
    for (int rd = 0; rd < ROUNDS; ++rd) {
        const int sl = rd * G + g;
        const bool live = sl < it.n_slices;                       // uniform over the group
        if (live) {
            const int base = (it.slice0 + sl) * FL + h;
            v2f v[1][BPL][4];
#pragma unroll
            for (int q = 0; q < BPL; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int idx = base + R * (lane + 64 * q + r * NQ);
                    v[0][q][r] = idx < jb.len ? ldg2(xj + idx) : mk(0.f, 0.f);
                }
            fft_wave<M, -1, 1>(v, own, 0, tw, lane);
#pragma unroll
            for (int q = 0; q < BPL; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if constexpr (R == 1) acc[4 * q + r] += v[0][q][r].x * v[0][q][r].x + v[0][q][r].y * v[0][q][r].y;
                    else own[lane + 64 * q + r * NQ] = v[0][q][r];
                }
        }
        if constexpr (R > 1) {
            __syncthreads();
            if (live) {
                const v2f *gs = rows + (size_t)g * R * M;
#pragma unroll
                for (int j = 0; j < JJ; ++j) {
                    const int kp = h * (M / R) + lane + 64 * j;
                    v2f y[R];
#pragma unroll
                    for (int t = 0; t < R; ++t) y[t] = gs[t * M + kp];
#pragma unroll
                    for (int t = 1; t < R; ++t) y[t] = cmul(y[t], cw[j][t - 1]);
                    v2f X_[R];
                    if constexpr (R == 2) {
                        X_[0] = y[0] + y[1];
                        X_[1] = y[0] - y[1];
                    } else if constexpr (R == 4) {
                        v2f u[4] = {y[0], y[1], y[2], y[3]};
                        radix4<-1>(u);
#pragma unroll
                        for (int c = 0; c < 4; ++c) X_[c] = u[c];
                    } else {
                        v2f u[2][4];                              // u[q][r] = y_t, t = q + 2 r
#pragma unroll
                        for (int t = 0; t < 8; ++t) u[t & 1][t >> 1] = y[t];
                        dft8<-1>(u);                              // u[q][r] = X_c, c = r + 4 q
#pragma unroll
                        for (int c = 0; c < 8; ++c) X_[c] = u[c >> 2][c & 3];
                    }
#pragma unroll
                    for (int c = 0; c < R; ++c) acc[j * R + c] += X_[c].x * X_[c].x + X_[c].y * X_[c].y;
                }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    float *red = reinterpret_cast<float *>(rows);                 // [G][FL] floats over the scratch rows
    if constexpr (R == 1) {
#pragma unroll
        for (int q = 0; q < BPL; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[g * FL + lane + 64 * q + r * NQ] = acc[4 * q + r];
    } else {
#pragma unroll
        for (int j = 0; j < JJ; ++j)
#pragma unroll
            for (int c = 0; c < R; ++c) red[g * FL + h * (M / R) + lane + 64 * j + M * c] = acc[j * R + c];
    }
    __syncthreads();
    for (int k = tid; k < FL; k += 512) {
        float t = 0.f;
        for (int gg = 0; gg < G; ++gg) t += red[gg * FL + k];
        partial[(size_t)blockIdx.x * FL + k] = t;
    }
}

// psd[job][8 N] = sum over the job's work items, in item order, of their partial spectra; fftshift-ed
template <int FL>
__global__ void __launch_bounds__(256) wofdm_psd_reduce_kernel(const wofdm_bjob *__restrict__ jobs,
                                                               const float *__restrict__ partial, float *__restrict__ psd)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= FL) return;
    const wofdm_bjob jb = jobs[blockIdx.y];
    float t = 0.f;
    for (int i = 0; i < jb.n_items; ++i) t += partial[(size_t)(jb.item0 + i) * FL + k];
    psd[(size_t)blockIdx.y * FL + ((k + FL / 2) & (FL - 1))] = t;
}

// Waveform step of a MASKED job (wofdm_tx_psd_batch_masked): per symbol the row r_s[P] of wofdm_txwave_batch_kernel
// (IDFT, CP/CS copy, Tx window), then the spectral Tx mask of wofdm_plan_set_tx_mask as fast convolution over FL = 8 N
// points (3 P - 2 <= FL):  y_s[i] = IFFT_FL( FFT_FL(r_s) . H )[i + P - 1], i < 2 P - 1, with H the transform of the mask's
// impulse response laid out as in the frame kernel's TXFFT variant, 1 / FL folded in (host, fp64; stored in fp32).
// The FL-point transforms are the R-way split of wofdm_psd_batch_kernel (R waves, M = FL / R points each) and its
// transpose:  forward  X[k' + M c] = sum_h W_R^(h c) (W_FL^(h k') E_h[k']),  E_h = FFT_M(r[R m + h]);
//             inverse  y[R m + h] = IFFT_M(F_h)[m],  F_h[k'] = W_FL^(-h k') sum_c W_R^(-h c) Z[k' + M c].
// Wave h of a group owns k' = h M / R + lane + 64 j in the combination, takes all R bins k' + M c, multiplies them by H
// and runs the inverse combination in registers -- the spectrum never leaves the workgroup.  8 waves = 8 / R symbols
// per workgroup.  LDS: twiddles [M] (+ [N] where N != M) | rows [8][M] | symbol rows [8 / R][PMAX].
// Output: the WHOLE y_s (2 P - 1 samples) by plain stores at Y + y_off + s (2 P - 1); the spill of symbol s onto s + 1
// and the overlap-add are the gather of wofdm_txmask_ola_kernel -- no atomics, a fixed order of additions.
template <int N> struct bmask_geo {
    static constexpr int FL = 8 * N, R = wofdm_psd_batch_r(N), M = FL / R, G = 8 / R;
    static constexpr int PMAX = wofdm_txmask_batch_pmax(N);
    static constexpr int TWN = N == M ? 0 : N;                    // a twiddle table of its own for the N-point IDFT
    static constexpr size_t LDS = 8 * (size_t)(M + TWN + 8 * M + G * PMAX);
    static_assert(LDS <= 160 * 1024 && N <= M && 3 * PMAX - 2 <= FL, "LDS / transform length");
};
template <int N>
__global__ void __launch_bounds__(512)
wofdm_txmask_batch_kernel(const wofdm_bjob *__restrict__ jobs, const wofdm_mjob *__restrict__ mjobs, int no_symbols,
                          const float *__restrict__ g_wtx, const float2 *__restrict__ X, const float2 *__restrict__ spec,
                          float2 *__restrict__ Y)
{
    using MG = bmask_geo<N>;
    constexpr int FL = MG::FL, R = MG::R, M = MG::M, G = MG::G, PMAX = MG::PMAX;
    constexpr int BPL = geo<M>::BPL, NQ = geo<M>::NQ, JJ = M / (64 * R);
    constexpr int BPLN = geo<N>::BPL, NQN = geo<N>::NQ;
    constexpr bool FULLN = geo<N>::FULL;
    static_assert(geo<M>::FULL, "512- or 1024-point transforms");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    v2f *twm = reinterpret_cast<v2f *>(smem);
    v2f *twn = N == M ? twm : twm + M;
    v2f *rows = twm + M + MG::TWN;                                // [8][M]
    v2f *srows = rows + 8 * M;                                    // [G][PMAX]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = wv / R, h = wv % R;
    fill_twiddles<M>(twm, tid, 512);
    if constexpr (N != M) fill_twiddles<N>(twn, tid, 512);
    const wofdm_mjob mj = mjobs[blockIdx.y];
    const wofdm_bjob jb = jobs[mj.job];
    const int P = N + jb.cp + jb.cs, L = 2 * P - 1;
    const int s = blockIdx.x * G + g;
    const bool live = s < no_symbols;                             // uniform over the group
    v2f cw[JJ][R > 1 ? R - 1 : 1];                                // W_FL^(t k'), t = 1 .. R-1
    if constexpr (R > 1) {
#pragma unroll
        for (int j = 0; j < JJ; ++j)
#pragma unroll
            for (int t = 1; t < R; ++t) {
                const int kp = h * (M / R) + lane + 64 * j;
                float sv, cv;
                sincospif(-2.0f * (float)(t * kp) / (float)FL, &sv, &cv);
                cw[j][t - 1] = mk(cv, sv);
            }
    }
    __syncthreads();
    v2f *own = rows + (size_t)wv * M;
    v2f *srow = srows + (size_t)g * PMAX;
    if (live && h == 0) {                                         // r_s: as wofdm_txwave_batch_kernel, into LDS
        const float2 *Xs = X + ((size_t)jb.block * no_symbols + s) * N;
        v2f v[1][BPLN][4];
#pragma unroll
        for (int q = 0; q < BPLN; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[0][q][r] = mk(0.f, 0.f);
                if (FULLN || lane + 64 * q < NQN) v[0][q][r] = ldg2(Xs + lane + 64 * q + r * NQN);
            }
        fft_wave<N, +1, 1>(v, own, 0, twn, lane);                 // N x[t]
        const float *wtx = g_wtx + jb.w_off;
        auto put = [&](int i, v2f val) { srow[i] = val * (wtx[i] * (1.0f / (float)N)); };
#pragma unroll
        for (int q = 0; q < BPLN; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (!(FULLN || lane + 64 * q < NQN)) continue;
                const int t = lane + 64 * q + r * NQN;
                put(t + jb.cp, v[0][q][r]);
                if (t >= N - jb.cp) put(t + jb.cp - N, v[0][q][r]);
                if (t < jb.cs) put(t + jb.cp + N, v[0][q][r]);
            }
    }
    __syncthreads();
    v2f v[1][BPL][4];
    if (live) {
#pragma unroll
        for (int q = 0; q < BPL; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int idx = R * (lane + 64 * q + r * NQ) + h;
                v[0][q][r] = idx < P ? srow[idx] : mk(0.f, 0.f);
            }
        fft_wave<M, -1, 1>(v, own, 0, twm, lane);
        if constexpr (R == 1) {
            const float2 *H = spec + (size_t)mj.spec * FL;
#pragma unroll
            for (int q = 0; q < BPL; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) v[0][q][r] = cmul(v[0][q][r], ldg2(H + lane + 64 * q + r * NQ));
        } else {
#pragma unroll
            for (int q = 0; q < BPL; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) own[lane + 64 * q + r * NQ] = v[0][q][r];
        }
    }
    if constexpr (R > 1) {
        __syncthreads();
        v2f F[JJ][R];                                             // F_t[k'] of this wave's k', t < R
        if (live) {
            const v2f *gs = rows + (size_t)g * R * M;
            const float2 *H = spec + (size_t)mj.spec * FL;
#pragma unroll
            for (int j = 0; j < JJ; ++j) {
                const int kp = h * (M / R) + lane + 64 * j;
                v2f y[R];
#pragma unroll
                for (int t = 0; t < R; ++t) y[t] = gs[t * M + kp];
#pragma unroll
                for (int t = 1; t < R; ++t) y[t] = cmul(y[t], cw[j][t - 1]);
                if constexpr (R == 2) {
                    const v2f z0 = cmul(y[0] + y[1], ldg2(H + kp)), z1 = cmul(y[0] - y[1], ldg2(H + kp + M));
                    F[j][0] = z0 + z1;
                    F[j][1] = z0 - z1;
                } else if constexpr (R == 4) {
                    v2f u[4] = {y[0], y[1], y[2], y[3]};
                    radix4<-1>(u);
#pragma unroll
                    for (int c = 0; c < 4; ++c) u[c] = cmul(u[c], ldg2(H + kp + M * c));
                    radix4<+1>(u);
#pragma unroll
                    for (int t = 0; t < 4; ++t) F[j][t] = u[t];
                } else {
                    v2f u[2][4], w[2][4];                         // u[q][r] = y_t, t = q + 2 r
#pragma unroll
                    for (int t = 0; t < 8; ++t) u[t & 1][t >> 1] = y[t];
                    dft8<-1>(u);                                  // u[q][r] = X_c, c = r + 4 q
#pragma unroll
                    for (int c = 0; c < 8; ++c) w[c & 1][c >> 1] = cmul(u[c >> 2][c & 3], ldg2(H + kp + M * c));
                    dft8<+1>(w);                                  // w[q][r] = F_t, t = r + 4 q
#pragma unroll
                    for (int t = 0; t < 8; ++t) F[j][t] = w[t >> 2][t & 3];
                }
#pragma unroll
                for (int t = 1; t < R; ++t) F[j][t] = cmul_conj(F[j][t], cw[j][t - 1]);
            }
        }
        __syncthreads();                                          // every wave has read the E rows
        if (live) {
            v2f *gs = rows + (size_t)g * R * M;
#pragma unroll
            for (int j = 0; j < JJ; ++j)
#pragma unroll
                for (int t = 0; t < R; ++t) gs[t * M + h * (M / R) + lane + 64 * j] = F[j][t];
        }
        __syncthreads();
        if (live) {
#pragma unroll
            for (int q = 0; q < BPL; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) v[0][q][r] = own[lane + 64 * q + r * NQ];
        }
    }
    if (!live) return;
    fft_wave<M, +1, 1>(v, own, 0, twm, lane);                     // y[R m + h + (P - 1)], the 1 / FL sits in H
    float2 *out = Y + mj.y_off + (size_t)s * L;
#pragma unroll
    for (int q = 0; q < BPL; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = R * (lane + 64 * q + r * NQ) + h - (P - 1);
            if (i >= 0 && i < L) out[i] = make_float2(v[0][q][r].x, v[0][q][r].y);
        }
}

// Filtered rows and overlap-add of a masked job, as a gather in a fixed order (no atomics):
//   row_s[i] = y_s[i] + y_{s-1}[P + i] (i < P - 1, s > 0),  row_s[P - 1] = y_s[P - 1]
//   x[s (P - overlap) + i] = row_s[i] (s < S) + row_{s-1}[i + P - overlap] (s > 0, i < overlap)
template <int N>
__global__ void __launch_bounds__(256)
wofdm_txmask_ola_kernel(const wofdm_bjob *__restrict__ jobs, const wofdm_mjob *__restrict__ mjobs, int no_symbols,
                        const float2 *__restrict__ Y, float2 *__restrict__ x)
{
    const wofdm_mjob mj = mjobs[blockIdx.y];
    const wofdm_bjob jb = jobs[mj.job];
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= jb.len) return;
    const int P = N + jb.cp + jb.cs, L = 2 * P - 1, Bo = P - jb.overlap;
    const float2 *y = Y + mj.y_off;
    auto row = [&](int ss, int i) {
        v2f a = ldg2(y + (size_t)ss * L + i);
        if (ss > 0 && i < P - 1) a = a + ldg2(y + (size_t)(ss - 1) * L + P + i);
        return a;
    };
    const int s = n / Bo, i = n - s * Bo;
    v2f val = mk(0.f, 0.f);
    if (s < no_symbols) val = row(s, i);
    if (s > 0 && i < jb.overlap) val = s < no_symbols ? val + row(s - 1, i + Bo) : row(s - 1, i + Bo);
    x[jb.x_off + n] = make_float2(val.x, val.y);
}

// ---------------------------------------------------------------------------------------------
// Closed-form ICI + ISI power of the half-band, spectrally masked system (wofdm_interference_masked):
//   zero padding + ifftshift  matlab/main_channel_mask.m:387-390
//   dft_rc_filt               matlab/main_channel_mask.m:398-417
//   calculate_interference    matlab/main_interference_calculation.m:177-225
// The mask turns the Tx column of bin n' into y = g (*) x (circular, length 2P - 1, g = the mask's impulse response);
// y[0, P) stays in the symbol's row and y[P, 2P - 1) goes into the next one, B samples later, so the on-air pulse is
//   u[j] = [j < P] y[j] + [B <= j < B + P - 1] y[P + j - B],   j < J = B + P - 1,
// and with the channel it covers three symbol periods: A_m, m = 0, 1, 2 (J + L - 1 <= 3 B for every supported
// geometry: tail_tx + L - 2 <= 35 < 64 <= B).
//
// Stage 1, once per window pair (the pulses do not depend on the channel): u is linear in x[c] = w_tx[c]
// e^{2 pi i ((c - mu) mod N) n' / N} / N, so for a fixed j the pulses of ALL bins are one N-point inverse DFT,
//   u[j][n'] = 1/N sum_t q_j[t] e^{2 pi i t n' / N},   q_j[t] = sum_{c < P, c = t + mu (mod N)} G[j][c] w_tx[c],
//   G[j][c] = [j < P] g[(j - c) mod (2P - 1)] + [B <= j < B + P - 1] g[j - B + P - c]
// -- a wave per sample j: it folds row j of G onto the N points and transforms; O(J (P + N log N)) per pair instead
// of O(J P N).  No mask (g == nullptr): u[j][n'] = x[j] itself, from the exponential table as wofdm_interf_kernel
// forms it.  cols[pair][n'][JP] holds the pulses, a row per bin; rows of unloaded bins are not written (nor read).
struct wofdm_mparams {
    int P, B, mu, delta, gam, kap, n_ch, J, JP;    // J = B + P - 1 pulse samples, JP = row pitch of cols
    float *power, *wanted;                         // [pairs][n_ch][N]; wanted may be null
};
template <int N> struct interfm_geo {
    // (the waves of wofdm_interf_kernel: the same columns per wave and the same order of the sums, so that without mask and
    // allocation the power comes out bit for bit as there)
    static constexpr int WAVES = interf_geo<N>::WAVES;
    static constexpr int RB3 = 3 * (N / 64 + 1);                      // FIR outputs per lane over 3B <= 3N + 192 samples
    static constexpr int CH = RB3 <= 6 ? RB3 : (RB3 % 5 == 0 ? 5 : 6);
    // 24 zeros (>= LT - 1 of history) + 64 RB3 samples: the last lane's FIR window ends at 64 RB3 + 23
    static constexpr int ROWLEN = 24 + 64 * RB3;
    // FFT stage twiddles [N] | w_rx [N + 64] | per wave: row [ROWLEN] + scratch [N]
    static constexpr int LDS = 8 * N + 4 * (N + 64) + WAVES * 8 * (ROWLEN + N);
    static_assert(LDS <= 160 * 1024 && WAVES * N * 4 <= WAVES * 8 * (ROWLEN + N), "LDS");
    static constexpr int PWAVES = N >= 512 ? 8 : 16;                  // pulse kernel: twiddles + e^{..} table + scratch rows
    static constexpr int PLDS = 8 * N * (2 + PWAVES);
};

template <int N>
__global__ void __launch_bounds__(interfm_geo<N>::PWAVES * 64)
wofdm_interf_pulse_kernel(const wofdm_mparams p, const float *__restrict__ g_wtx, const float2 *__restrict__ g,
                          const uint8_t *__restrict__ amask, float2 *__restrict__ cols)
{
    constexpr int BPL = geo<N>::BPL, NQ = geo<N>::NQ, WAVES = interfm_geo<N>::PWAVES;
    constexpr bool FULL = geo<N>::FULL;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    v2f *tw = reinterpret_cast<v2f *>(smem);
    v2f *wn = tw + N;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    v2f *scr = wn + N + (size_t)wv * N;
    fill_twiddles<N>(tw, tid, WAVES * 64);
    for (int i = tid; i < N; i += WAVES * 64) {
        float sv, cv;
        sincospif(2.0f * (float)i / (float)N, &sv, &cv);
        wn[i] = mk(cv, sv);
    }
    __syncthreads();
    const int pair = blockIdx.y, j = blockIdx.x * WAVES + wv;
    const int P = p.P, B = p.B, L = 2 * P - 1;
    if (j >= p.J) return;
    const float *__restrict__ wtx = g_wtx + (size_t)pair * P;
    v2f v[1][BPL][4];
    if (g == nullptr) {
        // u[j][n'] = x[j] = w_tx[j] e^{2 pi i ((j - mu) mod N) n' / N} / N (j < P), as wofdm_interf_kernel's Tx column
        const int t = (j - p.mu) & (N - 1);
        const float w = j < P ? wtx[j] * (1.0f / (float)N) : 0.f;
#pragma unroll
        for (int q = 0; q < BPL; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) v[0][q][r] = wn[(t * (lane + 64 * q + r * NQ)) & (N - 1)] * w;
    } else {
        const bool own = j < P, spill = j >= B;                  // (j < J = B + P - 1 here)
#pragma unroll
        for (int q = 0; q < BPL; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v2f a = mk(0.f, 0.f);
                if (FULL || lane + 64 * q < NQ) {
                    for (int c = (lane + 64 * q + r * NQ + p.mu) & (N - 1); c < P; c += N) {
                        v2f gg = mk(0.f, 0.f);
                        if (own) {
                            const int i = j - c;
                            gg = ldg2(g + (i < 0 ? i + L : i));
                        }
                        if (spill) gg = gg + ldg2(g + (j - B + P - c));     // in [1, 2P - 2]
                        a = a + gg * wtx[c];
                    }
                }
                v[0][q][r] = a;
            }
        fft_wave<N, +1, 1>(v, scr, 0, tw, lane);                 // N u[j][n']
#pragma unroll
        for (int q = 0; q < BPL; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) v[0][q][r] = v[0][q][r] * (1.0f / (float)N);
    }
#pragma unroll
    for (int q = 0; q < BPL; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int np = lane + 64 * q + r * NQ;
            if (!(FULL || lane + 64 * q < NQ) || (amask != nullptr && amask[np] == 0)) continue;
            cols[((size_t)pair * N + np) * p.JP + j] = make_float2(v[0][q][r].x, v[0][q][r].y);
        }
}

// Stage 2, one workgroup per (window pair, channel): wofdm_interf_kernel's pattern over the pulses of stage 1 -- FIR over
// three periods, per period Rx window / fold / shift + DFT, |.|^2 row sums in registers -- with the wanted term
// |A_0[n, n]|^2 kept apart and written out, the columns of unloaded bins skipped and the rows of unloaded bins zero.
template <int N>
__global__ void __launch_bounds__(interfm_geo<N>::WAVES * 64)
wofdm_interf_masked_kernel(const wofdm_mparams p, const float *__restrict__ g_wrx, const float2 *__restrict__ g_h_,
                           const uint8_t *__restrict__ amask, const float2 *__restrict__ cols)
{
    constexpr int WAVES = interfm_geo<N>::WAVES, RB3 = interfm_geo<N>::RB3, ROWLEN = interfm_geo<N>::ROWLEN, LT = WOFDM_LT;
    constexpr int BPL = geo<N>::BPL, NQ = geo<N>::NQ;
    constexpr bool FULL = geo<N>::FULL;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    v2f *tw = reinterpret_cast<v2f *>(smem);
    float *wrx = reinterpret_cast<float *>(tw + N);
    v2f *rows = reinterpret_cast<v2f *>(wrx + N + 64);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int job = blockIdx.x, pair = job / p.n_ch, ch = job - pair * p.n_ch;
    const int B = p.B;
    fill_twiddles<N>(tw, tid, WAVES * 64);
    for (int i = tid; i < N + p.delta; i += WAVES * 64) wrx[i] = g_wrx[(size_t)pair * (N + p.delta) + i];
    v2f *row = rows + (size_t)wv * (ROWLEN + N);
    v2f *scr = row + ROWLEN;
    for (int i = lane; i < ROWLEN; i += 64) row[i] = mk(0.f, 0.f);
    __syncthreads();
    const v2f *__restrict__ taps = reinterpret_cast<const v2f *>(g_h_) + (size_t)ch * LT;
    float pw[BPL][4], ww[BPL][4];
#pragma unroll
    for (int q = 0; q < BPL; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) pw[q][r] = ww[q][r] = 0.f;
    const int h2 = p.delta >> 1;
    for (int np = wv; np < N; np += WAVES) {
        if (amask != nullptr && amask[np] == 0) continue;          // (wave-uniform) an unloaded bin transmits nothing
        const float2 *__restrict__ col = cols + ((size_t)pair * N + np) * p.JP;
        for (int j = lane; j < p.J; j += 64) row[24 + j] = ldg2(col + j);
        for (int j = p.J + lane; j < ROWLEN - 24; j += 64) row[24 + j] = mk(0.f, 0.f);
        wave_sync();
        // z = conv(h, u) over three symbol periods: lane -> RB3 consecutive outputs from j0
        v2f acc[RB3];
        const int j0 = lane * RB3;
        fir_lane<RB3, interfm_geo<N>::CH>(row + 24 - (LT - 1) + j0, taps, acc);
        wave_sync();
#pragma unroll
        for (int r = 0; r < RB3; ++r)
            if (j0 + r < 3 * B) row[24 + j0 + r] = acc[r];
        wave_sync();
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            // Rx window, fold, circular shift (m:297-355) of period m, then the DFT
            const v2f *fb = row + 24 + m * B;
            v2f v[1][BPL][4];
#pragma unroll
            for (int q = 0; q < BPL; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    v[0][q][r] = mk(0.f, 0.f);
                    if (!(FULL || lane + 64 * q < NQ)) continue;
                    const int m0 = (lane + 64 * q + r * NQ + p.kap + h2) & (N - 1);
                    v2f z = fb[p.gam + m0] * wrx[m0];
                    if (m0 < p.delta) {
                        const float w2 = wrx[m0 + N];
                        z = __builtin_elementwise_fma(mk(w2, w2), fb[p.gam + m0 + N], z);
                    }
                    v[0][q][r] = z;
                }
            fft_wave<N, -1, 1>(v, scr, 0, tw, lane);
#pragma unroll
            for (int q = 0; q < BPL; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int n = lane + 64 * q + r * NQ;
                    const float e = v[0][q][r].x * v[0][q][r].x + v[0][q][r].y * v[0][q][r].y;
                    if (!(FULL || lane + 64 * q < NQ)) continue;
                    if (m == 0 && n == np) ww[q][r] += e;          // the wanted term A_0[n, n]
                    else pw[q][r] += e;
                }
        }
        wave_sync();
    }
    // sums over the waves in wave order (each wave's row is free now): float [WAVES][N] in the rows area, power then wanted
    float *red = reinterpret_cast<float *>(rows);
    for (int pass = 0; pass < 2; ++pass) {
        float *dst = pass == 0 ? p.power : p.wanted;
        if (dst == nullptr) break;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < BPL; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (FULL || lane + 64 * q < NQ) red[wv * N + lane + 64 * q + r * NQ] = pass == 0 ? pw[q][r] : ww[q][r];
        __syncthreads();
        for (int n = tid; n < N; n += WAVES * 64) {
            float t = 0.f;
            for (int w = 0; w < WAVES; ++w) t += red[w * N + n];
            dst[(size_t)job * N + n] = (amask != nullptr && amask[n] == 0) ? 0.f : t;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Tx PAPR and its histogram, for the frames the BER loop transmits (wofdm_tx_papr; the reference has no PAPR figure).
// Three steps per chunk of frames (wofdm_pparams): the symbol grids of the chunk from the Philox label streams -- what phase A
// of the frame kernel feeds its IDFT --, their waveforms by the waveform kernels above with one job per frame, and {peak,
// energy} of every symbol period of those waveforms with its histogram bin.
//
// Generation: thread = one Philox block of the label stream (stream p.stream of philox.h, 0 unless the caller asks for the
// neighbour's stream 2: counter (s bps + blk, frame lo, frame hi, stream << 28 | pair), key = seed), 256 blocks per workgroup into LDS; they are 256 * 128 / kslot consecutive subcarriers of X, which the
// workgroup then maps (qam_point, zero on unloaded bins) and stores side by side.  The first n_jobs threads of the grid also
// write the chunk's job tables: job j = frame (item0 + j) % frames of pair (item0 + j) / frames.
template <int N>
__global__ void __launch_bounds__(256) wofdm_papr_gen_kernel(const wofdm_pparams p)
{
    __shared__ uint32_t words[256 * 4];
    __shared__ v2f lut[64];
    const int tid = threadIdx.x, S = p.S;
    const int ks = p.k == 6 ? 8 : p.k, bps = N * ks / 128, per = 128 / ks;      // (wofdm_kslot)
    if (tid < (1 << p.k)) lut[tid] = qam_point(p.k, (uint32_t)tid);
    const uint32_t gid = blockIdx.x * 256u + (uint32_t)tid;           // (n_jobs S bps <= 65535 * 17 * 64 < 2^27)
    if (gid < (uint32_t)p.n_jobs) {
        const uint64_t pair = (p.item0 + gid) / p.frames;
        const int T = p.beta + S * (p.P - p.beta);
        wofdm_bjob jb;
        jb.block = (int32_t)gid; jb.cp = p.cp; jb.cs = p.cs; jb.overlap = p.beta;
        jb.w_off = (int32_t)(pair / p.wdiv * (uint64_t)p.P); jb.len = T; jb.item0 = 0; jb.n_items = 0;
        jb.x_off = (int64_t)gid * T;
        p.jobs[gid] = jb;
        if (p.mjobs != nullptr) {
            wofdm_mjob mj;
            mj.job = (int32_t)gid; mj.spec = 0; mj.y_off = (int64_t)gid * S * (2 * p.P - 1);
            p.mjobs[gid] = mj;
        }
    }
    if (gid < (uint32_t)p.n_jobs * (uint32_t)(S * bps)) {
        const uint32_t sym = gid / (uint32_t)bps, blk = gid - sym * (uint32_t)bps;
        const uint32_t j = sym / (uint32_t)S, s = sym - j * (uint32_t)S;
        const uint64_t item = p.item0 + j, pair = item / p.frames, frame = p.frame_offset + (item - pair * p.frames);
        const philox_out o = philox4x32_10(s * (uint32_t)bps + blk, (uint32_t)frame, (uint32_t)(frame >> 32),
                                           (p.stream << 28) | (uint32_t)pair, p.seed_lo, p.seed_hi);
#pragma unroll
        for (int i = 0; i < 4; ++i) words[4 * tid + i] = o.w[i];
    }
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * 256u * (uint32_t)per, total = (uint64_t)p.n_jobs * S * N;
    const uint32_t lmask = (1u << p.k) - 1u;
    for (int i = tid; i < 256 * per; i += 256) {
        const uint64_t e = base + (uint32_t)i;
        if (e >= total) break;
        const uint32_t bit = (uint32_t)i * (uint32_t)ks;
        const uint32_t lab = (words[bit >> 5] >> (bit & 31u)) & lmask;
        v2f v = lut[lab];
        if (p.amask != nullptr && p.amask[e & (uint64_t)(N - 1)] == 0) v = mk(0.f, 0.f);
        p.X[e] = make_float2(v.x, v.y);
    }
}

// Sum / maximum over the 64 lanes of a wave in a fixed order: four DPP steps inside each row of 16 lanes (two quad permutes,
// half-row mirror, row mirror), then the four row totals by lane reads.  The result is wave-uniform.
template <bool MAX> __device__ __forceinline__ float papr_wave_reduce(float v)
{
#define WOFDM_DPP_STEP(ctrl)                                                                                               \
    {                                                                                                                      \
        const float o = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, 0xf, 0xf, false)); \
        v = MAX ? fmaxf(v, o) : v + o;                                                                                     \
    }
    WOFDM_DPP_STEP(0xB1)         // quad_perm [1, 0, 3, 2]
    WOFDM_DPP_STEP(0x4E)         // quad_perm [2, 3, 0, 1]
    WOFDM_DPP_STEP(0x141)        // row_half_mirror
    WOFDM_DPP_STEP(0x140)        // row_mirror
#undef WOFDM_DPP_STEP
    const int b = __builtin_bit_cast(int, v);
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0));
    const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32));
    const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
    return MAX ? fmaxf(fmaxf(r0, r1), fmaxf(r2, r3)) : (r0 + r1) + (r2 + r3);
}

// Periods: period q = (job q / S, symbol q % S) of the chunk is the samples [s B, (s + 1) B) of the job's waveform.  A
// workgroup (16 waves) takes a contiguous run of batches of 256 periods; in a batch wave w reduces the periods 16 w ... 16 w + 15
// one after the other (lanes stride the samples, then papr_wave_reduce) and lane i < 16 keeps {peak, energy} of the i-th, so
// that the bins -- a log10 each -- are formed by 16 lanes of every wave side by side.  Counts go into a workgroup-local histogram in LDS
// (32-bit atomics) that belongs to ONE pair, the pair of the batch's first period; it is flushed to the 64-bit counters in
// global memory (one atomic per non-empty bin) when that pair changes and at the end.  A period of another pair than the
// batch's first -- frames * S no multiple of 256 -- adds to global memory directly.  The largest PAPR travels the same way as
// the bit pattern of a non-negative float under an integer maximum.  Integer counts and a maximum: no result depends on the
// order of the atomics.
#define WOFDM_PAPR_PER_WAVE 16
#define WOFDM_PAPR_WAVES 16
__global__ void __launch_bounds__(WOFDM_PAPR_WAVES * 64) wofdm_papr_period_kernel(const wofdm_pparams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t *lh = reinterpret_cast<uint32_t *>(smem);                // [n_bins] counts | [1] maximum
    constexpr int PW = WOFDM_PAPR_PER_WAVE, NT = WOFDM_PAPR_WAVES * 64, BATCH = WOFDM_PAPR_WAVES * PW;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int S = p.S, B = p.P - p.beta, T = p.beta + S * B, nb = p.n_bins;
    const uint32_t n_per = (uint32_t)p.n_jobs * (uint32_t)S;
    const uint32_t n_batches = (n_per + BATCH - 1) / BATCH, per_wg = (n_batches + gridDim.x - 1) / gridDim.x;
    const uint32_t b0 = blockIdx.x * per_wg, b1 = min(n_batches, b0 + per_wg);
    for (int i = tid; i <= nb; i += NT) lh[i] = 0u;
    __syncthreads();
    auto flush = [&](uint64_t pair) {                                 // (called by the whole workgroup)
        __syncthreads();
        for (int i = tid; i < nb; i += NT) {
            const uint32_t c = lh[i];
            if (c != 0u) {
                atomicAdd(&p.hist[pair * (uint64_t)nb + (uint32_t)i], (unsigned long long)c);
                lh[i] = 0u;
            }
        }
        if (tid == 0) {
            atomicMax(&p.max_bits[pair], lh[nb]);
            lh[nb] = 0u;
        }
        __syncthreads();
    };
    bool have = false;
    uint64_t cur = 0;
    for (uint32_t b = b0; b < b1; ++b) {
        const uint32_t q0 = b * BATCH;
        const uint64_t pair0 = (p.item0 + q0 / (uint32_t)S) / p.frames;
        if (have && pair0 != cur) flush(cur);
        cur = pair0;
        have = true;
        float pk = 0.f, en = 0.f;
        for (int i = 0; i < PW; ++i) {
            const uint32_t q = q0 + (uint32_t)(wv * PW + i);
            if (q >= n_per) break;                                    // (wave-uniform)
            const uint32_t j = q / (uint32_t)S, s = q - j * (uint32_t)S;
            const float2 *__restrict__ src = p.x + (size_t)j * T + (size_t)s * B;
            float m = 0.f, e = 0.f;
            for (int t = lane; t < B; t += 64) {
                const float2 v = src[t];
                const float a = v.x * v.x + v.y * v.y;
                m = fmaxf(m, a);
                e += a;
            }
            m = papr_wave_reduce<true>(m);
            e = papr_wave_reduce<false>(e);
            if (lane == i) {
                pk = m;
                en = e;
            }
        }
        const uint32_t q = q0 + (uint32_t)(wv * PW + lane);
        if (lane < PW && q < n_per) {
            const uint64_t item = p.item0 + q / (uint32_t)S, pair = item / p.frames;
            if (p.periods != nullptr) p.periods[item * (uint64_t)S + q % (uint32_t)S] = make_float2(pk, en);
            // PAPR = B peak / energy; bin = clamp(floor((10 log10 PAPR - lo) / step)); no energy: PAPR 0, bin 0
            const float papr = en > 0.f ? (float)B * pk / en : 0.f;
            const double t = papr > 0.f ? (10.0 * log10((double)papr) - (double)p.lo_db) / (double)p.step_db : -1.0;
            const int bin = t >= (double)nb ? nb - 1 : (t > 0.0 ? (int)t : 0);
            const uint32_t bits = __builtin_bit_cast(uint32_t, papr);
            if (pair == cur) {
                atomicAdd(&lh[bin], 1u);
                atomicMax(&lh[nb], bits);
            } else {
                atomicAdd(&p.hist[pair * (uint64_t)nb + (uint32_t)bin], 1ull);
                atomicMax(&p.max_bits[pair], bits);
            }
        }
    }
    if (have) flush(cur);
}

// ---------------------------------------------------------------------------------------------
// Per-subcarrier BER and EVM of the frames the BER loop runs (wofdm_rx_profile and its six arms _aci, _sync, _doppler, _pa, _pn,
// _link: one body, rxprof_body<N, ARM> below, whose comment says what each arm adds): a second, unfused implementation of the
// whole frame pipeline behind the Tx chain above,
//   conv, add_wgn, truncate        matlab/main_BER_calculation.m:260-261, 277-294
//   wofdm_rx                       main_BER_calculation.m:297-355 (Rx window, fold, circular shift, DFT)
//   LS estimate, equaliser, slicer main_BER_calculation.m:266-272
// (the semantics of the CPU checker's frame).  The chunk's items are (cell, frame) here: every cell draws its own
// labels, so the generation kernel runs with wdiv = n_snr n_channels cells per window pair.
//
// One workgroup per item.  Pass 1: Ps = sum |conv|^2 and Pn = sum |unit noise|^2 over the same NL samples (thread-strided
// partials, the wave sum of papr_wave_reduce, the waves in order: a fixed order), g = sqrt(Ps 10^(-snr/10) / Pn).  Pass 2: a
// wave per symbol, symbols wave, wave + W, ...: the N + delta + 20 samples of x under the symbol's receive window go into the
// wave's LDS row, every lane forms the received samples of its DFT inputs from them -- the 21-tap sum and the unit normal of
// that sample (stream 1 of philox.h, one block per sample: half of each block is drawn twice, which keeps the frame out of
// LDS) --, windows, folds and shifts them (literally, as the reference does), and the wave transforms its row: radix-2,
// decimation in time over bit-reversed stores, plain fp32 complex arithmetic -- not the transform of the frame kernels.
// Wave 0 publishes the pilot equaliser X0 / Y0 behind the first round's barrier; every lane keeps the counters of its bins
// n = lane + 64 j in registers over the wave's symbols.  The waves' sums are added in wave order into the item's partials
// part_pow[job][N] (fp32) and part_cnt[job][N] (bit errors | symbol errors << 16), and wofdm_rxprof_reduce_kernel adds a
// cell's items in frame order (fp64) onto the call's totals: no float atomics anywhere, repeated calls give identical bits.
// LDS does not grow with S or cp + cs: twiddles [N / 2] | G [N] | w_rx [N + 64] | 64 floats | per wave: row [N] + x [N + 88].
template <int N> struct rxp_geo {
    static constexpr int WAVES = N >= 1024 ? 4 : 8, BINS = N / 64;
    static constexpr int LOG2 = N == 64 ? 6 : (N == 128 ? 7 : (N == 256 ? 8 : (N == 512 ? 9 : 10)));
    static constexpr int XROW = N + 64 + 24;                          // tail_rx <= 64, WOFDM_LT - 1 <= 24 samples of history
    static constexpr int LDS = 8 * (N / 2) + 8 * N + 4 * (N + 64) + 4 * 64 + WAVES * 8 * (N + XROW);
    static constexpr int LDS_ACI = LDS + WAVES * 8 * XROW;            // the ACI arm: a second x row per wave (the neighbour's)
    static_assert(LDS <= 160 * 1024 && WAVES * 8 * N <= WAVES * 8 * (N + XROW) && (1 << LOG2) == N, "LDS");
    static_assert(LDS_ACI <= 160 * 1024, "LDS (ACI arm)");
    static constexpr int LDS_DOP = LDS + 8 * WOFDM_DOPPLER_KNOTS * WOFDM_LT;   // the moving channel: a track's knots [64][21] float2
    static_assert(LDS_DOP <= 160 * 1024 && LDS % 8 == 0, "LDS (moving channel)");
    // the link arm: the neighbour's row and the knots (75 776 B at N = 256, 129 024 B at N = 512, 131 584 B at N = 1024)
    static constexpr int LDS_LINK = LDS + WAVES * 8 * XROW + 8 * WOFDM_DOPPLER_KNOTS * WOFDM_LT;
    static_assert(LDS_LINK <= 160 * 1024, "LDS (link arm)");
    // the tracking receiver: one more float2 [N], HL (139 776 B at N = 1024)
    static constexpr int LDS_TRACK = LDS_LINK + 8 * N;
    static_assert(LDS_TRACK <= 160 * 1024, "LDS (tracking receiver)");
};

// the complex unit normal of sample a of (seed, cell, frame): philox.h, block a / 2, words 2 (a % 2) and 2 (a % 2) + 1
__device__ __forceinline__ v2f rxp_noise(uint32_t a, uint32_t f_lo, uint32_t f_hi, uint32_t cell, uint32_t k0, uint32_t k1, int which)
{
    const philox_out o = philox4x32_10(a, f_lo, f_hi, (WOFDM_STREAM_NOISE << 28) | cell, k0, k1);
    const uint32_t wa = which ? o.w[2] : o.w[0], wb = which ? o.w[3] : o.w[1];
    const float u1 = fmaf((float)wa, 2.3283064365386963e-10f, 1.1641532182693481e-10f);
    const float u2 = (float)(wb >> 9) * 1.1920928955078125e-07f;
    const float rad = sqrtf(-2.0f * logf(u1));
    float sv, cv;
    sincospif(2.0f * u2, &sv, &cv);
    return mk(rad * cv, rad * sv);
}
// The four phase-walk increments of Philox block b of (seed, cell, frame): philox.h, stream 3 -- the complex unit normals
// 2 b (words 0, 1) and 2 b + 1 (words 2, 3), real then imaginary part, are the increments of the on-air indices 4 b ... 4 b + 3.
// u1 and u2 are rxp_noise's, formed in single precision (exact values: a 32-bit word times 2^-32 plus 2^-33 rounded once,
// 23 bits times 2^-23); the Box-Muller step is in double precision.
__device__ __forceinline__ void pn_increments(uint32_t b, uint32_t f_lo, uint32_t f_hi, uint32_t cell, uint32_t k0, uint32_t k1, double xi[4])
{
    const philox_out o = philox4x32_10(b, f_lo, f_hi, (WOFDM_STREAM_PN << 28) | cell, k0, k1);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const float u1 = fmaf((float)o.w[2 * e], 2.3283064365386963e-10f, 1.1641532182693481e-10f);
        const float u2 = (float)(o.w[2 * e + 1] >> 9) * 1.1920928955078125e-07f;
        const double rad = sqrt(-2.0 * log((double)u1));
        double sv, cv;
        sincospi(2.0 * (double)u2, &sv, &cv);
        xi[2 * e] = rad * cv;
        xi[2 * e + 1] = rad * sv;
    }
}
// sum over the 64 lanes of a wave in double precision, in a fixed order: the butterfly over lane distances 1, 2, 4, ... 32
// (both partners form the same sum, addition being commutative, so the result is wave-uniform to the bit)
__device__ __forceinline__ double pn_wave_sum(double v)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The unit phase walks of wofdm_rx_profile_pn (wofdm_pnparams): one workgroup of 1024 threads per (cell, frame) item of the
// chunk, walk[job][a] = xi[0] + ... + xi[a] for a < len = S B, in double precision.  Thread t owns the run
// [t R, (t + 1) R) of on-air indices, R = 4 ceil(len / 4096): whole Philox blocks, each drawn once.  The order of additions is
// fixed:
//   1. the thread writes its increments to walk[] and adds them up, ascending from 0.0: its total;
//   2. the exclusive prefix of the totals: inside a wave the inclusive scan over lane distances 1, 2, 4, ... 32 (a lane adds
//      the partial sum of the lane that distance below it, where there is one); "lanes before" is the scan of the lane
//      below, 0.0 for lane 0; "waves before" is the sum of the earlier waves' totals (lane 63's scan, through LDS), added
//      in wave order from 0.0; prefix = (waves before) + (lanes before);
//   3. the thread reads its increments back and adds them one by one onto its prefix, ascending; every partial sum is u[a].
// rx_profile.pn_walk (a numpy cumsum in double) differs from it by the order of the additions only.
__global__ void __launch_bounds__(1024) wofdm_pn_walk_kernel(double *__restrict__ walk, int len, uint32_t seed_lo, uint32_t seed_hi,
                                                             uint64_t item0, uint64_t frames, uint64_t frame_offset)
{
    __shared__ double wtot[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint64_t item = item0 + blockIdx.x, cell64 = item / frames, frame = frame_offset + (item - cell64 * frames);
    const uint32_t cell = (uint32_t)cell64, f_lo = (uint32_t)frame, f_hi = (uint32_t)(frame >> 32);
    double *__restrict__ u = walk + (size_t)blockIdx.x * (size_t)len;
    const int R = 4 * ((len + 4095) / 4096), lo = tid * R, hi = lo + R < len ? lo + R : len;
    double tot = 0.0;
    for (int j = lo; j < hi; j += 4) {
        double xi[4];
        pn_increments((uint32_t)(j >> 2), f_lo, f_hi, cell, seed_lo, seed_hi, xi);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (j + e < hi) {
                u[j + e] = xi[e];
                tot += xi[e];
            }
    }
    double inc = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double below = __shfl_up(inc, o, 64);
        if (lane >= o) inc += below;
    }
    if (lane == 63) wtot[wv] = inc;
    double lanes_before = __shfl_up(inc, 1, 64);
    if (lane == 0) lanes_before = 0.0;
    __syncthreads();
    double waves_before = 0.0;
    for (int w = 0; w < wv; ++w) waves_before += wtot[w];
    double acc = waves_before + lanes_before;
    for (int j = lo; j < hi; ++j) {
        acc += u[j];
        u[j] = acc;
    }
}

// qamdemod, hard decision (main_BER_calculation.m:269-270): MATLAB Gray label of the nearest point
__device__ __forceinline__ uint32_t rxp_slice(int k, float re, float im)
{
    const int hb = k >> 1, mm = (1 << hb) - 1;
    const float a = k == 2 ? 1.4142135623730951f : (k == 4 ? 3.1622776601683795f : 6.4807406984078604f);
    int ii = (int)floorf((re * a + (float)mm) * 0.5f + 0.5f), qi = (int)floorf(((float)mm - im * a) * 0.5f + 0.5f);
    ii = ii < 0 ? 0 : (ii > mm ? mm : ii);
    qi = qi < 0 ? 0 : (qi > mm ? mm : qi);
    return ((uint32_t)(ii ^ (ii >> 1)) << hb) | (uint32_t)(qi ^ (qi >> 1));
}

// The knot interval of the on-air index a (wofdm_dparams): q = min(a / step, last), last = n_knots - 2, and the fraction
// f = (a - q step) / step.  The quotient comes from the single-precision reciprocal rstep = 1 / step and two corrections, not
// from a 32-bit division per sample: a < 2^22 is exact in single precision and the product carries under 3 2^-24 of a / step
// < 2^22, so its integer part is off by one at most.  The knots cover the frame, so only a = (last + 1) step meets the
// clamp, with f = 1.
__device__ __forceinline__ void dop_interval(uint32_t a, uint32_t step, float rstep, uint32_t last, uint32_t &q, float &f)
{
    uint32_t qq = (uint32_t)((float)a * rstep);
    int32_t r = (int32_t)(a - qq * step);
    if (r < 0) {
        --qq;
        r += (int32_t)step;
    }
    if (r >= (int32_t)step) {
        ++qq;
        r -= (int32_t)step;
    }
    if (qq > last) {
        r += (int32_t)((qq - last) * step);
        qq = last;
    }
    q = qq;
    f = (float)r * rstep;
}

// One tap of the 21-tap sum, cr += hv.x xv.x - hv.y xv.y and ci += hv.x xv.y + hv.y xv.x, for every arm and both passes.  The
// operations are written down: they are the ones the compiler once formed for these statements in the plain kernel, the first
// product of each line fused onto the rounded second, then the addition -- but in the copy of rxs() for the folded sample
// m0 + N (FOLD) the imaginary part has the second product fused onto the rounded first.  Left to itself the compiler chooses
// its fusions anew in every inlined copy (other ones still where the taps are per lane), and the arms' identities with the
// plain call -- an offset-free point, a static track, a linear amplifier -- would hang on its mood.  The real part is formed
// as cr - fma(-hv.x, xv.x, hv.y xv.y): the same value, rounding being symmetric, and the instructions the plain kernel had
// (a plain multiply and an fma with a negated source; with the negation on the product the plain call ran 0.3 % longer).
template <bool FOLD>
__device__ __forceinline__ void fir_tap(const float2 hv, const float2 xv, float &cr, float &ci)
{
#pragma clang fp contract(off)
    const float nre = __builtin_fmaf(-hv.x, xv.x, hv.y * xv.y);
    const float im = FOLD ? __builtin_fmaf(hv.y, xv.x, hv.x * xv.y) : __builtin_fmaf(hv.x, xv.y, hv.y * xv.x);
    cr = cr - nre;
    ci = ci + im;
}

// One tap of the neighbour's 21-tap sum in the link arm, ar += hv.x xv.x - hv.y xv.y and ai += hv.x xv.y + hv.y xv.x, written
// down like fir_tap and for the same reason: these are the operations the compiler forms today for the ACI arm's statements in
// wofdm_rxprof_aci_kernel, at every N (read from its assembly) -- the first product of the real part fused onto the rounded
// second; of the imaginary part the first product fused in the copy of rxs() for m0, the second in the copy for the folded
// sample m0 + N --, whereas in the link arm's copy for m0 + N it fused the first: wofdm_rx_profile_link's neighbour-only point
// then missed wofdm_rx_profile_aci's bytes wherever the Rx window has a tail.  The ACI arm keeps its statements: written down
// like this its kernel computes the same values but is scheduled differently (the negation moves from the fma's addend into
// the product), and the six earlier kernels are to come out instruction for instruction.
template <bool FOLD>
__device__ __forceinline__ void aci_tap(const float2 hv, const float2 xv, float &ar, float &ai)
{
#pragma clang fp contract(off)
    const float re = __builtin_fmaf(hv.x, xv.x, -(hv.y * xv.y));
    const float im = FOLD ? __builtin_fmaf(hv.y, xv.x, hv.x * xv.y) : __builtin_fmaf(hv.x, xv.y, hv.y * xv.x);
    ar = ar + re;
    ai = ai + im;
}

// log2(1 + x) for 0 <= x <= 1 with the hardware logarithm: below 2^-6 the rounding of 1 + x would cost 2^-24 / x of the
// result, and the series x log2(e) (1 - x / 2 + x^2 / 3) is good to x^3 / 4 <= 2^-20 there; above, 1 + x carries 2^-18 at most.
__device__ __forceinline__ float soft_log2_1p(float x)
{
    const float ser = x * 1.4426950408889634f * __builtin_fmaf(x, __builtin_fmaf(x, 0.33333333f, -0.5f), 1.0f);
    return x < 0.015625f ? ser : __builtin_amdgcn_logf(1.0f + x);
}

// The demapper of wofdm_rxprof_soft_kernel (wofdm_softparams, wofdm_link.h) for the wave's data symbol s >= 1: row = the symbol's
// DFT outputs, G the point's pilot equaliser, Xs the transmitted points, vw = v W2.  Per loaded bin n = lane + 64 j, j ascending:
//   e = G[n] row[n], rn = 1 / (a^2 |G[n]|^2 vw), a the constellation's scale (levels 2 l - (m - 1) over a per axis, m = 2^(k/2));
//   per axis and bit position of the axis' Gray index the smallest squared distance, in level units, to a level whose bit is 1
//   and to one whose bit is 0 -- the other axis' distance is common to both minima and cancels in their difference --, so
//   z_i = (1 - 2 b_i) Lambda_i = (1 - 2 b_i) (min1 - min0) rn, i = 0 the top bit of the label (the I axis' top bit), b_i the
//   transmitted bit (the label of Xs as rxp_slice reads it);
//   per scale j: pen_j = sum_i [max(-t, 0) + log2(1 + 2^-|t|)], t = cs[j] z_i, i ascending, with v_exp_f32 / v_log_f32.
// pen_j goes to bit_part[slot][s - 1][j][n] (0 on an unloaded bin: every element of the symbol's rows is written), the lane's
// sum over its bins, then the wave's (papr_wave_reduce), to sym_part[slot][j][s].  The bins' loop is not unrolled -- 16 scales
// times 6 bits of exp2 / log2 pairs are code enough once -- and the scales' loop is, so that the lane's sums stay in registers.
// TRACK (wofdm_rxprof_tracking_kernel): pil, the comb, or null -- a pilot bin is written as an unloaded one is, 0 --, and G is
// whatever equaliser the point's receiver formed for this symbol, e = G row and nu = |G|^2 vw as above.
// CODED (wofdm_rxprof_coded_kernel): beside the penalties the bin's soft bits d_i = clamp(rint(llr z_i), -127, 127), round half
// even, NaN -> 0, 0 where the bin takes no decision, as ONE 8-byte store to sb[slot][s - 1][n][8] (bytes k ... 7 are 0).
template <int N, bool TRACK = false, bool CODED = false>
__device__ __forceinline__ void soft_symbol(const wofdm_rparams &p, const wofdm_softparams &so, const float2 *row, const float2 *G,
                                            const float2 *__restrict__ Xs, float vw, size_t slot, int s, int lane,
                                            [[maybe_unused]] const uint8_t *__restrict__ pil = nullptr,
                                            [[maybe_unused]] float llr = 0.f, [[maybe_unused]] int8_t *__restrict__ sb = nullptr)
{
    constexpr int BINS = N / 64, SC = WOFDM_SOFT_SCALES;
    const int k = p.k, hb = k >> 1, mm = (1 << hb) - 1, nsc = so.n_scales, S = p.S;
    const float a = k == 2 ? 1.4142135623730951f : (k == 4 ? 3.1622776601683795f : 6.4807406984078604f);
    float *__restrict__ bp = so.bit_part + (slot * (size_t)(S - 1) + (size_t)(s - 1)) * (size_t)nsc * N;
    float ssum[SC];
#pragma unroll
    for (int j = 0; j < SC; ++j) ssum[j] = 0.f;
#pragma unroll 1
    for (int j = 0; j < BINS; ++j) {
        const int n = lane + 64 * j;
        bool on = p.amask == nullptr || p.amask[n] != 0;
        if constexpr (TRACK) on = on && (pil == nullptr || pil[n] == 0);
        const float2 y = row[n], gq = G[n], xs = Xs[n];
        const float er = y.x * gq.x - y.y * gq.y, ei = y.x * gq.y + y.y * gq.x;
        const float rn = 1.0f / (a * a * (gq.x * gq.x + gq.y * gq.y) * vw);
        const uint32_t lab = rxp_slice(k, xs.x, xs.y);
        // z[i], i = 0 ... k - 1: the I axis' bits from its top one, then the Q axis'
        float z[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ax = 0; ax < 2; ++ax) {
            const float u = ax == 0 ? er * a : -ei * a;               // level units: the levels are 2 l - mm, l = 0 ... mm
            float m0[3], m1[3];
#pragma unroll
            for (int b = 0; b < 3; ++b) m0[b] = m1[b] = 3.0e38f;
#pragma unroll
            for (int l = 0; l < 8; ++l) {
                if (l <= mm) {
                    const float t = u - (float)(2 * l - mm), d = t * t;
                    const int gry = l ^ (l >> 1);
#pragma unroll
                    for (int b = 0; b < 3; ++b) {
                        if ((gry >> b) & 1)
                            m1[b] = fminf(m1[b], d);
                        else
                            m0[b] = fminf(m0[b], d);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                // bit i of the axis from the top: position hb - 1 - i of the Gray index, hb - 1 - i + (I axis: hb) of the label
                float lam = 0.f;
                uint32_t bit = 0u;
#pragma unroll
                for (int b = 0; b < 3; ++b)
                    if (b == hb - 1 - i) {
                        lam = (m1[b] - m0[b]) * rn;
                        bit = (lab >> (ax == 0 ? b + hb : b)) & 1u;
                    }
                const float zz = bit ? -lam : lam;
#pragma unroll
                for (int q = 0; q < 6; ++q)
                    if (q == ax * hb + i && i < hb) z[q] = zz;
            }
        }
        if constexpr (CODED) {
            uint32_t w[2] = {0u, 0u};
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const float t = llr * z[i];                           // (z[i] = 0 for i >= k)
                const int d = t != t ? 0 : (int)__builtin_rintf(fminf(fmaxf(t, -127.f), 127.f));
                w[i >> 2] |= ((uint32_t)d & 0xFFu) << (8 * (i & 3));
            }
            uint2 *dst = reinterpret_cast<uint2 *>(sb + ((slot * (size_t)(S - 1) + (size_t)(s - 1)) * N + (size_t)n) * 8);
            *dst = on ? make_uint2(w[0], w[1]) : make_uint2(0u, 0u);
        }
#pragma unroll
        for (int c = 0; c < SC; ++c) {
            if (c < nsc) {
                const float cs = so.cs[c];
                float pen = 0.f;
#pragma unroll
                for (int i = 0; i < 6; ++i)
                    if (i < k) {
                        const float t = cs * z[i];
                        pen += fmaxf(-t, 0.f) + soft_log2_1p(__builtin_amdgcn_exp2f(-fabsf(t)));
                    }
                pen = on ? pen : 0.f;
                bp[(size_t)c * N + n] = pen;
                ssum[c] += pen;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < SC; ++c) {
        if (c < nsc) {
            const float t = papr_wave_reduce<false>(ssum[c]);
            if (lane == 0) so.sym_part[(slot * (size_t)nsc + (size_t)c) * (size_t)S + (size_t)s] = t;
        }
    }
}

// The scratch of a symbol that counts nothing (the postamble of a tracking point): the zeros soft_symbol would write on a
// symbol without a loaded bin, for wofdm_rxprof_soft_frame_kernel and the symbols' sums to add
template <int N>
__device__ __forceinline__ void soft_symbol_zero(const wofdm_softparams &so, int S, size_t slot, int s, int lane)
{
    const int nsc = so.n_scales;
    float *__restrict__ bp = so.bit_part + (slot * (size_t)(S - 1) + (size_t)(s - 1)) * (size_t)nsc * N;
    for (int i = lane; i < nsc * N; i += 64) bp[i] = 0.f;
    if (lane < nsc) so.sym_part[(slot * (size_t)nsc + (size_t)lane) * (size_t)S + (size_t)s] = 0.f;
}
// (CODED) and its soft bits: the zeros of a symbol that holds no codeword
template <int N>
__device__ __forceinline__ void coded_symbol_zero(int8_t *__restrict__ sb, int S, size_t slot, int s, int lane)
{
    uint2 *dst = reinterpret_cast<uint2 *>(sb + (slot * (size_t)(S - 1) + (size_t)(s - 1)) * (size_t)N * 8);
    for (int n = lane; n < N; n += 64) dst[n] = make_uint2(0u, 0u);
}

// The one body of the seven receive kernels; ARM selects at compile time what an arm adds to the pipeline above, and the
// parameters of the other arms are not read.
//   RXP_PLAIN    wofdm_rx_profile: nothing.
//   RXP_ACI      wofdm_rx_profile_aci: the wave stages a second row with the neighbour's samples under the same window -- the
//                victim's on-air sample t carries a_lvl xi[t + ioff], zero outside xi --, and rxs() adds their 21-tap sum with
//                the neighbour's channel hi[ch], scaled by a_lvl.  Pass 1 does not see the neighbour.  LDS: LDS_ACI.
//   RXP_SYNC     wofdm_rx_profile_sync: pass 2 once per point of sp.  The windows begin at s B + gam + theta (reads outside
//                [0, T) of x are zero, the noise of sample a is that of counter word (uint32) a: a negative a lands on words
//                no frame uses), and the received sample m under the window, signal and noise, is multiplied by
//                base[point][s] e^{2 pi i eps m / N} -- the host's base phasor carries the phase at the window's start (1 when
//                the common phase is tracked), the kernel forms the in-window factor from the fraction of eps m / N.  At
//                theta = 0, eps = 0 both factors are exactly 1: the point gives the plain kernel's bits.
//   RXP_DOPPLER  wofdm_rx_profile_doppler: both passes once per track of dp (sp.n_points tracks).  The workgroup stages the
//                knots of (track, the item's channel) behind the waves' rows, [n_knots][WOFDM_LT] float2, and every sample of
//                either pass forms its 21 taps from the two knots around its own on-air index, hv = K[q] + f (K[q + 1] - K[q])
//                -- the tap at the OUTPUT sample's time; with equal knots hv is the knot, bit for bit, so a static track gives
//                the plain kernel's bits.  Lanes of a wave sit on neighbouring samples, so their knot reads are broadcasts but
//                for the lanes astride a knot.  LDS: LDS_DOP.
//   RXP_PA       wofdm_rx_profile_pa: both passes once per point of pa (sp.n_points points) on the point's waveform,
//                y[job][point] of wofdm_pa_wave_kernel, or x itself for a linear point, which so gives the plain kernel's bits.
//   RXP_PN       wofdm_rx_profile_pn: pass 2 once per point of pn (sp.n_points points).  The received sample m of symbol s,
//                signal and noise, is multiplied by e^{2 pi i t}, t the fraction of turn (u[a0 + m] - c) in double precision
//                (t -= rint(t)), rounded to single for sincospif(2 t): u the item's unit walk (wofdm_pn_walk_kernel, read
//                from global memory: LDS does not grow), turn = sigma / (2 pi) the point's, c = 0 for a free-running
//                oscillator and, where the common phase error is tracked, the mean of u over the N + delta samples under
//                the symbol's window, formed in double as u[a0] + (sum of u[a0 + m] - u[a0]) / (N + delta) -- a lane's
//                samples m = lane, lane + 64, ... ascending, then pn_wave_sum.  |t| <= 1/2, so the rounding to single
//                costs at most 2^-26 of a turn, 1e-7 rad, and sincospif some 1e-7 more: the rotation is good to about
//                2e-7 rad for every beta and N, where the sync arm's in-window factor carries the rounding of eps m / N
//                in single precision (which is what limits |cfo| there; no such limit here).  At beta = 0 turn = 0, t = 0
//                exactly and the factor is exactly 1 under either flag: the point gives the plain kernel's bits.
//   RXP_LINK     wofdm_rx_profile_link: every stage above at once, per point of lk (sp.n_points points; wofdm_link.h) -- each
//                compile-time flag is "its arm or RXP_LINK".  Both passes run once per point on the point's waveform (pa) with
//                the taps of the point's track (dp: the static channel is one more track, h at every knot, so there is one tap
//                path); where the point's neighbour is on the air (wave-uniform) its row is staged with the point's offset and
//                added with the point's amplitude; the windows begin at s B + gam + theta; the received sample is multiplied by
//                the sync arm's factor (sp) and then by the phase noise's (pn), two multiplies, each exactly (1, 0) when neutral.
//                Under a timing offset the walk is read at clamp(a, 0, S B - 1) -- the oscillator holds its phase outside the
//                frame; at theta = 0 the clamp is never met --, the tracked mean over the same clamped values, and a sample
//                before the frame (a < 0: every product is zero) takes its taps at time 0.  LDS: LDS_LINK.
//   SOFT         (RXP_LINK only: wofdm_rx_profile_soft) behind pass 1 the point's v W2, and behind the hard decisions of every data
//                symbol the demapper soft_symbol above; with the flag false no statement of the body changes.
//   TRACK        (SOFT only: wofdm_rx_profile_tracking) per point the flags cpe and post of tk (wave-uniform).  A point with neither
//                runs the statements above, G = X0 / Y0 and the soft kernel's symbol-to-wave assignment; pilot bins of the comb
//                count nothing.  A point with either keeps H0 = Y0 / X0 in G's place.  With post the waves visit the symbols in
//                the order 0, S - 1, 1, 2, ... S - 2 over the same rounds, so that behind the first round's barrier wave 0
//                publishes H0 and wave 1 HL = Y_{S-1} / X_{S-1} (hl, one more float2 [N] behind the knots: LDS_TRACK); wave 0
//                then forms cL = sum_n HL[n] conj(H0[n]) -- a lane's bins ascending (an unloaded bin adds an exact zero), then
//                papr_wave_reduce on either component --, rho = cL / |cL| (1 where cL = 0), leaves rho in red[2 W], turns hl into
//                HL conj(rho) - H0, and one more barrier follows.  The wave of a data symbol s forms, with t = s / (S - 1),
//                Hh[n] = H0[n] + t hl[n] (post) or H0[n]; the phase q -- cpe: c = sum over the comb of Y_s[p] conj(Hh[p] X_s[p]), a
//                lane's pilot bins ascending, then papr_wave_reduce, q = c / |c| (1 where c = 0); post alone: e^{i t arg rho} --;
//                and the symbol's equaliser conj(q) conj(Hh) / |Hh|^2 per bin in its own x row, free behind the transform, which
//                the slicer's loop and the demapper then read in G's place: one e for both.  The postamble's wave counts
//                nothing and writes the zeros of its symbol.  With the flag false no statement of the body changes.
// The arms with a point loop (points, tracks) write the partials part_pow, part_cnt [job][point][N], and the wave of symbol
// s >= 1 leaves beside them the symbol's sums over the loaded bins -- a lane's bins ascending, then papr_wave_reduce -- in
// sym_pow, sym_cnt [job][point][S].  The pilot of a point sees what the point's data sees.  Where pass 1 runs per point, Ps
// is the point's; Pn depends on neither channel nor waveform and is measured with the first.
template <int N, int ARM, bool SOFT = false, bool TRACK = false, bool CODED = false>
__device__ __forceinline__ void rxprof_body(const wofdm_rparams &p, const wofdm_aparams &ap, const wofdm_sparams &sp,
                                            const wofdm_dparams &dp, const wofdm_paparams &pa, const wofdm_pnparams &pn,
                                            const wofdm_lparams &lk, [[maybe_unused]] const wofdm_softparams &so = wofdm_softparams{},
                                            [[maybe_unused]] const wofdm_trackparams &tk = wofdm_trackparams{},
                                            [[maybe_unused]] const wofdm_codeparams &cd = wofdm_codeparams{})
{
    static_assert(!SOFT || ARM == RXP_LINK, "the demapper is instantiated for the link arm only");
    static_assert(!TRACK || SOFT, "the tracking receiver is instantiated with the demapper only");
    static_assert(!CODED || TRACK, "the soft-bit stores are instantiated with the tracking receiver only");
    using RG = rxp_geo<N>;
    constexpr bool LINK = ARM == RXP_LINK;
    constexpr bool ACI = ARM == RXP_ACI || LINK, SYNC = ARM == RXP_SYNC || LINK, DOP = ARM == RXP_DOPPLER || LINK;
    constexpr bool PA = ARM == RXP_PA || LINK, PN = ARM == RXP_PN || LINK;
    constexpr bool POINTS = SYNC || DOP || PA || PN, PASS1_PER_POINT = DOP || PA;
    constexpr int ROWLEN = N + (ACI ? 2 : 1) * RG::XROW;
    constexpr int W = RG::WAVES, NT = W * 64, LT = WOFDM_LT, BINS = RG::BINS, LOG2 = RG::LOG2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *tw = reinterpret_cast<float2 *>(smem);                    // e^{-2 pi i k / N}, k < N / 2
    float2 *G = tw + N / 2;                                           // pilot equaliser X0 / Y0 (of the point)
    float *wrx = reinterpret_cast<float *>(G + N);
    float *red = wrx + N + 64;                                        // [2][W] power partials
    float2 *rows = reinterpret_cast<float2 *>(red + 64);
    [[maybe_unused]] float2 *kn = rows + (size_t)W * ROWLEN;          // (DOP) [n_knots][LT] knots of the track, the item's channel
    [[maybe_unused]] float2 *hl = kn + WOFDM_DOPPLER_KNOTS * LT;      // (TRACK) [N] HL, then HL conj(rho) - H0
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int S = p.S, B = p.B, T = p.T, NL = p.NL, delta = p.delta, NP = POINTS ? sp.n_points : 1;
    const uint32_t job = blockIdx.x;
    const uint64_t item = p.item0 + job, cell64 = item / p.frames, frame = p.frame_offset + (item - cell64 * p.frames);
    const uint32_t cell = (uint32_t)cell64, f_lo = (uint32_t)frame, f_hi = (uint32_t)(frame >> 32);
    const int ch = (int)(cell % (uint32_t)p.n_ch), sn = (int)((cell / (uint32_t)p.n_ch) % (uint32_t)p.n_snr);
    const int pair = (int)(cell / ((uint32_t)p.n_ch * (uint32_t)p.n_snr));
    const float2 *__restrict__ Xg = p.X + (size_t)job * S * N;
    const float2 *__restrict__ taps = p.h + (size_t)ch * LT;
    const float2 *__restrict__ xi = ACI ? ap.xi + (size_t)job * ap.Ti : nullptr;
    const float2 *__restrict__ itaps = ACI ? ap.hi + (size_t)ch * LT : nullptr;
    [[maybe_unused]] const double *__restrict__ walk = PN ? pn.walk + (size_t)job * (size_t)(S * B) : nullptr;
    [[maybe_unused]] const int walk_last = S * B - 1;                 // (LINK) the oscillator holds its phase outside the frame
    for (int i = tid; i < N / 2; i += NT) {
        float sv, cv;
        sincospif(-2.0f * (float)i / (float)N, &sv, &cv);
        tw[i] = make_float2(cv, sv);
    }
    for (int i = tid; i < N + delta; i += NT) wrx[i] = p.wrx[(size_t)pair * (N + delta) + i];
    // the 21 taps at the on-air index a: the channel's own, wave-uniform, or (DOP) a lane's, between the knots around a
    const uint32_t kstep = (uint32_t)dp.knot_step, klast = (uint32_t)(dp.n_knots - 2);
    const float rstep = 1.0f / (float)kstep;
    auto taps_at = [&]([[maybe_unused]] uint32_t a) {
        if constexpr (DOP) {
            uint32_t kq;
            float kf;
            dop_interval(a, kstep, rstep, klast, kq, kf);
            const float2 *k0 = kn + kq * LT;
            return [=](int l) {
                const float2 ka = k0[l], kb = k0[LT + l];
                return make_float2(ka.x + kf * (kb.x - ka.x), ka.y + kf * (kb.y - ka.y));
            };
        } else {
            return [=](int l) { return taps[l]; };
        }
    };
    // pass 1: signal and noise power over the same NL samples (add_wgn, m:277-294), the noise power only where `first`; a
    // thread takes whole Philox blocks.  Gives the noise gain g.
    auto pass1 = [&](const float2 *__restrict__ x, bool first) {
        float ps = 0.f, pn = 0.f;
        for (int q = tid; 2 * q < NL; q += NT) {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int jj = 2 * q + e;
                if (jj >= NL) break;
                const auto tap = taps_at((uint32_t)jj);
                float cr = 0.f, ci = 0.f;
                for (int l = 0; l < LT; ++l) {
                    const int t = jj - l;
                    if (t < 0 || t >= T) continue;
                    fir_tap<false>(tap(l), x[t], cr, ci);
                }
                ps += __builtin_fmaf(ci, ci, cr * cr);                // (written down: which square is fused moved with the code around it)
                if (first) {
                    const v2f nz = rxp_noise((uint32_t)q, f_lo, f_hi, cell, p.seed_lo, p.seed_hi, e);
                    pn += nz.x * nz.x + nz.y * nz.y;
                }
            }
        }
        ps = papr_wave_reduce<false>(ps);
        if (lane == 0) red[wv] = ps;
        if (first) {
            pn = papr_wave_reduce<false>(pn);
            if (lane == 0) red[W + wv] = pn;
        }
        __syncthreads();
        float Ps = 0.f, Pn = 0.f;
        for (int w = 0; w < W; ++w) {
            Ps += red[w];
            Pn += red[W + w];
        }
        return sqrtf(Ps * p.nlin[sn] / Pn);
    };
    float g = 0.f;
    if constexpr (!PASS1_PER_POINT) g = pass1(p.x + (size_t)job * T, true);   // (the gain never sees a point's offsets)
    float2 *buf = rows + (size_t)wv * ROWLEN;
    float2 *xr = buf + N;
    [[maybe_unused]] float2 *xir = xr + RG::XROW;                     // (ACI)
    const int h2 = delta >> 1;
#pragma unroll 1
    for (int pt = 0; pt < NP; ++pt) {
        // the point's on-air waveform
        const float2 *__restrict__ x = (!PA || pa.pts[pt].model == WOFDM_PA_M_LINEAR) ? p.x + (size_t)job * T
                                                                                      : pa.y + ((size_t)job * NP + pt) * (size_t)T;
        if constexpr (DOP) {
            const int trk = LINK ? lk.pts[pt].track : pt;
            const float2 *__restrict__ knots = dp.knots + ((size_t)trk * p.n_ch + ch) * (size_t)dp.n_knots * LT;
            for (int i = tid; i < dp.n_knots * LT; i += NT) kn[i] = knots[i];
            __syncthreads();
        }
        if constexpr (PASS1_PER_POINT) g = pass1(x, pt == 0);
        // (SOFT) v W2 of the point: v = g^2 Pn / NL, Pn the sum pass 1 formed (its partials stay in red), W2 the pair's
        [[maybe_unused]] float soft_vw = 0.f;
        if constexpr (SOFT) {
            float Pn = 0.f;
            for (int w = 0; w < W; ++w) Pn += red[W + w];
            soft_vw = g * g * Pn / (float)NL * so.w2[pair];
        }
        // pass 2
        const int theta = SYNC ? sp.pts[pt].theta : 0;
        [[maybe_unused]] const float turn = SYNC ? sp.pts[pt].eps * (1.0f / (float)N) : 0.f;   // (exact: N is a power of two)
        [[maybe_unused]] const double pn_turn = PN ? pn.pts[pt].turn : 0.0;
        [[maybe_unused]] const bool pn_tracked = PN ? pn.pts[pt].tracked != 0 : false;
        // (LINK) the neighbour of the point: on the air or not (wave-uniform), its offset and amplitude
        [[maybe_unused]] const bool nb_on = LINK ? lk.pts[pt].aci_on != 0 : ACI;
        [[maybe_unused]] const int ioff = LINK ? lk.pts[pt].ioff : ap.ioff;
        [[maybe_unused]] const float a_lvl = LINK ? lk.pts[pt].a_lvl : ap.a_lvl;
        const size_t slot = (size_t)job * NP + pt;
        // (TRACK) the point's receiver (wave-uniform): tracked = either mechanism is on
        [[maybe_unused]] bool tcpe = false, tpost = false;
        if constexpr (TRACK) {
            tcpe = __builtin_amdgcn_readfirstlane(tk.pts[pt].cpe) != 0;
            tpost = __builtin_amdgcn_readfirstlane(tk.pts[pt].post) != 0;
        }
        [[maybe_unused]] const bool tracked = tcpe || tpost;
        float pw[BINS];
        uint32_t cnt[BINS];
#pragma unroll
        for (int j = 0; j < BINS; ++j) {
            pw[j] = 0.f;
            cnt[j] = 0u;
        }
        for (int s0 = 0; s0 < S; s0 += W) {
            int s = s0 + wv;
            const bool live = s < S;                                  // (wave-uniform)
            if constexpr (TRACK) {
                if (tpost && live) s = s == 0 ? 0 : (s == 1 ? S - 1 : s - 1);   // the postamble in the first round
            }
            if (live) {
                const int a0 = s * B + p.gam + theta;                 // first sample under the Rx window (m:442-454)
                [[maybe_unused]] const float2 bs = SYNC ? sp.base[(size_t)pt * S + s] : make_float2(1.f, 0.f);
                // (PN) the walk under the window, a0 + m < S B, and the common phase the point takes off it
                // (LINK: a timing offset moves the window off [0, S B), and the index is clamped onto it)
                [[maybe_unused]] const double *__restrict__ uw = PN ? walk + a0 : nullptr;
                [[maybe_unused]] auto u_at = [&](int m) {
                    if constexpr (LINK) {
                        const int a = a0 + m;
                        return walk[a < 0 ? 0 : (a > walk_last ? walk_last : a)];
                    } else {
                        return uw[m];
                    }
                };
                [[maybe_unused]] double pn_c = 0.0;
                if constexpr (PN) {
                    if (pn_tracked) {
                        const double u0 = u_at(0);
                        double acc = 0.0;
                        for (int m = lane; m < N + delta; m += 64) acc += u_at(m) - u0;
                        pn_c = u0 + pn_wave_sum(acc) / (double)(N + delta);
                    }
                }
                for (int i = lane; i < N + delta + LT - 1; i += 64) {
                    const int t = a0 - (LT - 1) + i;
                    xr[i] = (t >= 0 && t < T) ? x[t] : make_float2(0.f, 0.f);
                    if constexpr (ACI) {
                        if (!LINK || nb_on) {
                            const int ti = t + ioff;
                            xir[i] = (ti >= 0 && ti < ap.Ti) ? xi[ti] : make_float2(0.f, 0.f);
                        }
                    }
                }
                wave_sync();
                // r[a] = conv[a] + g n[a] (m:260-261, 290-293) of the sample m under the window, a = a0 + m
                auto rxs = [&](int m, auto fold) {
                    const uint32_t a = (uint32_t)(a0 + m);
                    // (LINK: before the frame every product is zero, and the tap time is 0, never a wrapped index)
                    const auto tap = taps_at(LINK && a0 + m < 0 ? 0u : a);
                    float cr = 0.f, ci = 0.f;
#pragma unroll
                    for (int l = 0; l < LT; ++l) fir_tap<decltype(fold)::value>(tap(l), xr[m + (LT - 1) - l], cr, ci);
                    if constexpr (ACI) {
                        if (!LINK || nb_on) {
                            float ar = 0.f, ai = 0.f;
#pragma unroll
                            for (int l = 0; l < LT; ++l) {
                                const float2 xv = xir[m + (LT - 1) - l], hv = itaps[l];
                                if constexpr (LINK) {
                                    aci_tap<decltype(fold)::value>(hv, xv, ar, ai);
                                } else {
                                    ar += hv.x * xv.x - hv.y * xv.y;
                                    ai += hv.x * xv.y + hv.y * xv.x;
                                }
                            }
                            if constexpr (LINK) {
                                cr = __builtin_fmaf(a_lvl, ar, cr);   // (cr += a_lvl ar as the aci kernel has it)
                                ci = __builtin_fmaf(a_lvl, ai, ci);
                            } else {
                                cr += a_lvl * ar;
                                ci += a_lvl * ai;
                            }
                        }
                    }
                    const v2f nz = rxp_noise(a >> 1, f_lo, f_hi, cell, p.seed_lo, p.seed_hi, (int)(a & 1u));
                    float2 r = make_float2(cr + g * nz.x, ci + g * nz.y);
                    // (LINK: the carrier offset's rotation, then the phase noise's; each is exactly (1, 0) when neutral)
                    if constexpr (SYNC) {                             // rotated by the oscillator's phase at m
                        float tn = turn * (float)m, sv, cv;
                        tn -= rintf(tn);
                        sincospif(2.0f * tn, &sv, &cv);
                        const float qr = bs.x * cv - bs.y * sv, qi = bs.x * sv + bs.y * cv;
                        r = make_float2(r.x * qr - r.y * qi, __builtin_fmaf(r.x, qi, r.y * qr));   // (r.x qi + r.y qr, written down likewise)
                    }
                    if constexpr (PN) {                               // rotated by the oscillator's phase at a0 + m
                        double td = (u_at(m) - pn_c) * pn_turn;
                        td -= rint(td);
                        float sv, cv;
                        sincospif(2.0f * (float)td, &sv, &cv);
                        r = make_float2(r.x * cv - r.y * sv, __builtin_fmaf(r.x, sv, r.y * cv));   // (the sync arm's forms)
                    }
                    return r;
                };
#pragma unroll 1
                for (int j = 0; j < BINS; ++j) {
                    // Rx window, fold, circular shift (m:297-355): z[t] = sum_{m = t + kappa + delta/2 (mod N)} w[m] r[gamma + m]
                    const int t = lane + 64 * j, m0 = (t + p.kap + h2) & (N - 1);
                    float2 z = rxs(m0, std::false_type{});
                    z.x *= wrx[m0];
                    z.y *= wrx[m0];
                    if (m0 < delta) {
                        const float2 z2 = rxs(m0 + N, std::true_type{});
                        z.x += wrx[m0 + N] * z2.x;
                        z.y += wrx[m0 + N] * z2.y;
                    }
                    buf[__brev((uint32_t)t) >> (32 - LOG2)] = z;
                }
                wave_sync();
                // DFT (dftmtx(N), m:306): radix-2 stages in place
                for (int len = 2, sh = LOG2 - 1; len <= N; len <<= 1, --sh) {
                    const int half = len >> 1;
                    for (int b = lane; b < N / 2; b += 64) {
                        const int kk = b & (half - 1), i = ((b - kk) << 1) | kk;
                        const float2 w = tw[kk << sh], a = buf[i], c = buf[i + half];
                        const float tr = c.x * w.x - c.y * w.y, ti = c.x * w.y + c.y * w.x;
                        buf[i] = make_float2(a.x + tr, a.y + ti);
                        buf[i + half] = make_float2(a.x - tr, a.y - ti);
                    }
                    wave_sync();
                }
            }
            if (s0 == 0) {
                if constexpr (TRACK) {
                    if (tracked) {
                        // the channel estimates of the known symbols on the loaded bins: wave 0 H0 = Y0 / X0, wave 1 HL
                        if (wv == 0 || (tpost && wv == 1)) {
                            float2 *dst = wv == 0 ? G : hl;
                            const float2 *__restrict__ Xk = Xg + (size_t)s * N;
                            for (int n = lane; n < N; n += 64) {
                                const float2 y = buf[n], xk = Xk[n];
                                const float d = xk.x * xk.x + xk.y * xk.y;
                                const bool on = p.amask == nullptr || p.amask[n] != 0;
                                dst[n] = on ? make_float2((y.x * xk.x + y.y * xk.y) / d, (y.y * xk.x - y.x * xk.y) / d) : make_float2(0.f, 0.f);
                            }
                        }
                        __syncthreads();
                        if (tpost) {
                            if (wv == 0) {
                                float cx = 0.f, cy = 0.f;
                                for (int n = lane; n < N; n += 64) {
                                    const float2 a = hl[n], b = G[n];
                                    cx += a.x * b.x + a.y * b.y;
                                    cy += a.y * b.x - a.x * b.y;
                                }
                                cx = papr_wave_reduce<false>(cx);
                                cy = papr_wave_reduce<false>(cy);
                                const float m = sqrtf(cx * cx + cy * cy);
                                const float2 rho = m > 0.f ? make_float2(cx / m, cy / m) : make_float2(1.f, 0.f);
                                for (int n = lane; n < N; n += 64) {
                                    const float2 a = hl[n], b = G[n];
                                    hl[n] = make_float2(a.x * rho.x + a.y * rho.y - b.x, a.y * rho.x - a.x * rho.y - b.y);
                                }
                                if (lane == 0) {
                                    red[2 * W] = rho.x;
                                    red[2 * W + 1] = rho.y;
                                }
                            }
                            __syncthreads();
                        }
                    }
                }
                if (!tracked) {
                    // pilot LS estimate (m:266-267): G = X0 / Y0 on the loaded bins
                    if (wv == 0)
                        for (int n = lane; n < N; n += 64) {
                            const float2 y = buf[n], x0 = Xg[n];
                            const float d = y.x * y.x + y.y * y.y;
                            const bool on = p.amask == nullptr || p.amask[n] != 0;
                            G[n] = on ? make_float2((x0.x * y.x + x0.y * y.y) / d, (x0.y * y.x - x0.x * y.y) / d) : make_float2(0.f, 0.f);
                        }
                    __syncthreads();
                }
            }
            if (live) {
                [[maybe_unused]] float spw = 0.f;
                [[maybe_unused]] uint32_t scn = 0u;
                // (TRACK) a symbol that counts: not the pilot, and not the postamble of a point with post
                [[maybe_unused]] const bool counted = s >= 1 && !(tpost && s == S - 1);
                [[maybe_unused]] const float2 *Gs = G;                // the equaliser the symbol's decisions see
                if constexpr (TRACK) {
                    if (tracked && counted) {
                        const float2 *__restrict__ Xs = Xg + (size_t)s * N;
                        const float t = (float)s / (float)(S - 1);
                        float2 q = make_float2(1.f, 0.f);
                        if (tcpe) {
                            float cx = 0.f, cy = 0.f;
                            for (int n = lane; n < N; n += 64) {
                                if (tk.pilots[n] == 0) continue;
                                float2 hh = G[n];
                                if (tpost) hh = make_float2(hh.x + t * hl[n].x, hh.y + t * hl[n].y);
                                const float2 y = buf[n], xs = Xs[n];
                                const float zr = hh.x * xs.x - hh.y * xs.y, zi = hh.x * xs.y + hh.y * xs.x;
                                cx += y.x * zr + y.y * zi;
                                cy += y.y * zr - y.x * zi;
                            }
                            cx = papr_wave_reduce<false>(cx);
                            cy = papr_wave_reduce<false>(cy);
                            const float m = sqrtf(cx * cx + cy * cy);
                            if (m > 0.f) q = make_float2(cx / m, cy / m);
                        } else {
                            // e^{i t arg rho}, the principal value, in turns: atan2 / pi <= 1 in magnitude, so sincospif needs no reduction
                            float sv, cv;
                            sincospif(t * (atan2f(red[2 * W + 1], red[2 * W]) * 0.31830988618379067f), &sv, &cv);
                            q = make_float2(cv, sv);
                        }
                        // conj(q) conj(Hh) / |Hh|^2 per bin, 0 on an unloaded one as G is
                        for (int n = lane; n < N; n += 64) {
                            float2 hh = G[n];
                            if (tpost) hh = make_float2(hh.x + t * hl[n].x, hh.y + t * hl[n].y);
                            const float d = hh.x * hh.x + hh.y * hh.y;
                            const bool on = p.amask == nullptr || p.amask[n] != 0;
                            xr[n] = on ? make_float2((q.x * hh.x - q.y * hh.y) / d, -(q.x * hh.y + q.y * hh.x) / d) : make_float2(0.f, 0.f);
                        }
                        wave_sync();
                        Gs = xr;
                    }
                }
                if (TRACK ? counted : s >= 1) {
#pragma unroll
                    for (int j = 0; j < BINS; ++j) {
                        const int n = lane + 64 * j;
                        if (p.amask != nullptr && p.amask[n] == 0) continue;
                        if constexpr (TRACK) {
                            if (tk.pilots != nullptr && tk.pilots[n] != 0) continue;
                        }
                        const float2 y = buf[n], gq = (TRACK ? Gs : G)[n], xs = Xg[(size_t)s * N + n];
                        const float er = y.x * gq.x - y.y * gq.y, ei = y.x * gq.y + y.y * gq.x;   // equaliser (m:268)
                        const uint32_t d = rxp_slice(p.k, xs.x, xs.y) ^ rxp_slice(p.k, er, ei);    // (X is the point of its own label)
                        const uint32_t c = (uint32_t)__popc(d) + (d != 0u ? 0x10000u : 0u);
                        const float e2 = (er - xs.x) * (er - xs.x) + (ei - xs.y) * (ei - xs.y);
                        cnt[j] += c;
                        pw[j] += e2;
                        if constexpr (POINTS) {
                            scn += c;
                            spw += e2;
                        }
                    }
                }
                if constexpr (POINTS) {
                    // the symbol's sums over the bins: at most N k < 2^16 bit errors and N symbol errors, so the halves do not meet
                    spw = papr_wave_reduce<false>(spw);
#pragma unroll
                    for (int o = 32; o >= 1; o >>= 1) scn += (uint32_t)__shfl_xor((int)scn, o, 64);
                    if (lane == 0) {
                        sp.sym_pow[slot * S + s] = spw;
                        sp.sym_cnt[slot * S + s] = scn;
                    }
                }
                if constexpr (TRACK) {
                    if (counted) {
                        soft_symbol<N, true, CODED>(p, so, buf, Gs, Xg + (size_t)s * N, soft_vw, slot, s, lane, tk.pilots, cd.llr_scale,
                                                    cd.soft);
                    } else if (s >= 1) {
                        soft_symbol_zero<N>(so, S, slot, s, lane);
                        if constexpr (CODED) coded_symbol_zero<N>(cd.soft, S, slot, s, lane);
                    }
                } else if constexpr (SOFT) {
                    if (s >= 1) soft_symbol<N>(p, so, buf, G, Xg + (size_t)s * N, soft_vw, slot, s, lane);
                }
            }
            wave_sync();
        }
        // the waves' sums in wave order (their rows are free now): float [W][N], then uint32 [W][N]
        __syncthreads();
        float *redp = reinterpret_cast<float *>(rows);
        uint32_t *redc = reinterpret_cast<uint32_t *>(redp + W * N);
#pragma unroll
        for (int j = 0; j < BINS; ++j) {
            redp[wv * N + lane + 64 * j] = pw[j];
            redc[wv * N + lane + 64 * j] = cnt[j];
        }
        __syncthreads();
        for (int n = tid; n < N; n += NT) {
            float t = 0.f;
            uint32_t c = 0u;
            for (int w = 0; w < W; ++w) {
                t += redp[w * N + n];
                c += redc[w * N + n];
            }
            p.part_pow[slot * N + n] = t;
            p.part_cnt[slot * N + n] = c;
        }
        if constexpr (POINTS) __syncthreads();                        // the rows, G and the knots belong to the next point
    }
}

template <int N>
__global__ void __launch_bounds__(rxp_geo<N>::WAVES * 64) wofdm_rxprof_kernel(const wofdm_rparams p)
{
    rxprof_body<N, RXP_PLAIN>(p, wofdm_aparams{}, wofdm_sparams{}, wofdm_dparams{}, wofdm_paparams{}, wofdm_pnparams{}, wofdm_lparams{});
}
template <int N>
__global__ void __launch_bounds__(rxp_geo<N>::WAVES * 64) wofdm_rxprof_aci_kernel(const wofdm_rparams p, const wofdm_aparams ap)
{
    rxprof_body<N, RXP_ACI>(p, ap, wofdm_sparams{}, wofdm_dparams{}, wofdm_paparams{}, wofdm_pnparams{}, wofdm_lparams{});
}
template <int N>
__global__ void __launch_bounds__(rxp_geo<N>::WAVES * 64) wofdm_rxprof_sync_kernel(const wofdm_rparams p, const wofdm_sparams sp)
{
    rxprof_body<N, RXP_SYNC>(p, wofdm_aparams{}, sp, wofdm_dparams{}, wofdm_paparams{}, wofdm_pnparams{}, wofdm_lparams{});
}
template <int N>
__global__ void __launch_bounds__(rxp_geo<N>::WAVES * 64) wofdm_rxprof_doppler_kernel(const wofdm_rparams p, const wofdm_sparams sp,
                                                                                     const wofdm_dparams dp)
{
    rxprof_body<N, RXP_DOPPLER>(p, wofdm_aparams{}, sp, dp, wofdm_paparams{}, wofdm_pnparams{}, wofdm_lparams{});
}
template <int N>
__global__ void __launch_bounds__(rxp_geo<N>::WAVES * 64) wofdm_rxprof_pa_kernel(const wofdm_rparams p, const wofdm_sparams sp,
                                                                                const wofdm_paparams pa)
{
    rxprof_body<N, RXP_PA>(p, wofdm_aparams{}, sp, wofdm_dparams{}, pa, wofdm_pnparams{}, wofdm_lparams{});
}
template <int N>
__global__ void __launch_bounds__(rxp_geo<N>::WAVES * 64) wofdm_rxprof_pn_kernel(const wofdm_rparams p, const wofdm_sparams sp,
                                                                                const wofdm_pnparams pn)
{
    rxprof_body<N, RXP_PN>(p, wofdm_aparams{}, sp, wofdm_dparams{}, wofdm_paparams{}, pn, wofdm_lparams{});
}
template <int N>
__global__ void __launch_bounds__(rxp_geo<N>::WAVES * 64) wofdm_rxprof_link_kernel(const wofdm_rparams p, const wofdm_aparams ap,
                                                                                  const wofdm_sparams sp, const wofdm_dparams dp,
                                                                                  const wofdm_paparams pa, const wofdm_pnparams pn,
                                                                                  const wofdm_lparams lk)
{
    rxprof_body<N, RXP_LINK>(p, ap, sp, dp, pa, pn, lk);
}
// wofdm_rx_profile_soft: the link arm with the demapper (soft_symbol) behind the hard decisions of every data symbol
template <int N>
__global__ void __launch_bounds__(rxp_geo<N>::WAVES * 64) wofdm_rxprof_soft_kernel(const wofdm_rparams p, const wofdm_aparams ap,
                                                                                  const wofdm_sparams sp, const wofdm_dparams dp,
                                                                                  const wofdm_paparams pa, const wofdm_pnparams pn,
                                                                                  const wofdm_lparams lk, const wofdm_softparams so)
{
    rxprof_body<N, RXP_LINK, true>(p, ap, sp, dp, pa, pn, lk, so);
}
// wofdm_rx_profile_tracking: the soft kernel with the tracking receiver (TRACK) in the one-shot receiver's place, per point
template <int N>
__global__ void __launch_bounds__(rxp_geo<N>::WAVES * 64) wofdm_rxprof_tracking_kernel(const wofdm_rparams p, const wofdm_aparams ap,
                                                                                      const wofdm_sparams sp, const wofdm_dparams dp,
                                                                                      const wofdm_paparams pa, const wofdm_pnparams pn,
                                                                                      const wofdm_lparams lk, const wofdm_softparams so,
                                                                                      const wofdm_trackparams tk)
{
    rxprof_body<N, RXP_LINK, true, true>(p, ap, sp, dp, pa, pn, lk, so, tk);
}
// wofdm_rx_profile_coded: the tracking kernel plus the soft-bit stores (CODED) wofdm_viterbi_kernel decodes
template <int N>
__global__ void __launch_bounds__(rxp_geo<N>::WAVES * 64) wofdm_rxprof_coded_kernel(const wofdm_rparams p, const wofdm_aparams ap,
                                                                                   const wofdm_sparams sp, const wofdm_dparams dp,
                                                                                   const wofdm_paparams pa, const wofdm_pnparams pn,
                                                                                   const wofdm_lparams lk, const wofdm_softparams so,
                                                                                   const wofdm_trackparams tk, const wofdm_codeparams cd)
{
    rxprof_body<N, RXP_LINK, true, true, true>(p, ap, sp, dp, pa, pn, lk, so, tk, cd);
}

// totals[cell][n] += the chunk's items of the cell, in frame order; grid (N / 64, cells the chunk touches)
template <int N>
__global__ void __launch_bounds__(64) wofdm_rxprof_reduce_kernel(const wofdm_rparams p, uint64_t cell0)
{
    const int n = blockIdx.x * 64 + threadIdx.x;
    const uint64_t cell = cell0 + blockIdx.y, end = p.item0 + (uint64_t)p.n_jobs;
    const uint64_t lo = cell * p.frames > p.item0 ? cell * p.frames : p.item0;
    const uint64_t hi = (cell + 1) * p.frames < end ? (cell + 1) * p.frames : end;
    double acc = 0.0;
    unsigned long long be = 0ull, se = 0ull;
    for (uint64_t i = lo; i < hi; ++i) {
        const size_t idx = (size_t)(i - p.item0) * N + n;
        const uint32_t c = p.part_cnt[idx];
        acc += (double)p.part_pow[idx];
        be += c & 0xFFFFu;
        se += c >> 16;
    }
    if (lo < hi) {
        p.errs[2 * (cell * N + n)] += be;
        p.errs[2 * (cell * N + n) + 1] += se;
        p.pow[cell * N + n] += acc;
    }
}

// wofdm_rxprof_reduce_kernel per point: totals[point][cell][n] += the chunk's items of the cell, in frame order, one addition
// per frame onto the running total (so the sums do not depend on where a chunk ends); grid (N / 64 + 1, cells the chunk
// touches, points) -- the last block of x takes the data symbols s = 1 ... S - 1 in the bins' place
template <int N>
__global__ void __launch_bounds__(64) wofdm_rxprof_sync_reduce_kernel(const wofdm_rparams p, const wofdm_sparams sp, uint64_t cell0)
{
    const bool syms = blockIdx.x == N / 64;
    const int n = syms ? (int)threadIdx.x + 1 : (int)(blockIdx.x * 64 + threadIdx.x), len = syms ? p.S : N;
    if (syms && n >= p.S) return;
    const uint64_t cell = cell0 + blockIdx.y, end = p.item0 + (uint64_t)p.n_jobs;
    const uint64_t lo = cell * p.frames > p.item0 ? cell * p.frames : p.item0;
    const uint64_t hi = (cell + 1) * p.frames < end ? (cell + 1) * p.frames : end;
    if (lo >= hi) return;
    const uint32_t pt = blockIdx.z;
    const float *ppow = syms ? sp.sym_pow : p.part_pow;
    const uint32_t *pcnt = syms ? sp.sym_cnt : p.part_cnt;
    const size_t out = syms ? ((size_t)pt * sp.cells + cell) * (size_t)(p.S - 1) + (size_t)(n - 1) : ((size_t)pt * sp.cells + cell) * N + n;
    double *tot = syms ? sp.sym_tot : p.pow;
    unsigned long long *terr = syms ? sp.sym_errs : p.errs;
    double acc = tot[out];
    unsigned long long be = 0ull, se = 0ull;
    for (uint64_t i = lo; i < hi; ++i) {
        const size_t idx = ((size_t)(i - p.item0) * sp.n_points + pt) * (size_t)len + n;
        const uint32_t c = pcnt[idx];
        acc += (double)ppow[idx];
        be += c & 0xFFFFu;
        se += c >> 16;
    }
    terr[2 * out] += be;
    terr[2 * out + 1] += se;
    tot[out] = acc;
}

// The ordered sums of wofdm_rx_profile_soft, first step: the penalties of a frame's data symbols s = 1 ... S - 1, ascending in
// single precision from the first, per (item, point, scale, bin); the sum takes the place of the first symbol's element of
// bit_part.  One thread per element, every element of the chunk at once -- the second step's loop over the frames is serial,
// and S - 1 loads per frame inside it made the call six times the link call's length.
template <int N>
__global__ void __launch_bounds__(256) wofdm_rxprof_soft_frame_kernel(const wofdm_softparams so, int S, size_t n_elems)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;          // (slot, scale, n)
    if (e >= n_elems) return;
    const size_t row = (size_t)so.n_scales * N, slot = e / row;
    float *q = so.bit_part + slot * (size_t)(S - 1) * row + (e - slot * row);
    float f = q[0];
    for (int s = 2; s < S; ++s) f += q[(size_t)(s - 1) * row];
    q[0] = f;
}

// Second step: bit_tot[point][cell][scale][n] += the frames' sums of the chunk's items of the cell, one addition per frame
// onto the running fp64 total, frames ascending, so the totals do not depend on where a chunk ends; grid (N / 64 + 1, cells the
// chunk touches, points x scales) -- the last block of x adds the symbols' sums sym_part onto
// sym_tot[point][cell][scale][s - 1] the same way.  Eight frames' loads are in flight at a time; the additions stay in order.
template <int N>
__global__ void __launch_bounds__(64) wofdm_rxprof_soft_reduce_kernel(const wofdm_rparams p, const wofdm_sparams sp,
                                                                      const wofdm_softparams so, uint64_t cell0)
{
    const bool syms = blockIdx.x == N / 64;
    const int S = p.S, nsc = so.n_scales;
    const int n = syms ? (int)threadIdx.x + 1 : (int)(blockIdx.x * 64 + threadIdx.x);
    if (syms && n >= S) return;
    const uint64_t cell = cell0 + blockIdx.y, end = p.item0 + (uint64_t)p.n_jobs;
    const uint64_t lo = cell * p.frames > p.item0 ? cell * p.frames : p.item0;
    const uint64_t hi = (cell + 1) * p.frames < end ? (cell + 1) * p.frames : end;
    if (lo >= hi) return;
    const uint32_t pt = blockIdx.z / (uint32_t)nsc, sc = blockIdx.z - pt * (uint32_t)nsc;
    const size_t cellrow = ((size_t)pt * sp.cells + cell) * (size_t)nsc + sc;
    double *tot = syms ? so.sym_tot + cellrow * (size_t)(S - 1) + (size_t)(n - 1) : so.bit_tot + cellrow * N + n;
    // the element of item 0 of the chunk, and the distance from an item to the next
    const size_t per_item = (size_t)sp.n_points * (size_t)nsc * (syms ? (size_t)S : (size_t)(S - 1) * N);
    const float *src = syms ? so.sym_part + ((size_t)pt * nsc + sc) * (size_t)S + (size_t)n
                            : so.bit_part + ((size_t)pt * (size_t)(S - 1) * nsc + sc) * N + n;
    double acc = *tot;
    uint64_t i = lo - p.item0;
    const uint64_t stop = hi - p.item0;
    for (; i + 8 <= stop; i += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = src[(size_t)(i + u) * per_item];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += (double)v[u];
    }
    for (; i < stop; ++i) acc += (double)src[(size_t)i * per_item];
    *tot = acc;
}

// ---------------------------------------------------------------------------------------------
// The memoryless power amplifier behind the Tx chain (wofdm_rx_profile_pa, wofdm_tx_psd_batch_pa; wofdm_pa.h): y = g x with
// r = |x|, rho = r / a_sat; the phase is untouched (no AM/PM).
//   WOFDM_PA_M_LINEAR  y = x, no arithmetic at all
//   WOFDM_PA_M_RAPP    g = (1 + rho^(2p))^(-1/(2p)); above rho = 1 in the form (1 / rho) (1 + rho^(-2p))^(-1/(2p)), so that no
//                      finite input overflows: with u = 2^(-2p |log2 rho|) <= 1 both forms are 2^(-log2(1 + u) / (2p)), times
//                      1 / rho above 1.  log2 / exp2 are the hardware forms (v_log_f32, v_exp_f32): their absolute error of an ulp or so of the
//                      argument's logarithm reaches g as some 1e-7, the rounding of the fp32 chain around it.
//   WOFDM_PA_M_CLIP    the soft limiter, the p -> infinity limit: g = 1 up to rho = 1, 1 / rho above
// g = 1 at r = 0.  The ONE definition both routes' kernels call; rx_profile.pa_gain is its fp64 mirror.
__device__ __forceinline__ float2 pa_amplify(const float2 v, int model, float asat, float two_p, float inv_two_p)
{
    if (model == WOFDM_PA_M_LINEAR) return v;
    const float r = sqrtf(v.x * v.x + v.y * v.y);
    if (!(r > 0.f)) return v;
    const float rho = r / asat;
    float g;
    if (model == WOFDM_PA_M_CLIP) {
        g = rho > 1.f ? 1.0f / rho : 1.f;
    } else {
        const float u = __builtin_amdgcn_exp2f(-two_p * fabsf(__builtin_amdgcn_logf(rho)));
        g = __builtin_amdgcn_exp2f(-inv_two_p * __builtin_amdgcn_logf(1.f + u));
        if (rho > 1.f) g = g / rho;
    }
    return make_float2(g * v.x, g * v.y);
}

// The amplified waveforms of wofdm_rx_profile_pa: grid (jobs of the chunk, points), 256 threads.  y[job][point][t] =
// pa_amplify(x[job][t]) with a_sat of (point, the pair of the job's cell); a linear point writes nothing -- the receive kernel
// reads x itself.  pwr[job][point] = {sum |x|^2, sum |y|^2} over the T samples: thread-strided partials, the wave sum of
// papr_wave_reduce, the four waves in order.
__global__ void __launch_bounds__(256) wofdm_pa_wave_kernel(const wofdm_paparams pa, const float2 *__restrict__ x, int T, uint64_t item0,
                                                            uint64_t frames, uint32_t cpp)
{
    __shared__ float red[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t job = blockIdx.x, pt = blockIdx.y;
    const uint64_t cell = (item0 + job) / frames;
    const uint32_t pair = (uint32_t)(cell / cpp);
    const wofdm_papoint q = pa.pts[pt];
    const float asat = pa.asat[(size_t)pt * pa.pairs + pair];
    const float2 *__restrict__ src = x + (size_t)job * T;
    float2 *__restrict__ dst = pa.y + ((size_t)job * pa.n_points + pt) * (size_t)T;
    float si = 0.f, so = 0.f;
    if (q.model == WOFDM_PA_M_LINEAR) {
        for (int t = tid; t < T; t += 256) {
            const float2 v = src[t];
            si += v.x * v.x + v.y * v.y;
        }
        so = si;
    } else {
        for (int t = tid; t < T; t += 256) {
            const float2 v = src[t], w = pa_amplify(v, q.model, asat, q.two_p, q.inv_two_p);
            dst[t] = w;
            si += v.x * v.x + v.y * v.y;
            so += w.x * w.x + w.y * w.y;
        }
    }
    si = papr_wave_reduce<false>(si);
    so = papr_wave_reduce<false>(so);
    if (lane == 0) {
        red[0][wv] = si;
        red[1][wv] = so;
    }
    __syncthreads();
    if (tid < 2) {
        float t = 0.f;
        for (int w = 0; w < 4; ++w) t += red[tid][w];
        pa.pwr[((size_t)job * pa.n_points + pt) * 2 + tid] = t;
    }
}

// pwr_tot[point][cell][2] += the chunk's items of the cell, in frame order, one addition per frame onto the running fp64 total;
// grid (cells the chunk touches), a thread per (point, which)
__global__ void __launch_bounds__(64) wofdm_pa_power_reduce_kernel(const wofdm_paparams pa, uint64_t item0, int n_jobs, uint64_t frames,
                                                                   uint64_t cells, uint64_t cell0)
{
    const uint32_t pt = threadIdx.x >> 1, which = threadIdx.x & 1;
    if (pt >= (uint32_t)pa.n_points) return;
    const uint64_t cell = cell0 + blockIdx.x, end = item0 + (uint64_t)n_jobs;
    const uint64_t lo = cell * frames > item0 ? cell * frames : item0;
    const uint64_t hi = (cell + 1) * frames < end ? (cell + 1) * frames : end;
    if (lo >= hi) return;
    const size_t out = ((size_t)pt * cells + cell) * 2 + which;
    double acc = pa.pwr_tot[out];
    for (uint64_t i = lo; i < hi; ++i) acc += (double)pa.pwr[((size_t)(i - item0) * pa.n_points + pt) * 2 + which];
    pa.pwr_tot[out] = acc;
}

// The amplifier of wofdm_tx_psd_batch_pa, two kernels between the waveform kernels and the periodogram; grid (jobs), 1024
// threads each.  The first leaves power[job][0] = sum |x|^2 over the job's len samples (thread-strided partials,
// papr_wave_reduce, the 16 waves in order: a fixed order); the second forms a_sat^2 = (sum / len) 10^(ibo / 10) in double,
// stores a_sat in single precision, amplifies the job's waveform in place and leaves power[job][1] = sum |y|^2, in the same
// order.  A job without an amplifier, with a linear one or without power keeps its waveform, bit for bit, and gets
// power[job][1] = power[job][0].
__global__ void __launch_bounds__(1024) wofdm_pa_job_power_kernel(const wofdm_bjob *__restrict__ jobs, const float2 *__restrict__ x,
                                                                  float *__restrict__ power)
{
    __shared__ float red[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const wofdm_bjob jb = jobs[blockIdx.x];
    const float2 *__restrict__ src = x + jb.x_off;
    float si = 0.f;
    for (int t = tid; t < jb.len; t += 1024) {
        const float2 v = src[t];
        si += v.x * v.x + v.y * v.y;
    }
    si = papr_wave_reduce<false>(si);
    if (lane == 0) red[wv] = si;
    __syncthreads();
    if (tid == 0) {
        float t = 0.f;
        for (int w = 0; w < 16; ++w) t += red[w];
        power[2 * blockIdx.x] = t;
    }
}
__global__ void __launch_bounds__(1024) wofdm_pa_job_apply_kernel(const wofdm_bjob *__restrict__ jobs, const wofdm_pajob *__restrict__ pa,
                                                                  float2 *__restrict__ x, float *__restrict__ power)
{
    __shared__ float red[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const wofdm_bjob jb = jobs[blockIdx.x];
    const wofdm_pajob q = pa[blockIdx.x];
    const float sum_in = power[2 * blockIdx.x];
    if (q.model < 0 || q.model == WOFDM_PA_M_LINEAR || !(sum_in > 0.f)) {         // (uniform over the workgroup)
        if (tid == 0) power[2 * blockIdx.x + 1] = sum_in;
        return;
    }
    const float asat = (float)sqrt((double)sum_in / (double)jb.len * q.scale);
    float2 *__restrict__ xj = x + jb.x_off;
    float so = 0.f;
    for (int t = tid; t < jb.len; t += 1024) {
        const float2 w = pa_amplify(xj[t], q.model, asat, q.two_p, q.inv_two_p);
        xj[t] = w;
        so += w.x * w.x + w.y * w.y;
    }
    so = papr_wave_reduce<false>(so);
    if (lane == 0) red[wv] = so;
    __syncthreads();
    if (tid == 0) {
        float t = 0.f;
        for (int w = 0; w < 16; ++w) t += red[w];
        power[2 * blockIdx.x + 1] = t;
    }
}

#if WOFDM_TU_N == 64
// Philox known-answer kernel (wofdm_philox_kat): in one unit only
__global__ void philox_kat_kernel(const uint32_t *ck, uint32_t *out)
{
    if (threadIdx.x == 0) {
        const philox_out o = philox4x32_10(ck[0], ck[1], ck[2], ck[3], ck[4], ck[5]);
        for (int i = 0; i < 4; ++i) out[i] = o.w[i];
    }
}
#endif

// The launchers of this unit's DFT length (wofdm_aux_fns, wofdm_kernel.h)
hipError_t interf_launch(int jobs, int P, int B, int mu, int delta, int gam, int kap, int n_ch, const float *wtx,
                         const float *wrx, const float2 *h, float *power, hipStream_t s)
{
    constexpr int N = WOFDM_TU_N, W = interf_geo<N>::WAVES;
    wofdm_iparams ip;
    ip.P = P; ip.B = B; ip.mu = mu; ip.delta = delta; ip.gam = gam; ip.kap = kap; ip.n_ch = n_ch;
    ip.rowlen = (24 + 2 * B + 24 + 64 * interf_geo<N>::RB2 - 2 * B + 1) / 2 * 2;   // covers every lane's FIR window
    ip.power = power;
    const size_t lds = 8 * (size_t)N * 2 + 4 * (size_t)(N + 64) + (size_t)W * 8 * (ip.rowlen + N);
    if (lds > 160u * 1024u) return hipErrorInvalidValue;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(wofdm_interf_kernel<N>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(wofdm_interf_kernel<N>, dim3(jobs), dim3(W * 64), lds, s, ip, wtx, wrx, h);
    return hipGetLastError();
}

#if WOFDM_TU_N <= 256
// Tx waveform + periodogram (row f4)
hipError_t psd_launch(int P, int mu, int rho, int overlap, int no_symbols, const float *wtx, const float2 *X, float2 *x,
                      int len, float *psd, hipStream_t s)
{
    constexpr int N = WOFDM_TU_N, FL = 8 * N, M = FL == 2048 ? 1024 : FL;
    wofdm_wparams wp;
    wp.P = P; wp.mu = mu; wp.rho = rho; wp.overlap = overlap; wp.no_symbols = no_symbols; wp.x = x;
    const size_t lds_a = 8 * (size_t)N * 17, lds_b = 8 * (size_t)M * 9;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(wofdm_psd_kernel<FL>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(wofdm_txwave_kernel<N>, dim3((no_symbols + 15) / 16), dim3(1024), lds_a, s, wp, wtx, X);
    hipLaunchKernelGGL(wofdm_psd_kernel<FL>, dim3(1), dim3(512), lds_b, s, (const float2 *)x, len, (len + FL - 1) / FL, psd);
    return hipGetLastError();
}
#endif

// the same for a batch of jobs (wofdm_tx_psd_batch), every DFT length; x zeroed by the caller, partial [n_items][8 N]
hipError_t psd_batch_launch(int n_jobs, int no_symbols, int n_items, const wofdm_bjob *jobs, const wofdm_bitem *items,
                            const float *wtx, const float2 *X, float2 *x, float *partial, float *psd, hipStream_t s)
{
    constexpr int N = WOFDM_TU_N, FL = 8 * N, M = FL / wofdm_psd_batch_r(N), WW = bwave_geo<N>::WAVES;
    const size_t lds_a = 8 * (size_t)N * (1 + WW), lds_b = 8 * (size_t)M * 9;
    static_assert(8 * N * (1 + WW) <= 160 * 1024 && 8 * M * 9 <= 160 * 1024, "LDS");
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(wofdm_txwave_batch_kernel<N>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_a);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(wofdm_psd_batch_kernel<FL>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(wofdm_txwave_batch_kernel<N>, dim3((no_symbols + WW - 1) / WW, n_jobs), dim3(WW * 64), lds_a, s, jobs,
                       no_symbols, wtx, X, x);
    hipLaunchKernelGGL(wofdm_psd_batch_kernel<FL>, dim3(n_items), dim3(512), lds_b, s, jobs, items, (const float2 *)x, partial);
    hipLaunchKernelGGL(wofdm_psd_reduce_kernel<FL>, dim3((FL + 255) / 256, n_jobs), dim3(256), 0, s, jobs,
                       (const float *)partial, psd);
    return hipGetLastError();
}

// wofdm_tx_psd_batch_masked: the unmasked jobs' waveforms by wofdm_txwave_batch_kernel, the masked ones by the fast-convolution
// kernel and its gather, then periodogram and reduction of all jobs as in psd_batch_launch
// (pa, power: the amplifier of wofdm_tx_psd_batch_pa between the waveforms and the periodogram, or null)
hipError_t psd_batch_masked_impl(int n_jobs, int no_symbols, int n_items, const wofdm_bjob *jobs, const wofdm_bitem *items,
                                 int n_plain, const wofdm_bjob *plain_jobs, int n_masked, const wofdm_mjob *mjobs, int max_len,
                                 const float2 *spec, float2 *Y, const float *wtx, const float2 *X, float2 *x, float *partial,
                                 float *psd, const wofdm_pajob *pa, float *power, hipStream_t s)
{
    constexpr int N = WOFDM_TU_N, FL = 8 * N, M = FL / wofdm_psd_batch_r(N), WW = bwave_geo<N>::WAVES, G = bmask_geo<N>::G;
    const size_t lds_a = 8 * (size_t)N * (1 + WW), lds_b = 8 * (size_t)M * 9, lds_m = bmask_geo<N>::LDS;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(wofdm_txwave_batch_kernel<N>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_a);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(wofdm_psd_batch_kernel<FL>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(wofdm_txmask_batch_kernel<N>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_m);
    if (e != hipSuccess) return e;
    if (n_plain > 0)
        hipLaunchKernelGGL(wofdm_txwave_batch_kernel<N>, dim3((no_symbols + WW - 1) / WW, n_plain), dim3(WW * 64), lds_a, s,
                           plain_jobs, no_symbols, wtx, X, x);
    if (n_masked > 0) {
        hipLaunchKernelGGL(wofdm_txmask_batch_kernel<N>, dim3((no_symbols + G - 1) / G, n_masked), dim3(512), lds_m, s, jobs,
                           mjobs, no_symbols, wtx, X, spec, Y);
        hipLaunchKernelGGL(wofdm_txmask_ola_kernel<N>, dim3((max_len + 255) / 256, n_masked), dim3(256), 0, s, jobs, mjobs,
                           no_symbols, (const float2 *)Y, x);
    }
    if (pa != nullptr) {
        hipLaunchKernelGGL(wofdm_pa_job_power_kernel, dim3(n_jobs), dim3(1024), 0, s, jobs, (const float2 *)x, power);
        hipLaunchKernelGGL(wofdm_pa_job_apply_kernel, dim3(n_jobs), dim3(1024), 0, s, jobs, pa, x, power);
    }
    hipLaunchKernelGGL(wofdm_psd_batch_kernel<FL>, dim3(n_items), dim3(512), lds_b, s, jobs, items, (const float2 *)x, partial);
    hipLaunchKernelGGL(wofdm_psd_reduce_kernel<FL>, dim3((FL + 255) / 256, n_jobs), dim3(256), 0, s, jobs,
                       (const float *)partial, psd);
    return hipGetLastError();
}
hipError_t psd_batch_masked_launch(int n_jobs, int no_symbols, int n_items, const wofdm_bjob *jobs, const wofdm_bitem *items,
                                   int n_plain, const wofdm_bjob *plain_jobs, int n_masked, const wofdm_mjob *mjobs, int max_len,
                                   const float2 *spec, float2 *Y, const float *wtx, const float2 *X, float2 *x, float *partial,
                                   float *psd, hipStream_t s)
{
    return psd_batch_masked_impl(n_jobs, no_symbols, n_items, jobs, items, n_plain, plain_jobs, n_masked, mjobs, max_len, spec, Y,
                                 wtx, X, x, partial, psd, nullptr, nullptr, s);
}
// wofdm_tx_psd_batch_pa (wofdm_pa_fns)
hipError_t psd_batch_pa_launch(int n_jobs, int no_symbols, int n_items, const wofdm_bjob *jobs, const wofdm_bitem *items,
                               int n_plain, const wofdm_bjob *plain_jobs, int n_masked, const wofdm_mjob *mjobs, int max_len,
                               const float2 *spec, float2 *Y, const float *wtx, const float2 *X, float2 *x, float *partial,
                               float *psd, const wofdm_pajob *pa, float *power, hipStream_t s)
{
    if (pa == nullptr || power == nullptr) return hipErrorInvalidValue;
    return psd_batch_masked_impl(n_jobs, no_symbols, n_items, jobs, items, n_plain, plain_jobs, n_masked, mjobs, max_len, spec, Y,
                                 wtx, X, x, partial, psd, pa, power, s);
}

// wofdm_interference_masked: the pulses of every pair, then the (pair, channel) jobs
hipError_t interf_masked_launch(int pairs, int n_ch, int P, int B, int mu, int delta, int gam, int kap, int JP, const float *wtx,
                                const float *wrx, const float2 *h, const float2 *g, const uint8_t *amask, float2 *cols,
                                float *power, float *wanted, hipStream_t s)
{
    constexpr int N = WOFDM_TU_N, W = interfm_geo<N>::WAVES, PW = interfm_geo<N>::PWAVES;
    wofdm_mparams mp;
    mp.P = P; mp.B = B; mp.mu = mu; mp.delta = delta; mp.gam = gam; mp.kap = kap; mp.n_ch = n_ch;
    mp.J = B + P - 1; mp.JP = JP;
    mp.power = power; mp.wanted = wanted;
    // the row of a wave holds three periods: 3 B <= 64 RB3, and the pulse with the channel ends within them
    if (3 * B > 64 * interfm_geo<N>::RB3 || mp.J + WOFDM_LT - 1 > 3 * B || JP < mp.J || delta > 64) return hipErrorInvalidValue;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(wofdm_interf_pulse_kernel<N>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, interfm_geo<N>::PLDS);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(wofdm_interf_masked_kernel<N>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, interfm_geo<N>::LDS);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(wofdm_interf_pulse_kernel<N>, dim3((mp.J + PW - 1) / PW, pairs), dim3(PW * 64), interfm_geo<N>::PLDS, s,
                       mp, wtx, g, amask, cols);
    hipLaunchKernelGGL(wofdm_interf_masked_kernel<N>, dim3(pairs * n_ch), dim3(W * 64), interfm_geo<N>::LDS, s, mp, wrx, h,
                       amask, (const float2 *)cols);
    return hipGetLastError();
}

// The Tx chain of one chunk (wofdm_tx_papr, wofdm_rx_profile): grids and job tables, then the jobs' waveforms
// (wofdm_txwave_batch_kernel onto a zeroed x, or the fast-convolution kernel and its gather, which writes every sample of x)
hipError_t tx_chain_launch(const wofdm_pparams &p, hipStream_t s)
{
    constexpr int N = WOFDM_TU_N, WW = bwave_geo<N>::WAVES, G = bmask_geo<N>::G;
    const int S = p.S, T = p.beta + S * (p.P - p.beta), bps = N * wofdm_kslot(p.k) / 128;
    const bool masked = p.spec != nullptr;
    if (p.n_jobs < 1 || p.n_jobs > WOFDM_PAPR_MAX_JOBS || p.frames < 1 || p.wdiv < 1 ||
        p.cp > N || p.cs > N || 2 * p.beta > p.P || (masked && (p.P > bmask_geo<N>::PMAX || p.mjobs == nullptr || p.Y == nullptr)))
        return hipErrorInvalidValue;
    const size_t lds_a = 8 * (size_t)N * (1 + WW), lds_m = bmask_geo<N>::LDS;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(wofdm_txwave_batch_kernel<N>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_a);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(wofdm_txmask_batch_kernel<N>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_m);
    if (e == hipSuccess && !masked) e = hipMemsetAsync(p.x, 0, (size_t)p.n_jobs * T * sizeof(float2), s);
    if (e != hipSuccess) return e;
    const unsigned n_blk = (unsigned)p.n_jobs * (unsigned)(S * bps);
    hipLaunchKernelGGL(wofdm_papr_gen_kernel<N>, dim3((n_blk + 255) / 256), dim3(256), 0, s, p);
    if (!masked) {
        hipLaunchKernelGGL(wofdm_txwave_batch_kernel<N>, dim3((S + WW - 1) / WW, p.n_jobs), dim3(WW * 64), lds_a, s,
                           (const wofdm_bjob *)p.jobs, S, p.wtx, (const float2 *)p.X, p.x);
    } else {
        hipLaunchKernelGGL(wofdm_txmask_batch_kernel<N>, dim3((S + G - 1) / G, p.n_jobs), dim3(512), lds_m, s,
                           (const wofdm_bjob *)p.jobs, (const wofdm_mjob *)p.mjobs, S, p.wtx, (const float2 *)p.X, p.spec, p.Y);
        hipLaunchKernelGGL(wofdm_txmask_ola_kernel<N>, dim3((T + 255) / 256, p.n_jobs), dim3(256), 0, s,
                           (const wofdm_bjob *)p.jobs, (const wofdm_mjob *)p.mjobs, S, (const float2 *)p.Y, p.x);
    }
    return hipGetLastError();
}

// wofdm_tx_papr, one chunk: the Tx chain, then the periods
hipError_t papr_launch(const wofdm_pparams *pp, hipStream_t s)
{
    const wofdm_pparams &p = *pp;
    if (p.n_bins < 1 || p.n_bins > WOFDM_PAPR_MAX_BINS) return hipErrorInvalidValue;
    const hipError_t e = tx_chain_launch(p, s);
    if (e != hipSuccess) return e;
    const int S = p.S;
    // (at most two workgroups per CU's worth: a workgroup then flushes its histogram once per 256 periods or more)
    constexpr unsigned BATCH = WOFDM_PAPR_WAVES * WOFDM_PAPR_PER_WAVE;
    const unsigned n_batches = ((unsigned)p.n_jobs * (unsigned)S + BATCH - 1) / BATCH;
    hipLaunchKernelGGL(wofdm_papr_period_kernel, dim3(n_batches < 512u ? n_batches : 512u), dim3(WOFDM_PAPR_WAVES * 64),
                       4 * (size_t)(p.n_bins + 1), s, p);
    return hipGetLastError();
}

// What the chunk of a receive profile (wofdm_rxchunk) has to satisfy, stage by stage.  The chunk of r is the chunk of pp's Tx
// chain, within the receive kernel's geometry:
bool rxprof_args_ok(const wofdm_pparams *pp, const wofdm_rparams &r)
{
    constexpr int N = WOFDM_TU_N;
    return !(r.n_jobs != pp->n_jobs || r.item0 != pp->item0 || r.frames != pp->frames || r.delta < 0 || r.delta > 64 || (r.delta & 1) ||
             r.gam < 0 || r.B != N + r.delta + r.gam || r.T != pp->beta + r.S * r.B || r.NL > r.T + WOFDM_LT - 1 || r.n_ch < 1 ||
             r.n_snr < 1);
}
// the arms with a point loop: the points, the per-symbol partials and totals, and the chunk's cells within the totals
bool rxprof_points_ok(const wofdm_sparams &sp, const wofdm_rparams &r, int max_points)
{
    return !(sp.n_points < 1 || sp.n_points > max_points || sp.sym_pow == nullptr || sp.sym_cnt == nullptr || sp.sym_errs == nullptr ||
             sp.sym_tot == nullptr || r.S < 2 || r.S > 64 || (r.item0 + (uint64_t)r.n_jobs - 1) / r.frames >= sp.cells);
}
// the cells the chunk's items touch: the first, and how many
unsigned rxprof_cells(const wofdm_rparams &r, uint64_t &cell0)
{
    cell0 = r.item0 / r.frames;
    return (unsigned)((r.item0 + (uint64_t)r.n_jobs - 1) / r.frames - cell0 + 1);
}
// the neighbour: the victim's chunk and frame geometry with S + 1 symbols, tables and buffers of its own; own_offset: the offset
// is the call's (wofdm_rx_profile_aci), not the points'
bool rxprof_nb_ok(const wofdm_rxchunk &c, bool own_offset)
{
    const wofdm_pparams &p = c.tx, &nb = c.nb;
    const wofdm_rparams &r = c.r;
    const wofdm_aparams &a = c.a;
    return !(nb.n_jobs != p.n_jobs || nb.item0 != p.item0 || nb.frames != p.frames || nb.frame_offset != p.frame_offset ||
             nb.S != r.S + 1 || nb.P != p.P || nb.beta != p.beta || nb.cp != p.cp || nb.cs != p.cs || nb.wdiv != p.wdiv ||
             a.Ti != r.T + r.B || (own_offset && (a.ioff < 1 || a.ioff > r.B)) || a.xi != nb.x || a.hi == nullptr || nb.X == p.X ||
             nb.x == p.x || nb.jobs == p.jobs);
}
// the knots fit the LDS image and cover every sample either pass takes a tap at -- late: a window max_theta samples late reaches
// further, by less than a stride --; the indices stay exact in single precision
bool rxprof_knots_ok(const wofdm_dparams &dp, const wofdm_rparams &r, bool late, int max_theta)
{
    return !(dp.knots == nullptr || dp.n_knots < 2 || dp.n_knots > WOFDM_DOPPLER_KNOTS || dp.knot_step < 1 ||
             r.T + (late ? r.B : 0) + WOFDM_LT >= (1 << 22) ||
             (int64_t)(dp.n_knots - 1) * dp.knot_step < (int64_t)(r.NL > r.T ? r.NL : r.T) - 1 + max_theta);
}
// the amplifier: a point of its own per point of sp, and a saturation table that covers the pair of every cell of the chunk
bool rxprof_pa_ok(const wofdm_rxchunk &c)
{
    const wofdm_paparams &pa = c.pa;
    uint64_t cell0;
    const unsigned n_cells = rxprof_cells(c.r, cell0);
    return !(pa.n_points != c.sp.n_points || pa.pairs < 1 || pa.pts == nullptr || pa.asat == nullptr || pa.y == nullptr ||
             pa.pwr == nullptr || pa.pwr_tot == nullptr || c.r.x != c.tx.x || (cell0 + n_cells - 1) / c.tx.wdiv >= (uint64_t)pa.pairs);
}
// the demapper: its scales and scratch
bool rxprof_soft_ok(const wofdm_softparams &so)
{
    return !(so.n_scales < 1 || so.n_scales > WOFDM_SOFT_SCALES || so.w2 == nullptr || so.bit_part == nullptr ||
             so.sym_part == nullptr || so.bit_tot == nullptr || so.sym_tot == nullptr);
}
// the ordered sums of the chunk onto the totals: per point of sp, or (null) the plain ones
void rxprof_reduce_launch(const wofdm_rparams &r, const wofdm_sparams *sp, hipStream_t s)
{
    constexpr int N = WOFDM_TU_N;
    uint64_t cell0;
    const unsigned n_cells = rxprof_cells(r, cell0);
    if (sp == nullptr)
        hipLaunchKernelGGL(wofdm_rxprof_reduce_kernel<N>, dim3(N / 64, n_cells), dim3(64), 0, s, r, cell0);
    else
        hipLaunchKernelGGL(wofdm_rxprof_sync_reduce_kernel<N>, dim3(N / 64 + 1, n_cells, (unsigned)sp->n_points), dim3(64), 0, s, r,
                           *sp, cell0);
}

// One chunk of a receive profile, whichever of the entry points it belongs to (wofdm_link.h): the stages the arm switches
// on are checked, then enqueued in the one order there is -- the Tx chain of the chunk's (cell, frame) items; the neighbour's;
// the points' amplified waveforms and power sums; the items' unit phase walks; the arm's receive kernel; the ordered sums
// (per point where the arm has points); the amplifier's power sums in frame order; the demapper's ordered sums behind the others.
hipError_t rx_profile_chunk(const wofdm_rxchunk *cp, hipStream_t s)
{
    constexpr int N = WOFDM_TU_N;
    // the most points an arm's kernel takes (the arms without a point loop: none)
    constexpr int MAX_POINTS[] = {0, 0, WOFDM_SYNC_POINTS, WOFDM_DOPPLER_TRACKS, WOFDM_PA_POINTS, WOFDM_PN_POINTS, WOFDM_LINK_POINTS};
    const wofdm_rxchunk &c = *cp;
    const wofdm_rparams &r = c.r;
    if (c.arm < RXP_PLAIN || c.arm > RXP_LINK) return hipErrorInvalidValue;
    const bool link = c.arm == RXP_LINK, points = MAX_POINTS[c.arm] > 0;
    const bool nb = c.arm == RXP_ACI || (link && c.nb_on), sync = c.arm == RXP_SYNC || link, knots = c.arm == RXP_DOPPLER || link;
    const bool amp = c.arm == RXP_PA || link, walk = c.arm == RXP_PN || link, soft = link && c.soft_on, track = soft && c.track_on;
    const bool code = track && c.code_on, frame = code && c.frame_on, ldpc = code && !frame && c.ldpc_on;
    const bool coset = code && !frame && !ldpc && c.coset_on;
    if (nb != c.nb_on || soft != c.soft_on || track != c.track_on || code != c.code_on || frame != c.frame_on || ldpc != c.ldpc_on ||
        coset != c.coset_on || (code && !frame && !ldpc && !coset && !wofdm_viterbi_ok(c.cd, true)) ||
        ((frame || ldpc) && (c.cd.soft == nullptr || !(c.cd.llr_scale > 0.f) || c.cd.n_codes < 1 || c.cd.n_codes > WOFDM_CODE_CODES)) ||
        (coset && (c.cd.soft == nullptr || !(c.cd.llr_scale > 0.f) || c.cs_nv < 0 || c.cs_nv > WOFDM_CODE_CODES || c.cs_nl < 0 ||
                   c.cs_nl > WOFDM_CODE_CODES || c.cs_nv + c.cs_nl < 1)) ||
        c.hq_rounds < 0 || c.hq_rounds > WOFDM_HARQ_ROUNDS ||
        (c.hq_rounds > 0 && (!coset || c.cs_nv != 0 || r.n_jobs % c.hq_rounds != 0 || r.item0 % (uint64_t)c.hq_rounds != 0 ||
                             r.frames % (uint64_t)c.hq_rounds != 0)) ||
        (track && (c.tk.pts == nullptr || r.S > 64)) || !rxprof_args_ok(&c.tx, r) || (points && !rxprof_points_ok(c.sp, r, MAX_POINTS[c.arm])) ||
        (nb && !rxprof_nb_ok(c, !link)) || (sync && (c.sp.pts == nullptr || c.sp.base == nullptr)) ||
        (knots && !rxprof_knots_ok(c.dp, r, link, link ? c.max_theta : 0)) || (amp && !rxprof_pa_ok(c)) ||
        // (rxprof_args_ok: B = N + delta + gam, so the last sample under the last window is the walk's last, index S B - 1)
        (walk && (c.pn.pts == nullptr || c.pn.walk == nullptr)) ||
        (link && (c.lk.pts == nullptr || c.n_tracks < 1 || c.max_theta < 0 || c.max_theta >= r.B)) || (soft && !rxprof_soft_ok(c.soft)))
        return hipErrorInvalidValue;
    uint64_t cell0;
    const unsigned n_cells = rxprof_cells(r, cell0);
    hipError_t e = tx_chain_launch(c.tx, s);
    if (e == hipSuccess && nb) e = tx_chain_launch(c.nb, s);
    if (e != hipSuccess) return e;
    // the arm's kernel with its LDS, behind what it reads: the points' waveforms, the walks
    const auto receive = [&](auto kernel, int lds, const auto &...args) {
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return;
        if (amp)
            hipLaunchKernelGGL(wofdm_pa_wave_kernel, dim3((unsigned)r.n_jobs, (unsigned)c.pa.n_points), dim3(256), 0, s, c.pa, r.x, r.T,
                               r.item0, r.frames, c.tx.wdiv);
        if (walk)
            hipLaunchKernelGGL(wofdm_pn_walk_kernel, dim3((unsigned)r.n_jobs), dim3(1024), 0, s, c.pn.walk, r.S * r.B, r.seed_lo, r.seed_hi,
                               r.item0, r.frames, r.frame_offset);
        hipLaunchKernelGGL(kernel, dim3((unsigned)r.n_jobs), dim3(rxp_geo<N>::WAVES * 64), lds, s, r, args...);
    };
    switch (c.arm) {
    case RXP_PLAIN: receive(wofdm_rxprof_kernel<N>, rxp_geo<N>::LDS); break;
    case RXP_ACI: receive(wofdm_rxprof_aci_kernel<N>, rxp_geo<N>::LDS_ACI, c.a); break;
    case RXP_SYNC: receive(wofdm_rxprof_sync_kernel<N>, rxp_geo<N>::LDS, c.sp); break;
    case RXP_DOPPLER: receive(wofdm_rxprof_doppler_kernel<N>, rxp_geo<N>::LDS_DOP, c.sp, c.dp); break;
    case RXP_PA: receive(wofdm_rxprof_pa_kernel<N>, rxp_geo<N>::LDS, c.sp, c.pa); break;
    case RXP_PN: receive(wofdm_rxprof_pn_kernel<N>, rxp_geo<N>::LDS, c.sp, c.pn); break;
    default:
        if (code)
            receive(wofdm_rxprof_coded_kernel<N>, rxp_geo<N>::LDS_TRACK, c.a, c.sp, c.dp, c.pa, c.pn, c.lk, c.soft, c.tk, c.cd);
        else if (track)
            receive(wofdm_rxprof_tracking_kernel<N>, rxp_geo<N>::LDS_TRACK, c.a, c.sp, c.dp, c.pa, c.pn, c.lk, c.soft, c.tk);
        else if (soft)
            receive(wofdm_rxprof_soft_kernel<N>, rxp_geo<N>::LDS_LINK, c.a, c.sp, c.dp, c.pa, c.pn, c.lk, c.soft);
        else
            receive(wofdm_rxprof_link_kernel<N>, rxp_geo<N>::LDS_LINK, c.a, c.sp, c.dp, c.pa, c.pn, c.lk);
    }
    if (e != hipSuccess) return e;
    rxprof_reduce_launch(r, points ? &c.sp : nullptr, s);
    if (amp)
        hipLaunchKernelGGL(wofdm_pa_power_reduce_kernel, dim3(n_cells), dim3(64), 0, s, c.pa, r.item0, r.n_jobs, r.frames, c.sp.cells,
                           cell0);
    if (soft) {
        const size_t n_elems = (size_t)r.n_jobs * (size_t)c.sp.n_points * (size_t)c.soft.n_scales * N;
        hipLaunchKernelGGL(wofdm_rxprof_soft_frame_kernel<N>, dim3((unsigned)((n_elems + 255) / 256)), dim3(256), 0, s, c.soft, r.S,
                           n_elems);
        hipLaunchKernelGGL(wofdm_rxprof_soft_reduce_kernel<N>, dim3(N / 64 + 1, n_cells, (unsigned)(c.sp.n_points * c.soft.n_scales)),
                           dim3(64), 0, s, r, c.sp, c.soft, cell0);
    }
    if (frame) {
        // the decoder behind the soft bits: one wave per (frame, point), one launch per code -- they share the history
        wofdm_longparams lp = c.fr;
        lp.soft = c.cd.soft;
        lp.cw_stride = (int64_t)(r.S - 1) * N * 8;
        lp.pts = c.tk.pts; lp.n_points = c.sp.n_points; lp.n_codes = c.cd.n_codes;
        lp.item0 = r.item0; lp.frames = r.frames; lp.cells = c.sp.cells;
        lp.bits = nullptr; lp.metric = nullptr;
        lp.n_cw = (uint32_t)r.n_jobs * (uint32_t)lp.n_points;
        for (int i = 0; i < lp.n_codes; ++i) {
            lp.rate = c.cd.rate[i]; lp.code = i;
            lp.steps[0] = c.fr_steps[i][0]; lp.steps[1] = c.fr_steps[i][1];
            const hipError_t le = wofdm_viterbi_long_enqueue(lp, true, s);
            if (le != hipSuccess) return le;
        }
    } else if (ldpc) {
        // the decoder behind the soft bits: one workgroup per (frame, point, word of the frame), one launch per code
        wofdm_ldpcparams lp = c.ld;
        lp.soft = c.cd.soft;
        lp.cw_stride = (int64_t)(r.S - 1) * N * 8;
        lp.pts = c.tk.pts; lp.n_points = c.sp.n_points; lp.n_codes = c.cd.n_codes;
        lp.item0 = r.item0; lp.frames = r.frames; lp.cells = c.sp.cells;
        lp.bits = nullptr; lp.iters = nullptr; lp.conv = nullptr;
        lp.n_cw = (uint32_t)r.n_jobs * (uint32_t)lp.n_points;
        for (int i = 0; i < lp.n_codes; ++i) {
            lp.J = c.ld_code[i][0]; lp.L = c.ld_code[i][1]; lp.max_iter = c.ld_code[i][2]; lp.code = i;
            lp.Z[0] = c.ld_Z[i][0]; lp.Z[1] = c.ld_Z[i][1];
            const hipError_t le = wofdm_ldpc_enqueue(lp, true, s);
            if (le != hipSuccess) return le;
        }
    } else if (coset) {
        // both decoders behind the same soft bits, in the coset view: the frame launches' and the LDPC launches' parameters as
        // above, one launch per code, the Viterbi codes first
        wofdm_longparams fp = c.fr;
        fp.soft = c.cd.soft;
        fp.cw_stride = (int64_t)(r.S - 1) * N * 8;
        fp.pts = c.tk.pts; fp.n_points = c.sp.n_points; fp.n_codes = c.cs_nv;
        fp.item0 = r.item0; fp.frames = r.frames; fp.cells = c.sp.cells;
        fp.bits = nullptr; fp.metric = nullptr;
        fp.n_cw = (uint32_t)r.n_jobs * (uint32_t)fp.n_points;
        for (int i = 0; i < c.cs_nv; ++i) {
            fp.rate = c.cd.rate[i]; fp.code = i;
            fp.steps[0] = c.fr_steps[i][0]; fp.steps[1] = c.fr_steps[i][1];
            const hipError_t le = wofdm_viterbi_coset_enqueue(fp, c.cs, s);
            if (le != hipSuccess) return le;
        }
        wofdm_ldpcparams lp = c.ld;
        lp.soft = c.cd.soft;
        lp.cw_stride = fp.cw_stride;
        lp.pts = c.tk.pts; lp.n_points = c.sp.n_points; lp.n_codes = c.cs_nl;
        lp.item0 = r.item0; lp.frames = r.frames; lp.cells = c.sp.cells;
        lp.bits = nullptr; lp.iters = nullptr; lp.conv = nullptr;
        lp.n_cw = fp.n_cw;
        for (int i = 0; i < c.cs_nl; ++i) {
            lp.J = c.ld_code[i][0]; lp.L = c.ld_code[i][1]; lp.max_iter = c.ld_code[i][2]; lp.code = i;
            lp.Z[0] = c.ld_Z[i][0]; lp.Z[1] = c.ld_Z[i][1];
            hipError_t le;
            if (c.hq_rounds > 0) {
                // retransmissions: one workgroup per group of hq_rounds frames, point and word
                wofdm_ldpcparams gp = lp;
                gp.n_cw = (uint32_t)(r.n_jobs / c.hq_rounds) * (uint32_t)lp.n_points;
                const wofdm_harqparams hq = {c.hq_rounds, c.hq_combine, nullptr};
                le = wofdm_ldpc_harq_enqueue(gp, c.cs, hq, true, s);
            } else {
                le = wofdm_ldpc_coset_enqueue(lp, c.cs, s);
            }
            if (le != hipSuccess) return le;
        }
    } else if (code) {
        // the decoder behind the soft bits: one wave per (frame, point, data symbol) and code
        wofdm_codeparams cd = c.cd;
        cd.cw_stride = (int64_t)N * 8;
        cd.pts = c.tk.pts; cd.n_points = c.sp.n_points; cd.S1 = r.S - 1;
        cd.item0 = r.item0; cd.frames = r.frames; cd.cells = c.sp.cells;
        cd.bits = nullptr; cd.metric = nullptr;
        cd.n_cw = (uint32_t)r.n_jobs * (uint32_t)cd.n_points * (uint32_t)cd.S1;
        wofdm_viterbi_enqueue(cd, s);
    }
    return hipGetLastError();
}

}  // namespace

const wofdm_pa_fns *WOFDM_CAT(wofdm_aux_pa_n, WOFDM_TU_N)(void)
{
    static const wofdm_pa_fns fns = {psd_batch_pa_launch};
    return &fns;
}

const wofdm_link_fns *WOFDM_CAT(wofdm_aux_link_n, WOFDM_TU_N)(void)
{
    static const wofdm_link_fns fns = {rx_profile_chunk};
    return &fns;
}

// The five rx_profile* members behind papr stay null and nothing reads them: every receive profile goes through
// wofdm_link_fns::rx_profile_chunk.  Their declarations are in wofdm_kernel.h, a file of the frame kernels' source hash, and
// leave with the next change that re-stamps profiles/hbm_traffic.json anyway.
const wofdm_aux_fns *WOFDM_CAT(wofdm_aux_n, WOFDM_TU_N)(void)
{
#if WOFDM_TU_N <= 256
    static const wofdm_aux_fns fns = {interf_launch, interf_masked_launch, psd_launch, psd_batch_launch, psd_batch_masked_launch,
                                      papr_launch};
#else
    static const wofdm_aux_fns fns = {interf_launch, interf_masked_launch, nullptr, psd_batch_launch, psd_batch_masked_launch,
                                      papr_launch};
#endif
    return &fns;
}

#if WOFDM_TU_N == 64
hipError_t wofdm_philox_kat_launch(const uint32_t *ctr_key_dev, uint32_t *out_dev, hipStream_t s)
{
    hipLaunchKernelGGL(philox_kat_kernel, dim3(1), dim3(64), 0, s, ctr_key_dev, out_dev);
    return hipGetLastError();
}
#endif
