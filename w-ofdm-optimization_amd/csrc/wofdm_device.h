// Device primitives shared by the frame kernel (wofdm_kernel.hip) and the auxiliary kernels (wofdm_aux.hip): packed complex
// arithmetic, the in-register DFTs, the wave's FFT through LDS with its twiddle tables, and the VALU FIR.
#pragma once
#include "wofdm_kernel.h"

namespace {

// Complex samples are 2-wide float vectors: gfx950 issues one wave64 VALU instruction per
// ~4 cycles per SIMD whether it is v_fma_f32 or v_pk_fma_f32 (tools/ubench/valu_rate.hip:
// 4.5 vs 5.1 cycles), so the fp32 peak is only reachable with packed math, and complex
// arithmetic packs naturally as (re, im).
// That price holds with the matrix pipe idle.  Beside MFMAs a packed fp32 instruction waits for the pipe where a plain one issues
// under it (tools/ubench/valu_beside_mfma.hip, profiles/packed_beside_mfma.txt: 13 v_pk_fma_f32 behind each MFMA of a wave cost
// 57 cycles per MFMA more than alone, 13 v_fma_f32 24), so the matrix-pipe FIR's kernels write the arithmetic that sits between and
// right behind their tile's MFMAs per component (fma2 / mul2 below) -- the sites an A/B of correct builds confirmed, no others.
typedef float v2f __attribute__((ext_vector_type(2)));

__device__ __forceinline__ v2f mk(float x, float y) { return (v2f){x, y}; }

// a b + c and a w per component: the two IEEE operations of v_pk_fma_f32 / v_pk_mul_f32 as plain instructions (-fno-slp-vectorize:
// nothing packs them again)
__device__ __forceinline__ v2f fma2(v2f a, v2f b, v2f c) { return mk(__builtin_fmaf(a.x, b.x, c.x), __builtin_fmaf(a.y, b.y, c.y)); }
__device__ __forceinline__ v2f mul2(v2f a, float w) { return mk(a.x * w, a.y * w); }

__device__ __forceinline__ v2f ldg2(const float2 *p) { const float2 t = *p; return mk(t.x, t.y); }

__device__ __forceinline__ void wave_sync()
{
    // LDS traffic between lanes of ONE wave: DS ops execute in issue order, so only the
    // compiler has to be kept from reordering across this point.
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// a * w  (2 packed instructions; swizzle and sign live in the VOP3P modifiers)
__device__ __forceinline__ v2f cmul(v2f a, v2f w)
{
    v2f t, r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(t) : "v"(a), "v"(w));
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]"
        : "=v"(r) : "v"(a), "v"(w), "v"(t));
    return r;
}
// a * conj(w)
__device__ __forceinline__ v2f cmul_conj(v2f a, v2f w)
{
    v2f t, r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1] neg_hi:[0,1]" : "=v"(t) : "v"(a), "v"(w));
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1]"
        : "=v"(r) : "v"(a), "v"(w), "v"(t));
    return r;
}
// a + (-i) d = (a.x + d.y, a.y - d.x)   and   a + (+i) d = (a.x - d.y, a.y + d.x)
__device__ __forceinline__ v2f add_mi(v2f a, v2f d)
{
    v2f r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(d));
    return r;
}
__device__ __forceinline__ v2f add_pi(v2f a, v2f d)
{
    v2f r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(r) : "v"(a), "v"(d));
    return r;
}
// tw tables hold exp(-2 pi i ...): the forward DFT multiplies by them, the inverse by the conjugate
template <int DIR> __device__ __forceinline__ v2f twid(v2f a, v2f w)
{
    return DIR < 0 ? cmul(a, w) : cmul_conj(a, w);
}

// qammod(label) of the frame kernel's constellation table (Gray, unit average power; main_BER_calculation.m:248-249) for k = 2,
// 4, 6 bits: the same integers times the same fp32 scale, so the same bits.
__device__ __forceinline__ v2f qam_point(int k, uint32_t label)
{
    const int hb = k >> 1, mm = (1 << hb) - 1;
    const float qs = k == 2 ? 0.70710678118654752f : (k == 4 ? 0.31622776601683794f : 0.15430334996209191f);
    const uint32_t gi = label >> hb, gq = label & (uint32_t)mm;
    const int li = (int)(gi ^ (gi >> 1) ^ (gi >> 2)), lq = (int)(gq ^ (gq >> 1) ^ (gq >> 2));
    return mk((float)(2 * li - mm), (float)(mm - 2 * lq)) * qs;
}

template <int DIR> __device__ __forceinline__ void radix4(v2f (&u)[4])
{
    const v2f a0 = u[0] + u[2], a1 = u[0] - u[2];
    const v2f a2 = u[1] + u[3], d = u[1] - u[3];
    u[0] = a0 + a2;
    u[2] = a0 - a2;
    u[1] = DIR < 0 ? add_mi(a1, d) : add_pi(a1, d);      // a1 + (-+ i) d
    u[3] = DIR < 0 ? add_pi(a1, d) : add_mi(a1, d);      // a1 - (-+ i) d
}

template <int N> struct geo {
    static constexpr int NQ = N / 4;                 // radix-4 butterflies per stage
    static constexpr int BPL = (NQ + 63) / 64;       // ... per lane
    static constexpr int RB = N / 64 + 1;            // FIR outputs per lane
    static constexpr bool FULL = NQ >= 64 * BPL;     // every lane owns BPL butterflies
    // Twiddle tables, one per stage after the first, laid out [k][r-1] so that the three
    // factors of a butterfly are adjacent and lanes hit distinct banks:
    //   radix-4 stage NS: 3*NS entries exp(-2 pi i r k / (4 NS));  radix-2 stage NS: NS entries.
    static constexpr int tw_off(int stage_ns)
    {
        // stages in execution order for this N (after the twiddle-free first stage)
        int off = 0, ns = 4;
        while (ns < stage_ns) {
            const bool r2 = (N == 128 && ns == 4) || (N == 512 && ns == 16);
            off += r2 ? ns : 3 * ns;
            ns *= r2 ? 2 : 4;
        }
        return off;
    }
};

// Stockham autosort stages on the wave's LDS slices.  Lane data v[u][q][r] always means element
// (lane + 64 q) + r N/4 of the wave's u-th symbol, both as the first stage's input and the last
// stage's output.  Every stage handles the wave's SPW symbols together (slices `sb` apart), so
// the independent transforms share one write->read turnaround per stage instead of queueing
// behind each other's fences.
template <int N, int DIR, int SPW>
__device__ __forceinline__ void fft_first(v2f (&v)[SPW][geo<N>::BPL][4], v2f *fb, int sb, int lane)
{
#pragma unroll
    for (int u = 0; u < SPW; ++u) {
#pragma unroll
        for (int q = 0; q < geo<N>::BPL; ++q) {
            const int j = lane + 64 * q;
            if (geo<N>::FULL || j < geo<N>::NQ) {
                radix4<DIR>(v[u][q]);
#pragma unroll
                for (int r = 0; r < 4; ++r) fb[u * sb + 4 * j + r] = v[u][q][r];
            }
        }
    }
    wave_sync();
}

template <int N, int NS, int DIR, int SPW>
__device__ __forceinline__ void fft_mid4(v2f *fb, int sb, const v2f *tw, int lane)
{
    v2f u4[SPW][geo<N>::BPL][4];
    const v2f *t = tw + geo<N>::tw_off(NS);
#pragma unroll
    for (int u = 0; u < SPW; ++u) {
#pragma unroll
        for (int q = 0; q < geo<N>::BPL; ++q) {
            const int j = lane + 64 * q;
            if (geo<N>::FULL || j < geo<N>::NQ) {
                const int k = j & (NS - 1);
#pragma unroll
                for (int r = 0; r < 4; ++r) u4[u][q][r] = fb[u * sb + j + r * geo<N>::NQ];
#pragma unroll
                for (int r = 1; r < 4; ++r) u4[u][q][r] = twid<DIR>(u4[u][q][r], t[3 * k + r - 1]);
                radix4<DIR>(u4[u][q]);
            }
        }
    }
    wave_sync();
#pragma unroll
    for (int u = 0; u < SPW; ++u) {
#pragma unroll
        for (int q = 0; q < geo<N>::BPL; ++q) {
            const int j = lane + 64 * q;
            if (geo<N>::FULL || j < geo<N>::NQ) {
                const int k = j & (NS - 1);
#pragma unroll
                for (int r = 0; r < 4; ++r) fb[u * sb + ((j - k) << 2) + k + r * NS] = u4[u][q][r];
            }
        }
    }
    wave_sync();
}

template <int N, int NS, int DIR, int SPW>
__device__ __forceinline__ void fft_mid2(v2f *fb, int sb, const v2f *tw, int lane)
{
    constexpr int NB = N / 2, PER = (NB + 63) / 64;
    v2f y0[SPW][PER], y1[SPW][PER];
    const v2f *t = tw + geo<N>::tw_off(NS);
#pragma unroll
    for (int u = 0; u < SPW; ++u) {
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int j = lane + 64 * q;
            if (j < NB) {
                const int k = j & (NS - 1);
                const v2f a = fb[u * sb + j];
                const v2f b = twid<DIR>(fb[u * sb + j + NB], t[k]);
                y0[u][q] = a + b; y1[u][q] = a - b;
            }
        }
    }
    wave_sync();
#pragma unroll
    for (int u = 0; u < SPW; ++u) {
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int j = lane + 64 * q;
            if (j < NB) {
                const int k = j & (NS - 1);
                fb[u * sb + ((j - k) << 1) + k] = y0[u][q];
                fb[u * sb + ((j - k) << 1) + k + NS] = y1[u][q];
            }
        }
    }
    wave_sync();
}

template <int N, int DIR, int SPW>
__device__ __forceinline__ void fft_last(v2f (&v)[SPW][geo<N>::BPL][4], const v2f *fb, int sb,
                                         const v2f *tw, int lane)
{
    const v2f *t = tw + geo<N>::tw_off(geo<N>::NQ);
#pragma unroll
    for (int u = 0; u < SPW; ++u) {
#pragma unroll
        for (int q = 0; q < geo<N>::BPL; ++q) {
            const int j = lane + 64 * q;
            if (geo<N>::FULL || j < geo<N>::NQ) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[u][q][r] = fb[u * sb + j + r * geo<N>::NQ];
#pragma unroll
                for (int r = 1; r < 4; ++r) v[u][q][r] = twid<DIR>(v[u][q][r], t[3 * j + r - 1]);
                radix4<DIR>(v[u][q]);
            }
        }
    }
    wave_sync();
}

// ---------------------------------------------------------------------------------------------
// N = 512 / 1024: three Stockham stages  R . R2 . R  with R = 8 / 16 points held by one lane
// (N = 8.8.8 = 16.4.16), i.e. two LDS round trips instead of four.  A lane owns elements
// lane + 64 t, t = q + BPL r -- exactly the inputs of butterfly `lane` of a first stage of radix
// R = 4 BPL (Ns = 1) and the outputs of butterfly `lane` of a last stage of radix R (Ns = 64),
// so natural order in and out survives.  The in-register R-point DFT is a radix-4 pass over r,
// constant twiddles, and a radix-4 (radix-2) pass over q.
//
// Twiddle table (fill_twiddles):  N = 1024: [0,48) stage 2 exp(-2 pi i r k/64) at [3k + r-1];
// [48,1008) stage 3 exp(-2 pi i t j/1024) at [48 + 15 j + t-1].  N = 512: [0,56) stage 2
// exp(-2 pi i t k/64) at [7k + t-1]; [56,504) stage 3 exp(-2 pi i t j/512) at [56 + 7j + t-1].
//
// Stage 1 stores R consecutive outputs per lane (stride R v2f across lanes: every lane on the same
// banks); the position inside each group of R is XOR-swizzled with the group number so that a
// store instruction spreads over all banks, and stage 2 undoes it when it loads.
template <int R> __device__ __forceinline__ int swz(int idx)
{
    constexpr int LG = R == 16 ? 4 : 3;
    const int a = idx >> LG;
    return idx ^ ((a ^ (a >> LG)) & (R - 1));
}

// x[q][r] = x_t, t = q + 4 r   ->   x[q][r] = X_u, u = r + 4 q     (16 points)
template <int DIR> __device__ __forceinline__ void dft16(v2f (&x)[4][4])
{
    constexpr float c1 = 0.92387953251128674f, s1 = 0.38268343236508977f, h = 0.70710678118654752f;
    // exp(-2 pi i m/16) for m = q c
    const v2f w1 = mk(c1, -s1), w2 = mk(h, -h), w3 = mk(s1, -c1), w4 = mk(0.f, -1.f), w6 = mk(-h, -h),
              w9 = mk(-c1, s1);
#pragma unroll
    for (int q = 0; q < 4; ++q) radix4<DIR>(x[q]);
    x[1][1] = twid<DIR>(x[1][1], w1); x[1][2] = twid<DIR>(x[1][2], w2); x[1][3] = twid<DIR>(x[1][3], w3);
    x[2][1] = twid<DIR>(x[2][1], w2); x[2][2] = twid<DIR>(x[2][2], w4); x[2][3] = twid<DIR>(x[2][3], w6);
    x[3][1] = twid<DIR>(x[3][1], w3); x[3][2] = twid<DIR>(x[3][2], w6); x[3][3] = twid<DIR>(x[3][3], w9);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        v2f col[4] = {x[0][c], x[1][c], x[2][c], x[3][c]};
        radix4<DIR>(col);
#pragma unroll
        for (int d = 0; d < 4; ++d) x[d][c] = col[d];
    }
}
// x[q][r] = x_t, t = q + 2 r   ->   x[q][r] = X_u, u = r + 4 q     (8 points)
template <int DIR> __device__ __forceinline__ void dft8(v2f (&x)[2][4])
{
    constexpr float h = 0.70710678118654752f;
    radix4<DIR>(x[0]);
    radix4<DIR>(x[1]);
    x[1][1] = twid<DIR>(x[1][1], mk(h, -h));
    x[1][2] = twid<DIR>(x[1][2], mk(0.f, -1.f));
    x[1][3] = twid<DIR>(x[1][3], mk(-h, -h));
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const v2f a = x[0][c], b = x[1][c];
        x[0][c] = a + b;
        x[1][c] = a - b;
    }
}
template <int N, int DIR> __device__ __forceinline__ void dft_lane(v2f (&x)[geo<N>::BPL][4])
{
    if constexpr (N == 1024) dft16<DIR>(x);
    else dft8<DIR>(x);
}

template <int N, int DIR>
__device__ __forceinline__ void fft_big(v2f (&v)[1][geo<N>::BPL][4], v2f *fb, const v2f *tw, int lane)
{
    static_assert(N == 512 || N == 1024, "fft_big is the 8.8.8 / 16.4.16 scheme");
    constexpr int BPL = geo<N>::BPL, R = 4 * BPL;             // 2, 8  or  4, 16
    constexpr int T2 = N == 1024 ? 48 : 56;                    // start of the stage-3 twiddles
    // ---- stage 1: radix R, Ns = 1, from registers; out[R lane + u]
    dft_lane<N, DIR>(v[0]);
#pragma unroll
    for (int q = 0; q < BPL; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) fb[swz<R>(R * lane + r + 4 * q)] = v[0][q][r];
    wave_sync();
    if constexpr (N == 1024) {
        // ---- stage 2: radix 4, Ns = 16: butterflies j = lane + 64 q
        v2f u4[4][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = lane + 64 * q, k = j & 15;
#pragma unroll
            for (int r = 0; r < 4; ++r) u4[q][r] = fb[swz<16>(j + 256 * r)];
#pragma unroll
            for (int r = 1; r < 4; ++r) u4[q][r] = twid<DIR>(u4[q][r], tw[3 * k + r - 1]);
            radix4<DIR>(u4[q]);
        }
        wave_sync();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = lane + 64 * q, k = j & 15;
#pragma unroll
            for (int r = 0; r < 4; ++r) fb[((j - k) << 2) + k + 16 * r] = u4[q][r];
        }
    } else {
        // ---- stage 2: radix 8, Ns = 8: butterfly j = lane
        v2f u8[2][4];
        const int k = lane & 7;
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int t = q + 2 * r;
                u8[q][r] = fb[swz<8>(lane + 64 * t)];
                if (t > 0) u8[q][r] = twid<DIR>(u8[q][r], tw[7 * k + t - 1]);
            }
        dft8<DIR>(u8);
        wave_sync();
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) fb[((lane - k) << 3) + k + 8 * (r + 4 * q)] = u8[q][r];
    }
    wave_sync();
    // ---- stage 3: radix R, Ns = 64, to registers: in[lane + 64 t], twiddle^(t lane), out lane + 64 u
    v2f x[BPL][4];
#pragma unroll
    for (int q = 0; q < BPL; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int t = q + BPL * r;
            x[q][r] = fb[lane + 64 * t];
            if (t > 0) x[q][r] = twid<DIR>(x[q][r], tw[T2 + (R - 1) * lane + t - 1]);
        }
    dft_lane<N, DIR>(x);
    // x[q'][r'] = X_u with u = r' + 4 q';  the lane owns u = q + BPL r
#pragma unroll
    for (int q = 0; q < BPL; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int u = q + BPL * r;
            v[0][q][r] = x[u >> 2][u & 3];
        }
    wave_sync();
}

// registers -> (LDS stages) -> registers, natural order in and out, SPW symbols at once
template <int N, int DIR, int SPW>
__device__ __forceinline__ void fft_wave(v2f (&v)[SPW][geo<N>::BPL][4], v2f *fb, int sb, const v2f *tw,
                                         int lane)
{
    // N = 512 / 1024: 8.8.8 / 16.4.16 with the outer stages in registers (fft_big); the smaller sizes: the radix-4/2 ladder
    // through LDS
    if constexpr (N == 512 || N == 1024) {
        static_assert(SPW == 1, "one symbol per wave at N >= 512");
        fft_big<N, DIR>(v, fb, tw, lane);
    } else {
        fft_first<N, DIR, SPW>(v, fb, sb, lane);
        if constexpr (N == 64) {
            fft_mid4<N, 4, DIR, SPW>(fb, sb, tw, lane);
        } else if constexpr (N == 128) {
            fft_mid2<N, 4, DIR, SPW>(fb, sb, tw, lane);
            fft_mid4<N, 8, DIR, SPW>(fb, sb, tw, lane);
        } else {
            static_assert(N == 256, "unsupported DFT length");
            fft_mid4<N, 4, DIR, SPW>(fb, sb, tw, lane);
            fft_mid4<N, 16, DIR, SPW>(fb, sb, tw, lane);
        }
        fft_last<N, DIR, SPW>(v, fb, sb, tw, lane);
    }
}

// Fill the per-stage twiddle tables (once per workgroup).
template <int N> __device__ __forceinline__ void fill_twiddles(v2f *tw, int tid, int nthreads)
{
    if constexpr (N == 512 || N == 1024) {
        // tables of fft_big
        constexpr int R = N / 64, T2 = N == 1024 ? 48 : 56;
        for (int i = tid; i < T2 + (R - 1) * 64; i += nthreads) {
            float num, den;
            if (i < T2) {
                const int per = N == 1024 ? 3 : 7;
                num = (float)((i / per) * (1 + i % per)); den = 64.0f;                   // r k / 64
            } else {
                const int e = i - T2;
                num = (float)((e / (R - 1)) * (1 + e % (R - 1))); den = (float)N;        // t j / N
            }
            float sv, cv;
            sincospif(-2.0f * num / den, &sv, &cv);
            tw[i] = mk(cv, sv);
        }
        return;
    }
    int off = 0, ns = 4;
    while (ns <= N / 4) {
        const bool r2 = (N == 128 && ns == 4) || (N == 512 && ns == 16);
        const int cnt = r2 ? ns : 3 * ns;
        for (int i = tid; i < cnt; i += nthreads) {
            const int k = r2 ? i : i / 3, r = r2 ? 1 : 1 + i % 3;
            float sv, cv;
            sincospif(-2.0f * (float)(r * k) / (float)((r2 ? 2 : 4) * ns), &sv, &cv);
            tw[off + i] = mk(cv, sv);
        }
        off += cnt;
        ns *= r2 ? 2 : 4;
    }
}

// CNT consecutive FIR outputs starting at window base w (w[i] = tx[j0 - (LT-1) + i]).
// The taps are wave-uniform and read through a noalias kernel argument, so they arrive by
// scalar loads as SGPR pairs and feed v_pk_fma_f32 directly: 2 instructions per complex MAC.
template <int CNT>
__device__ __forceinline__ void fir_chunk(const v2f *w, const v2f *__restrict__ taps, v2f *acc)
{
    constexpr int LT = WOFDM_LT;
    v2f win[CNT + LT - 1];
#pragma unroll
    for (int i = 0; i < CNT + LT - 1; ++i) win[i] = w[i];
#pragma unroll
    for (int r = 0; r < CNT; ++r) acc[r] = mk(0.f, 0.f);
#pragma unroll
    for (int l = 0; l < LT; ++l) {
        const v2f t = taps[l];
        const v2f tn = mk(-t.y, t.y);
#pragma unroll
        for (int r = 0; r < CNT; ++r) {
            const v2f x = win[r + LT - 1 - l];
            acc[r] = __builtin_elementwise_fma(t.xx, x, acc[r]);
            acc[r] = __builtin_elementwise_fma(tn, x.yx, acc[r]);
        }
    }
}

template <int RB, int CH>
__device__ __forceinline__ void fir_lane(const v2f *w, const v2f *__restrict__ taps, v2f (&acc)[RB])
{
    constexpr int FULL = RB / CH, REM = RB % CH;
#pragma unroll
    for (int c = 0; c < FULL; ++c) fir_chunk<CH>(w + c * CH, taps, &acc[c * CH]);
    if constexpr (REM != 0) fir_chunk<REM>(w + FULL * CH, taps, &acc[FULL * CH]);
}

}  // namespace
