// Developer microbenchmark: what the vector instruction kinds of the frame loop cost BESIDE a busy matrix pipe -- the instruction the
// frame kernels use (v_mfma_f32_16x16x32_f16) at their occupancy (three waves per SIMD: one workgroup of 12 waves per CU).
// tools/ubench/valu_dep.hip priced the same kinds with no MFMA running; the kernels never run that way.  Per kind, five arrangements:
//   alone       every wave runs the vector stream (13 instructions x 6 per iteration, four independent chains)
//   same wave   every wave runs chains of six MFMAs (two accumulators in turn, as mma33) with 13 vector instructions behind each MFMA:
//               the kernel's ratio (148 MFMAs among 1 970 vector instructions per wave and frame).  Beside it: the MFMAs alone.
//   other wave  one wave of each SIMD runs MFMA chains, the other two the vector stream:
//                 idle   the MFMA wave does nothing (the two-wave baseline),
//                 kernel a chain of six MFMAs, then s_sleep: about a third of the SIMD's time, the kernel's density,
//                 full   MFMAs back to back.
// A wave's role comes from the SIMD it really runs on (HW_ID) and its arrival rank there, not from its index in the workgroup; time
// is the wave's own s_memtime, so no clock rate is assumed.  Vector instructions are inline asm: nothing is packed, split or removed.
// hipcc --offload-arch=gfx950 -O3 -fno-slp-vectorize valu_beside_mfma.hip -o valu_beside_mfma
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <vector>

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));

enum { K_PKFMA, K_PKMUL, K_PKADD, K_FMA, K_MUL, K_FMAC, K_MIXF32, K_CVTPK, K_MADU64, K_BITOP3, K_SIN, K_LOG, K_COUNT };
enum { M_VALU, M_MFMA, M_BOTH, M_SPLIT };
enum { S_IDLE, S_KERNEL, S_FULL };

#define NV 13          // vector instructions behind each MFMA (the groups below are written out for 13)
#define NM 6           // MFMAs of a chain
#define WAVES 12       // per workgroup = per CU: three per SIMD

struct vstate { uint32_t a[4], b[1]; uint64_t q[4]; f2 p[4]; };

// The 13 vector instructions behind one MFMA are ONE asm statement (the compiler pads every statement that touches a register the one
// before wrote with an s_nop; one per group instead of one per four instructions), the four chains in turn, the first chain of group g
// being g % 4, so that no chain's instructions ever follow each other directly.
#define G4(I, a, b, c, d) I(a) I(b) I(c) I(d)
#define GRP0(I) G4(I, 0, 1, 2, 3) G4(I, 0, 1, 2, 3) G4(I, 0, 1, 2, 3) I(0)
#define GRP1(I) G4(I, 1, 2, 3, 0) G4(I, 1, 2, 3, 0) G4(I, 1, 2, 3, 0) I(1)
#define GRP2(I) G4(I, 2, 3, 0, 1) G4(I, 2, 3, 0, 1) G4(I, 2, 3, 0, 1) I(2)
#define GRP3(I) G4(I, 3, 0, 1, 2) G4(I, 3, 0, 1, 2) G4(I, 3, 0, 1, 2) I(3)
#define EMIT(I, A, C)                                                                                                               \
    do {                                                                                                                            \
        if ((g & 3) == 0) asm volatile(GRP0(I) : "+v"(A[0]), "+v"(A[1]), "+v"(A[2]), "+v"(A[3]) : "v"(C), "s"(m0) : "vcc");          \
        if ((g & 3) == 1) asm volatile(GRP1(I) : "+v"(A[0]), "+v"(A[1]), "+v"(A[2]), "+v"(A[3]) : "v"(C), "s"(m0) : "vcc");          \
        if ((g & 3) == 2) asm volatile(GRP2(I) : "+v"(A[0]), "+v"(A[1]), "+v"(A[2]), "+v"(A[3]) : "v"(C), "s"(m0) : "vcc");          \
        if ((g & 3) == 3) asm volatile(GRP3(I) : "+v"(A[0]), "+v"(A[1]), "+v"(A[2]), "+v"(A[3]) : "v"(C), "s"(m0) : "vcc");          \
    } while (0)
#define I_PKFMA(c) "v_pk_fma_f32 %" #c ", %" #c ", %4, %4\n\t"
#define I_PKMUL(c) "v_pk_mul_f32 %" #c ", %" #c ", %4\n\t"
#define I_PKADD(c) "v_pk_add_f32 %" #c ", %" #c ", %4\n\t"
#define I_FMA(c) "v_fma_f32 %" #c ", %" #c ", %4, %4\n\t"
#define I_MUL(c) "v_mul_f32_e32 %" #c ", %" #c ", %4\n\t"
#define I_FMAC(c) "v_fmac_f32_e32 %" #c ", %4, %4\n\t"
#define I_MIXF32(c) "v_fma_mix_f32 %" #c ", %" #c ", -1.0, %4 op_sel_hi:[1,0,0]\n\t"
#define I_CVTPK(c) "v_cvt_pk_f16_f32 %" #c ", %" #c ", %4\n\t"
#define I_MADU64(c) "v_mad_u64_u32 %" #c ", vcc, %4, %5, %" #c "\n\t"
#define I_BITOP3(c) "v_bitop3_b32 %" #c ", %" #c ", %4, %5 bitop3:0x96\n\t"
#define I_SIN(c) "v_sin_f32_e32 %" #c ", %" #c "\n\t"
#define I_LOG(c) "v_log_f32_e32 %" #c ", %" #c "\n\t"
template <int KIND> __device__ __forceinline__ void vgroup(vstate &s, int g)
{
    const uint32_t m0 = 0xD2511F53u;
    const f2 pc = {1.0001f, 0.5f};
    const uint32_t y = s.b[0];
    if (KIND == K_PKFMA) EMIT(I_PKFMA, s.p, pc);
    if (KIND == K_PKMUL) EMIT(I_PKMUL, s.p, pc);
    if (KIND == K_PKADD) EMIT(I_PKADD, s.p, pc);
    if (KIND == K_FMA) EMIT(I_FMA, s.a, y);
    if (KIND == K_MUL) EMIT(I_MUL, s.a, y);
    if (KIND == K_FMAC) EMIT(I_FMAC, s.a, y);
    if (KIND == K_MIXF32) EMIT(I_MIXF32, s.a, y);
    if (KIND == K_CVTPK) EMIT(I_CVTPK, s.a, y);
    if (KIND == K_MADU64) EMIT(I_MADU64, s.q, y);
    if (KIND == K_BITOP3) EMIT(I_BITOP3, s.a, y);
    if (KIND == K_SIN) EMIT(I_SIN, s.a, y);
    if (KIND == K_LOG) EMIT(I_LOG, s.a, y);
}
// everything an MFMA and the vector stream around it touch passes through one empty statement: the compiler keeps their order
#define TIE(s, d0, d1)                                                                                                              \
    asm volatile("" : "+v"(d0), "+v"(d1), "+v"(s.a[0]), "+v"(s.a[1]), "+v"(s.a[2]), "+v"(s.a[3]), "+v"(s.q[0]), "+v"(s.q[1]),       \
                 "+v"(s.q[2]), "+v"(s.q[3]), "+v"(s.p[0]), "+v"(s.p[1]), "+v"(s.p[2]), "+v"(s.p[3]))

// out: per wave {cycles, role (0 vector, 1 MFMA), SIMD, MFMAs issued}
template <int KIND, int MODE>
__global__ void __launch_bounds__(64 * WAVES) k(uint64_t *out, int iters, int split_mfma, float fa)
{
    __shared__ uint32_t arrived[4], done[4];
    __shared__ uint32_t alone_on_cu[24 * 1024];                     // 96 KB of the CU's 160: no second workgroup beside this one
    if (threadIdx.x < 4) { arrived[threadIdx.x] = 0; done[threadIdx.x] = 0; alone_on_cu[(iters + threadIdx.x) & 1023] = 0; }
    __syncthreads();
    const uint32_t simd = (__builtin_amdgcn_s_getreg(4 | (4 << 6) | (1 << 11))) & 3u;          // HW_ID[5:4]
    uint32_t rank = 0;
    if ((threadIdx.x & 63) == 0) rank = atomicAdd(&arrived[simd], 1u);
    rank = __builtin_amdgcn_readfirstlane(rank);
    __syncthreads();
    const uint32_t here = arrived[simd];

    vstate s;
    for (int j = 0; j < 4; ++j) {
        s.a[j] = __builtin_bit_cast(uint32_t, 1.0f + 0.001f * (float)(threadIdx.x + j));
        s.q[j] = threadIdx.x + j;
        s.p[j] = (f2){1.f + j, 2.f};
    }
    s.b[0] = __builtin_bit_cast(uint32_t, fa);
    h8 av, bv;
    for (int i = 0; i < 8; ++i) { av[i] = (_Float16)(fa + (float)(threadIdx.x & 7)); bv[i] = (_Float16)(fa * (float)i); }
    f4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = {1.f, 1.f, 1.f, 1.f};
    const bool mfma_wave = MODE == M_SPLIT && rank == 0;
    uint64_t nm = 0;

    __syncthreads();
    const uint64_t t0 = __builtin_readcyclecounter();
    if (MODE != M_SPLIT || !mfma_wave) {
        for (int it = 0; it < iters; ++it) {
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                if (MODE == M_MFMA || MODE == M_BOTH) {
                    TIE(s, d0, d1);
                    if (m & 1) d1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, bv, d1, 0, 0, 0);
                    else d0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, bv, d0, 0, 0, 0);
                    TIE(s, d0, d1);
                }
                if (MODE != M_MFMA) {
                    vgroup<KIND>(s, m);
                }
            }
        }
        if (MODE == M_MFMA || MODE == M_BOTH) nm = (uint64_t)iters * NM;
        if (MODE == M_SPLIT && (threadIdx.x & 63) == 0) atomicAdd(&done[simd], 1u);
    } else if (split_mfma != S_IDLE) {
        // until the vector waves of this SIMD are through (looked at every 8 chains; bounded, so it ends whatever happens)
        for (int it = 0; it < 64 * iters; ++it) {
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                if (m & 1) d1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, bv, d1, 0, 0, 0);
                else d0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, bv, d0, 0, 0, 0);
                asm volatile("" : "+v"(d0), "+v"(d1));
            }
            nm += NM;
            if (split_mfma == S_KERNEL) __builtin_amdgcn_s_sleep(3);
            if ((it & 7) == 7 && *(volatile uint32_t *)&done[simd] >= here - 1) break;
        }
    }
    const uint64_t t1 = __builtin_readcyclecounter();

    float r = d0[0] + d0[1] + d0[2] + d0[3] + d1[0] + d1[1] + d1[2] + d1[3];
    for (int j = 0; j < 4; ++j) r += __builtin_bit_cast(float, s.a[j]) + (float)(uint32_t)s.q[j] + s.p[j].x + s.p[j].y;
    if ((threadIdx.x & 63) == 0) {
        uint64_t *o = out + 4 * ((size_t)blockIdx.x * WAVES + (threadIdx.x >> 6));
        o[0] = t1 - t0; o[1] = mfma_wave; o[2] = simd | ((uint64_t)here << 8) | (r == 12345.678f ? 1ull << 63 : 0); o[3] = nm;
    }
}

struct result { double cyc_vec, cyc_mfma, density; bool three; };

template <int KIND, int MODE> result run(int split_mfma)
{
    const int grid = 256, iters = 1500;
    uint64_t *d;
    hipMalloc(&d, (size_t)grid * WAVES * 4 * sizeof(uint64_t));
    k<KIND, MODE><<<grid, 64 * WAVES>>>(d, 4, split_mfma, 1.0f);
    hipDeviceSynchronize();
    k<KIND, MODE><<<grid, 64 * WAVES>>>(d, iters, split_mfma, 1.0f);
    if (hipDeviceSynchronize() != hipSuccess) { fprintf(stderr, "launch failed\n"); exit(1); }
    std::vector<uint64_t> h((size_t)grid * WAVES * 4);
    hipMemcpy(h.data(), d, h.size() * sizeof(uint64_t), hipMemcpyDeviceToHost);
    hipFree(d);
    result r = {0, 0, 0, true};
    double nv = 0, nmw = 0, mf = 0;
    for (size_t w = 0; w < (size_t)grid * WAVES; ++w) {
        const uint64_t *o = &h[4 * w];
        if (((o[2] >> 8) & 0xFF) != 3) r.three = false;
        if (o[1]) { r.cyc_mfma += (double)o[0]; mf += (double)o[3]; nmw += 1; }
        else { r.cyc_vec += (double)o[0]; nv += 1; if (MODE != M_SPLIT) mf += (double)o[3]; }
    }
    if (MODE == M_SPLIT) r.density = r.cyc_mfma > 0 ? 16.0 * mf / r.cyc_mfma : 0;
    r.cyc_vec /= nv > 0 ? nv : 1;
    r.cyc_mfma /= nmw > 0 ? nmw : 1;
    // per iteration of a wave
    r.cyc_vec /= iters;
    return r;
}

template <int KIND> void kind(const char *name, double mfma_alone)
{
    const int per_it = NV * NM;
    const result a = run<KIND, M_VALU>(0), b = run<KIND, M_BOTH>(0);
    const result c0 = run<KIND, M_SPLIT>(S_IDLE), c1 = run<KIND, M_SPLIT>(S_KERNEL), c2 = run<KIND, M_SPLIT>(S_FULL);
    // SIMD cycles per wave-instruction: a wave's time over the instructions the SIMD's vector waves issued meanwhile
    const double ca = a.cyc_vec / (3 * per_it), cc0 = c0.cyc_vec / (2 * per_it), cc1 = c1.cyc_vec / (2 * per_it),
                 cc2 = c2.cyc_vec / (2 * per_it);
    // same wave: how much of the MFMAs' time disappears under the vector stream (1 = all of it, 0 = the two add up)
    const double hidden = (a.cyc_vec + mfma_alone - b.cyc_vec) / mfma_alone;
    printf("%-18s %6.2f | %8.0f %8.0f %8.0f  %5.2f | %6.2f  %6.2f (d %.2f) x%.3f  %6.2f (d %.2f) x%.3f %s\n", name, ca, a.cyc_vec,
           mfma_alone, b.cyc_vec, hidden, cc0, cc1, c1.density, cc1 / cc0, cc2, c2.density, cc2 / cc0,
           a.three && b.three && c0.three && c1.three && c2.three ? "" : " (!) not three waves on every SIMD");
}

int main()
{
    const result m = run<K_FMA, M_MFMA>(0);
    printf("v_mfma_f32_16x16x32_f16, 3 waves per SIMD, chains of %d, alone: %.0f cycles per iteration of a wave = %.2f SIMD cycles per MFMA\n",
           NM, m.cyc_vec, m.cyc_vec / (3 * NM));
    printf("per iteration of a wave: %d MFMAs, %d vector instructions (%d behind each MFMA), four independent chains\n", NM, NV * NM, NV);
    printf("columns: alone = SIMD cycles per wave-instruction, 3 waves | same wave: vector alone, MFMAs alone, both (cycles per\n"
           "iteration of a wave), share of the MFMAs' time hidden | other wave: SIMD cycles per wave-instruction of two vector waves with\n"
           "the third idle, with it running MFMA chains at the kernel's density, and back to back (d = share of the SIMD's time an MFMA\n"
           "executes; x = against idle)\n");
    printf("%-18s %6s | %8s %8s %8s  %5s | %6s  %s\n", "kind", "alone", "vector", "mfma", "both", "hid", "idle", "kernel density / full");
    kind<K_PKFMA>("v_pk_fma_f32", m.cyc_vec);
    kind<K_PKMUL>("v_pk_mul_f32", m.cyc_vec);
    kind<K_PKADD>("v_pk_add_f32", m.cyc_vec);
    kind<K_FMA>("v_fma_f32", m.cyc_vec);
    kind<K_MUL>("v_mul_f32", m.cyc_vec);
    kind<K_FMAC>("v_fmac_f32", m.cyc_vec);
    kind<K_MIXF32>("v_fma_mix_f32", m.cyc_vec);
    kind<K_CVTPK>("v_cvt_pk_f16_f32", m.cyc_vec);
    kind<K_MADU64>("v_mad_u64_u32", m.cyc_vec);
    kind<K_BITOP3>("v_bitop3_b32", m.cyc_vec);
    kind<K_SIN>("v_sin_f32", m.cyc_vec);
    kind<K_LOG>("v_log_f32", m.cyc_vec);
    return 0;
}
