// wofdm_code.hip -- the coded link: the decoders behind the receive profile's soft bits (wofdm_rx_profile_coded, _coded_frame,
// _ldpc, _coset, _harq) and on soft bits of the caller's (wofdm_viterbi_decode, wofdm_viterbi_decode_long, wofdm_ldpc_decode,
// wofdm_ldpc_harq_decode), and the encoders (wofdm_conv_encode, wofdm_ldpc_encode).  None of these kernels knows the DFT length,
// so the unit is compiled once; the per-N units (wofdm_aux.hip), whose receive kernels write the soft bits, and the C ABI reach it
// through the functions wofdm_link.h declares, and every kernel is launched from here.
#include "wofdm_link.h"

namespace {

// The K = 7 decoder of include/wofdm.h, generators 133 / 171 octal: one wave per (codeword, code), lane = state s.  The wave
// first gathers its codeword through cd.gather and depunctures it into LDS -- step t's pair (dA, dB) as two int8, 0 where the
// pattern keeps nothing: a lane takes the steps t = lane, lane + 64, ... --, then walks the trellis: the metrics of the
// predecessors p0 = (s << 1) & 63 and p1 = p0 | 1 come by two cross-lane reads, the branch into s with input bit u = s >> 5 has
// the coded bits A = parity(r & 0133), B = parity(r & 0171) of r = (u << 6) | p -- bit 0 of r is in both generators, so p1's pair
// is the complement of p0's --, the metric is the sum of d over the hypothesised ones, int32, and the survivor is p0 unless p1's
// metric is strictly smaller.  The 64 decisions of a step are one __ballot word, which lane 0 leaves in LDS; the traceback from
// state 0 at step T reads them back (wave-uniform) and leaves u_t as bytes, which the lanes then count (the profile: integer
// atomics on errs) or copy out (wofdm_viterbi_decode).  LDS: 11 bytes per step (8 decisions, 2 branch metrics, 1 decoded bit),
// at most 50 688 B at T = 4608; every loop has a wave-uniform trip count.
__global__ void __launch_bounds__(64) wofdm_viterbi_kernel(const wofdm_codeparams cd)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char vsm[];
    const int lane = threadIdx.x;
    const int code = blockIdx.y, rate = cd.rate[code], T = cd.steps[code], n_c = cd.n_c;
    const uint64_t w = blockIdx.x;
    // the profile: codeword w = (job, point, data symbol); the postamble of a point with post holds no codeword, and its wave
    // leaves before it does anything (wave-uniform; the workgroup is this one wave)
    int sym = 0, pt = 0;
    if (cd.errs != nullptr) {
        sym = (int)(w % (uint64_t)cd.S1);
        pt = (int)((w / (uint64_t)cd.S1) % (uint64_t)cd.n_points);
        if (cd.pts[pt].post != 0 && sym == cd.S1 - 1) return;
    }
    unsigned long long *hist = reinterpret_cast<unsigned long long *>(vsm);        // [T]
    uint16_t *bm = reinterpret_cast<uint16_t *>(hist + T);                          // [T] dA | dB << 8
    uint8_t *ub = reinterpret_cast<uint8_t *>(bm + T);                              // [T]
    const int8_t *__restrict__ soft = cd.soft + (int64_t)w * cd.cw_stride;
    // the coded-stream indices of step t's kept outputs, A before B: rate 1/2 (2 t, 2 t + 1); rate 2/3, period 2, A 1 1, B 1 0;
    // rate 3/4, period 3, A 1 1 0, B 1 0 1
    for (int t = lane; t < T; t += 64) {
        int ca, cb;
        if (rate == 0) {
            ca = 2 * t;
            cb = 2 * t + 1;
        } else if (rate == 1) {
            const int q = t >> 1, ph = t & 1;
            ca = 3 * q + 2 * ph;
            cb = ph == 0 ? 3 * q + 1 : -1;
        } else {
            const int q = t / 3, ph = t - 3 * q;
            ca = ph == 2 ? -1 : 4 * q + 2 * ph;
            cb = ph == 1 ? -1 : 4 * q + (ph == 0 ? 1 : 3);
        }
        const int da = ca >= 0 && ca < n_c ? soft[cd.gather[ca]] : 0;
        const int db = cb >= 0 && cb < n_c ? soft[cd.gather[cb]] : 0;
        bm[t] = (uint16_t)(((uint32_t)da & 0xFFu) | (((uint32_t)db & 0xFFu) << 8));
    }
    __syncthreads();
    const int p0 = (lane << 1) & 63, u = lane >> 5, r0 = (u << 6) | p0;
    const bool a0 = (__popc(r0 & 0133) & 1) != 0, b0 = (__popc(r0 & 0171) & 1) != 0;
    int m = lane == 0 ? 0 : (1 << 30);
    for (int t = 0; t < T; ++t) {
        const uint32_t pr = bm[t];
        const int da = (int)(int8_t)(pr & 0xFFu), db = (int)(int8_t)(pr >> 8);
        const int c0 = __shfl(m, p0, 64) + (a0 ? da : 0) + (b0 ? db : 0);
        const int c1 = __shfl(m, p0 | 1, 64) + (a0 ? 0 : da) + (b0 ? 0 : db);
        const bool dec = c1 < c0;
        m = dec ? c1 : c0;
        const unsigned long long word = __ballot(dec);
        if (lane == 0) hist[t] = word;
    }
    __syncthreads();
    // traceback from state 0 at step T (every lane walks the same path: the reads are broadcasts)
    int st = 0;
    for (int t = T - 1; t >= 0; --t) {
        const unsigned long long word = hist[t];
        if (lane == 0) ub[t] = (uint8_t)(st >> 5);
        st = ((st << 1) & 63) | (int)((word >> st) & 1ull);
    }
    __syncthreads();
    if (cd.errs != nullptr) {
        // info-bit errors over t < T - 6, a codeword error for any u_t != 0
        const uint64_t job = w / ((uint64_t)cd.S1 * (uint64_t)cd.n_points), cell = (cd.item0 + job) / cd.frames;
        int info = 0, any = 0;
        for (int t = lane; t < T; t += 64) {
            const int b = ub[t];
            info += t < T - 6 ? b : 0;
            any |= b;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            info += __shfl_xor(info, o, 64);
            any |= __shfl_xor(any, o, 64);
        }
        if (lane == 0 && any != 0) {
            unsigned long long *e = cd.errs + ((((uint64_t)pt * cd.cells + cell) * (uint64_t)cd.n_codes + (uint64_t)code) * (uint64_t)cd.S1 + (uint64_t)sym) * 2;
            if (info != 0) atomicAdd(e, (unsigned long long)info);
            atomicAdd(e + 1, 1ull);
        }
    } else {
        uint8_t *__restrict__ out = cd.bits + w * (uint64_t)T;
        for (int t = lane; t < T; t += 64) out[t] = ub[t];
        if (lane == 0 && cd.metric != nullptr) cd.metric[w] = m;
    }
}

// The coded-stream indices of step t's kept outputs, A before B, -1 where the pattern keeps nothing (wofdm_viterbi_kernel's
// closed form, for the streaming decoders and the encoder)
__device__ __forceinline__ void conv_kept(int rate, int t, int &ca, int &cb)
{
    if (rate == 0) {
        ca = 2 * t;
        cb = 2 * t + 1;
    } else if (rate == 1) {
        const int q = t >> 1, ph = t & 1;
        ca = 3 * q + 2 * ph;
        cb = ph == 0 ? 3 * q + 1 : -1;
    } else {
        const int q = t / 3, ph = t - 3 * q;
        ca = ph == 2 ? -1 : 4 * q + 2 * ph;
        cb = ph == 1 ? -1 : 4 * q + (ph == 0 ? 1 : 3);
    }
}

// The pair (dA, dB) of step t as wofdm_viterbi_kernel forms it, in two stages so that both loads of a block can be in flight
// while an earlier block is walked: the byte offsets of the two kept outputs through the gather table (-1: the pattern keeps
// nothing, c >= n_c, or t >= T), then the soft bits behind them.
__device__ __forceinline__ void vlong_offsets(const int32_t *__restrict__ gather, int rate, int n_c, int T, int t, int &oa, int &ob)
{
    int ca, cb;
    conv_kept(rate, t, ca, cb);
    // (the loads themselves are unconditional, on an index clamped into the table, so that nothing waits for them here)
    const int ga = gather[min(max(ca, 0), n_c - 1)], gb = gather[min(max(cb, 0), n_c - 1)];
    oa = t < T && ca >= 0 && ca < n_c ? ga : -1;
    ob = t < T && cb >= 0 && cb < n_c ? gb : -1;
}
typedef short vlong_i16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int vlong_pair(const int8_t *__restrict__ soft, int oa, int ob)
{
    const int sa = soft[max(oa, 0)], sb = soft[max(ob, 0)];             // (unconditional as well: byte 0 is the block's)
    const int da = oa >= 0 ? sa : 0, db = ob >= 0 ? sb : 0;
    return (int)(((uint32_t)da & 0xFFFFu) | ((uint32_t)db << 16));       // two int16
}

// The decoder of wofdm_viterbi_kernel for codewords of any length up to WOFDM_CODE_LONG_STEPS (wofdm_longparams): the same code,
// metric, start and tie rules -- the decoded bits and the metric are that kernel's wherever it takes the word --, one wave per
// codeword, lane = state, and no LDS: the survivor history goes to device memory in blocks of 64 steps.
//   Forward.  Lane l holds the pair of step 64 b + l of the current block; the pairs of block b + 1 and the gather offsets of
// block b + 2 are loaded before block b is walked.  Step i of a block reads its pair from lane i (v_readlane: a constant lane in
// the unrolled full block, a wave-uniform one in the last, partial block), and every lane keeps its own decision as bit i of a
// 64-bit word: the block's history is the 64 x 64 bit matrix [state][step], one word per lane, and leaves as one 512-byte
// store.  (The transpose of wofdm_viterbi_kernel's ballot words: a lane ORs a bit into its own register, so the step needs
// neither a ballot nor a write into another lane.)
//   Traceback.  Blocks descending: one 512-byte load, one word per lane, then the steps descending -- the decision of the path's
// state st at step i is bit i of lane st's word, a lane read with a wave-uniform index; the state and the block's 64 decoded
// bits are wave-uniform.  The profile counts the masks' bits -- t < T - 6: info bits -- and ends with integer atomics where the
// codeword has an error; the decoder alone stores bit l of a block's mask from lane l, one byte each.
//   Every trip count is wave-uniform; the workgroup is the one wave, and no wave waits for another.  int32 suffices: |d| <= 128,
// two outputs per step, so |metric| <= 2^28 at T = 2^20 beside the 2^30 of the start.
__global__ void __launch_bounds__(64) wofdm_viterbi_long_kernel(const wofdm_longparams lp)
{
    const int lane = threadIdx.x;
    const uint64_t w = blockIdx.x;
    int v = 0, pt = 0;
    if (lp.errs != nullptr) {
        pt = (int)(w % (uint64_t)lp.n_points);
        v = lp.pts[pt].post != 0 ? 1 : 0;
    }
    const int rate = lp.rate, T = lp.steps[v], n_c = lp.n_c[v];
    if (T < 7) return;                                                  // (a point without a data symbol: wave-uniform)
    const int n_blocks = (T + 63) >> 6;
    const int32_t *__restrict__ gather = lp.gather[v];
    const int8_t *__restrict__ soft = lp.soft + (int64_t)w * lp.cw_stride;
    unsigned long long *__restrict__ hist = lp.hist + (size_t)w * (size_t)lp.hist_blocks * 64;

    const int p0 = (lane << 1) & 63, u = lane >> 5, r0 = (u << 6) | p0;
    const bool a0 = (__popc(r0 & 0133) & 1) != 0, b0 = (__popc(r0 & 0171) & 1) != 0;
    int m = lane == 0 ? 0 : (1 << 30);
    // one step: the survivor into this lane's state; its decision is bit i of the lane's history word of the block
    uint32_t hlo, hhi;
    // (the branch metric is a dot product of the step's pair, two int16, with the lane's 0 / 1 pair: v_dot2c_i32_i16, exact)
    const vlong_i16x2 sel0 = {(short)(a0 ? 1 : 0), (short)(b0 ? 1 : 0)}, sel1 = {(short)(a0 ? 0 : 1), (short)(b0 ? 0 : 1)};
    const auto step = [&](int i, int pair) {
        const vlong_i16x2 d = __builtin_bit_cast(vlong_i16x2, pair);
        const int c0 = __builtin_amdgcn_sdot2(sel0, d, __shfl(m, p0, 64), false);
        const int c1 = __builtin_amdgcn_sdot2(sel1, d, __shfl(m, p0 | 1, 64), false);
        const bool dec = c1 < c0;
        m = dec ? c1 : c0;
        if (i < 32)
            hlo |= dec ? 1u << i : 0u;
        else
            hhi |= dec ? 1u << (i - 32) : 0u;
    };
    int dp, oa, ob;
    vlong_offsets(gather, rate, n_c, T, lane, oa, ob);
    dp = vlong_pair(soft, oa, ob);
    vlong_offsets(gather, rate, n_c, T, 64 + lane, oa, ob);
    for (int b = 0; b < n_blocks; ++b) {
        int noa, nob;
        const int ndp = vlong_pair(soft, oa, ob);                        // block b + 1 (zeros behind the codeword's end)
        vlong_offsets(gather, rate, n_c, T, 64 * (b + 2) + lane, noa, nob);
        hlo = hhi = 0u;
        const int n = T - 64 * b;
        if (n >= 64) {
#pragma unroll
            for (int i = 0; i < 64; ++i) step(i, __builtin_amdgcn_readlane(dp, i));
        } else {
            for (int i = 0; i < n; ++i) step(i, __builtin_amdgcn_readlane(dp, i));
        }
        hist[(size_t)b * 64 + (size_t)lane] = ((unsigned long long)hhi << 32) | (unsigned long long)hlo;
        dp = ndp; oa = noa; ob = nob;
    }
    // (a lane reads back what it stored itself: program order, no fence is needed)
    int st = 0, info = 0;
    bool any = false;
    uint8_t *__restrict__ out = lp.errs == nullptr ? lp.bits + w * (uint64_t)T : nullptr;
    for (int b = n_blocks - 1; b >= 0; --b) {
        const unsigned long long hw = hist[(size_t)b * 64 + (size_t)lane];
        const int wlo = (int)(uint32_t)hw, whi = (int)(uint32_t)(hw >> 32);
        const int n = T - 64 * b;
        unsigned long long mask = 0ull;
        // step i of the block: the decision of the path's state st is bit i of lane st's word
        const auto back = [&](int i) {
            const uint32_t word = (uint32_t)__builtin_amdgcn_readlane(i < 32 ? wlo : whi, st);
            mask |= (unsigned long long)(st >> 5) << i;
            st = ((st << 1) & 63) | (int)((word >> (i & 31)) & 1u);
        };
        if (n >= 64) {
#pragma unroll
            for (int i = 63; i >= 0; --i) back(i);
        } else {
            for (int i = n - 1; i >= 0; --i) back(i);
        }
        if (out != nullptr) {
            if (lane < n) out[(size_t)b * 64 + (size_t)lane] = (uint8_t)((mask >> lane) & 1ull);
        } else {
            // info bits: t < T - 6, the first lim = T - 6 - 64 b of the block
            const int lim = T - 6 - 64 * b;
            const unsigned long long im = lim >= 64 ? ~0ull : (lim <= 0 ? 0ull : (1ull << lim) - 1ull);
            info += __popcll(mask & im);
            any = any || mask != 0ull;
        }
    }
    if (lp.errs != nullptr) {
        if (lane == 0 && any) {
            const uint64_t job = w / (uint64_t)lp.n_points, cell = (lp.item0 + job) / lp.frames;
            unsigned long long *e = lp.errs + (((uint64_t)pt * lp.cells + cell) * (uint64_t)lp.n_codes + (uint64_t)lp.code) * 2;
            if (info != 0) atomicAdd(e, (unsigned long long)info);
            atomicAdd(e + 1, 1ull);
        }
    } else if (lane == 0 && lp.metric != nullptr) {
        lp.metric[w] = m;
    }
}

// ---- the encoders, alone (wofdm_conv_encode, wofdm_ldpc_encode) and inside the coset instantiations of the two decoders ----

// A | B << 1 of step t from r = (u_t << 6) | state, whose bit j is u_(t - 6 + j): each a parity of seven information bits
__device__ __forceinline__ uint32_t conv_ab(uint32_t r)
{
    return (uint32_t)(__popc(r & 0133u) & 1) | ((uint32_t)(__popc(r & 0171u) & 1) << 1);
}

// The K = 7 encoder of include/wofdm.h (wofdm_convencparams): one step per lane, grid (n_cw, ceil(T / 256)).  Lane t gathers u_(t
// - 6) ... u_t -- zero before the word and on the six tail steps --, forms A and B and stores them at their closed-form
// positions; the last step's lane also clears the positions behind the kept outputs.
__global__ void __launch_bounds__(256) wofdm_conv_encode_kernel(const wofdm_convencparams ep)
{
    const int t = (int)(blockIdx.y * 256u + threadIdx.x), T = ep.steps, K = T - 6, n_c = ep.n_c;
    if (t >= T) return;
    const uint8_t *__restrict__ info = ep.info + (uint64_t)blockIdx.x * (uint64_t)K;
    uint8_t *__restrict__ out = ep.coded + (uint64_t)blockIdx.x * (uint64_t)n_c;
    uint32_t r = 0u;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const int i = t - 6 + j;
        r |= (i >= 0 && i < K ? (uint32_t)info[i] & 1u : 0u) << j;
    }
    int ca, cb;
    conv_kept(ep.rate, t, ca, cb);
    const uint32_t ab = conv_ab(r);
    if (ca >= 0 && ca < n_c) out[ca] = (uint8_t)(ab & 1u);
    if (cb >= 0 && cb < n_c) out[cb] = (uint8_t)(ab >> 1);
    if (t == T - 1)
        for (int c = max(ca, cb) + 1; c < n_c; ++c) out[c] = 0;
}

// s(i, j) = (i 2^j) mod Z into sh [J L]: the decoders' and the encoder's shifts
__device__ __forceinline__ void ldpc_shifts(int16_t *__restrict__ sh, int J, int L, int Z, int tid, int nt)
{
    for (int x = tid; x < J * L; x += nt) {
        const int i = x / L, j = x - i * L;
        int p = 1 % Z;
        for (int q = 0; q < j; ++q) {
            p += p;
            p = p >= Z ? p - Z : p;
        }
        sh[x] = (int16_t)((i * p) % Z);
    }
}
// a codeword as bits in LDS: variable v is bit v mod 32 of word v div 32
__device__ __forceinline__ uint32_t ldpc_bit(const uint32_t *xb, int v) { return (xb[v >> 5] >> (v & 31)) & 1u; }

// The encoder of include/wofdm.h on a word held as bits in LDS: back-substitution from block row J - 1 up to 0 -- check r of row
// i XORs x[j Z + (r + s(i, j)) mod Z] over j > i into variable i Z + (r + s(i, i)) mod Z.  A row reads block columns above its
// own and writes its own: its Z checks are independent, strided over the threads, and an LDS atomic OR sets the bit (neighbours
// share a word).  Entered behind a barrier that left sh, the information bits and zeros everywhere else; one barrier per row.
__device__ __forceinline__ void ldpc_encode_lds(uint32_t *xb, const int16_t *__restrict__ sh, int J, int L, int Z, int tid, int nt)
{
    for (int i = J - 1; i >= 0; --i) {
        const int16_t *__restrict__ si = sh + i * L;
        for (int r = tid; r < Z; r += nt) {
            uint32_t par = 0u;
            for (int j = i + 1; j < L; ++j) {
                int c = r + si[j];
                c = c >= Z ? c - Z : c;
                par ^= ldpc_bit(xb, j * Z + c);
            }
            int c = r + si[i];
            c = c >= Z ? c - Z : c;
            const int v = i * Z + c;
            if (par != 0u) atomicOr(&xb[v >> 5], 1u << (v & 31));
        }
        __syncthreads();
    }
}

// wofdm_ldpc_encode (wofdm_ldpcencparams): one workgroup per codeword, the word as bits in LDS behind the shifts (288 bytes)
#define WOFDM_LDPC_ENC_HEAD 288            // 6 x 24 int16 shifts
__global__ void __launch_bounds__(256) wofdm_ldpc_encode_kernel(const wofdm_ldpcencparams ep)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char esm[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int J = ep.J, L = ep.L, n = ep.n, Z = ep.Z, k0 = J * Z, words = (L * Z + 31) >> 5;
    int16_t *__restrict__ sh = reinterpret_cast<int16_t *>(esm);
    uint32_t *xb = reinterpret_cast<uint32_t *>(esm + WOFDM_LDPC_ENC_HEAD);
    const uint8_t *__restrict__ info = ep.info + (uint64_t)blockIdx.x * (uint64_t)(n - k0);
    ldpc_shifts(sh, J, L, Z, tid, nt);
    for (int x = tid; x < words; x += nt) {
        uint32_t wv = 0u;
        for (int b = 0; b < 32; ++b) {
            const int v = 32 * x + b;
            wv |= (v >= k0 && v < n ? (uint32_t)info[v - k0] & 1u : 0u) << b;
        }
        xb[x] = wv;
    }
    __syncthreads();
    ldpc_encode_lds(xb, sh, J, L, Z, tid, nt);
    uint8_t *__restrict__ out = ep.word + (uint64_t)blockIdx.x * (uint64_t)n;
    for (int x = tid; x < n; x += nt) out[x] = (uint8_t)ldpc_bit(xb, x);
}

// 32 bits of the information stream of (cell, frame) from bit `start` > -32 on; a bit below 0 reads 0
__device__ __forceinline__ uint32_t coset_bits32(const wofdm_cosetparams &cs, uint32_t cell, uint64_t frame, int start)
{
    if (start < 0) return wofdm_info_word(cs.seed_lo, cs.seed_hi, cell, frame, 0u) << (-start);
    const uint32_t q = (uint32_t)start >> 5, sft = (uint32_t)start & 31u;
    const uint32_t lo = wofdm_info_word(cs.seed_lo, cs.seed_hi, cell, frame, q);
    return sft == 0u ? lo : (lo >> sft) | (wofdm_info_word(cs.seed_lo, cs.seed_hi, cell, frame, q + 1u) << (32u - sft));
}

// wofdm_viterbi_long_kernel in the coset view (wofdm_rx_profile_coset): the transmitted word is conv_encode of the frame's
// information stream, bits 0 ... T - 7, and the decoder sees d' = x_c ? -d : d.  The stream comes as one Philox block per 128
// steps, kept as two 64-bit words (wave-uniform); lane l forms the register of step 64 b + l from the block's word and the six
// bits before it, its A and B by conv_ab, and flips its pair before the block is walked.  The traceback draws the blocks again,
// descending, and XORs a block's 64 decoded bits with the stream's (the tail's are zero): what is left are the errors, counted
// as wofdm_viterbi_long_kernel counts the ones.  The loads ahead of a block (vlong_offsets, vlong_pair) are that kernel's
// functions; the two block walks -- step, back, their unrolled and partial loops -- and the information-bit mask are a COPY of
// that kernel's and have to change with them: behind shared walkers this kernel spills 16 SGPRs where it spills none now
// (profiles/code_unit.txt, section 4).
__global__ void __launch_bounds__(64) wofdm_viterbi_coset_kernel(const wofdm_longparams lp, const wofdm_cosetparams cs)
{
    const int lane = threadIdx.x;
    const uint64_t w = blockIdx.x;
    const int pt = (int)(w % (uint64_t)lp.n_points);
    const int v = lp.pts[pt].post != 0 ? 1 : 0;
    const int rate = lp.rate, T = lp.steps[v], n_c = lp.n_c[v];
    if (T < 7) return;                                                  // (a point without a data symbol: wave-uniform)
    const int n_blocks = (T + 63) >> 6;
    const int32_t *__restrict__ gather = lp.gather[v];
    const int8_t *__restrict__ soft = lp.soft + (int64_t)w * lp.cw_stride;
    unsigned long long *__restrict__ hist = lp.hist + (size_t)w * (size_t)lp.hist_blocks * 64;
    const uint64_t item = lp.item0 + w / (uint64_t)lp.n_points, cell = item / lp.frames;
    const uint64_t frame = cs.frame_offset + (item - cell * lp.frames);

    // the stream's bits 64 b ... 64 b + 63, those of the tail (t >= T - 6) zero
    int drawn = -1;
    unsigned long long even = 0ull, odd = 0ull;
    const auto stream64 = [&](int b) {
        if ((b >> 1) != drawn) {
            drawn = b >> 1;
            const philox_out o = philox4x32_10((uint32_t)drawn, (uint32_t)frame, (uint32_t)(frame >> 32),
                                               (WOFDM_STREAM_INFO << 28) | (uint32_t)cell, cs.seed_lo, cs.seed_hi);
            even = ((unsigned long long)o.w[1] << 32) | o.w[0];
            odd = ((unsigned long long)o.w[3] << 32) | o.w[2];
        }
        const int lim = T - 6 - 64 * b;
        const unsigned long long im = lim >= 64 ? ~0ull : (lim <= 0 ? 0ull : (1ull << lim) - 1ull);
        return ((b & 1) != 0 ? odd : even) & im;
    };

    const int p0 = (lane << 1) & 63, u = lane >> 5, r0 = (u << 6) | p0;
    const bool a0 = (__popc(r0 & 0133) & 1) != 0, b0 = (__popc(r0 & 0171) & 1) != 0;
    int m = lane == 0 ? 0 : (1 << 30);
    uint32_t hlo, hhi;
    const vlong_i16x2 sel0 = {(short)(a0 ? 1 : 0), (short)(b0 ? 1 : 0)}, sel1 = {(short)(a0 ? 0 : 1), (short)(b0 ? 0 : 1)};
    const auto step = [&](int i, int pair) {
        const vlong_i16x2 d = __builtin_bit_cast(vlong_i16x2, pair);
        const int c0 = __builtin_amdgcn_sdot2(sel0, d, __shfl(m, p0, 64), false);
        const int c1 = __builtin_amdgcn_sdot2(sel1, d, __shfl(m, p0 | 1, 64), false);
        const bool dec = c1 < c0;
        m = dec ? c1 : c0;
        if (i < 32)
            hlo |= dec ? 1u << i : 0u;
        else
            hhi |= dec ? 1u << (i - 32) : 0u;
    };
    int dp, oa, ob;
    vlong_offsets(gather, rate, n_c, T, lane, oa, ob);
    dp = vlong_pair(soft, oa, ob);
    vlong_offsets(gather, rate, n_c, T, 64 + lane, oa, ob);
    unsigned long long before = 0ull;                                    // the stream's word of block b - 1
    for (int b = 0; b < n_blocks; ++b) {
        int noa, nob;
        const int ndp = vlong_pair(soft, oa, ob);                        // block b + 1 (zeros behind the codeword's end)
        vlong_offsets(gather, rate, n_c, T, 64 * (b + 2) + lane, noa, nob);
        // the transmitted pair of step 64 b + lane, and d' for both of its outputs (|d| <= 127: the negation is exact)
        const unsigned long long cur = stream64(b);
        const uint32_t ab = conv_ab((uint32_t)((lane >= 6 ? cur >> (lane - 6) : (cur << (6 - lane)) | (before >> (58 + lane))) & 0x7Full));
        const int da = (int)(short)(dp & 0xFFFF), db = dp >> 16;
        const int fp = (int)(((uint32_t)((ab & 1u) != 0u ? -da : da) & 0xFFFFu) | ((uint32_t)((ab & 2u) != 0u ? -db : db) << 16));
        hlo = hhi = 0u;
        const int n = T - 64 * b;
        if (n >= 64) {
#pragma unroll
            for (int i = 0; i < 64; ++i) step(i, __builtin_amdgcn_readlane(fp, i));
        } else {
            for (int i = 0; i < n; ++i) step(i, __builtin_amdgcn_readlane(fp, i));
        }
        hist[(size_t)b * 64 + (size_t)lane] = ((unsigned long long)hhi << 32) | (unsigned long long)hlo;
        dp = ndp; oa = noa; ob = nob;
        before = cur;
    }
    // (a lane reads back what it stored itself: program order, no fence is needed)
    int st = 0, info = 0;
    bool any = false;
    for (int b = n_blocks - 1; b >= 0; --b) {
        const unsigned long long hw = hist[(size_t)b * 64 + (size_t)lane];
        const int wlo = (int)(uint32_t)hw, whi = (int)(uint32_t)(hw >> 32);
        const int n = T - 64 * b;
        unsigned long long mask = 0ull;
        const auto back = [&](int i) {
            const uint32_t word = (uint32_t)__builtin_amdgcn_readlane(i < 32 ? wlo : whi, st);
            mask |= (unsigned long long)(st >> 5) << i;
            st = ((st << 1) & 63) | (int)((word >> (i & 31)) & 1u);
        };
        if (n >= 64) {
#pragma unroll
            for (int i = 63; i >= 0; --i) back(i);
        } else {
            for (int i = n - 1; i >= 0; --i) back(i);
        }
        mask ^= stream64(b);
        const int lim = T - 6 - 64 * b;
        const unsigned long long im = lim >= 64 ? ~0ull : (lim <= 0 ? 0ull : (1ull << lim) - 1ull);
        info += __popcll(mask & im);
        any = any || mask != 0ull;
    }
    if (lane == 0 && any) {
        unsigned long long *e = lp.errs + (((uint64_t)pt * lp.cells + cell) * (uint64_t)lp.n_codes + (uint64_t)lp.code) * 2;
        if (info != 0) atomicAdd(e, (unsigned long long)info);
        atomicAdd(e + 1, 1ull);
    }
}

// The layered, normalised min-sum decoder of the quasi-cyclic (J, L) code of include/wofdm.h (wofdm_ldpcparams): pure integer,
// held bit for bit to the numpy mirror.  One workgroup per codeword of blockDim.x = 64 ... 256 threads (the launcher: Z rounded up
// to waves); Q (int16) and R (int8) live in LDS for the whole decode, the soft bits are gathered straight into Q.
//   A layer i touches every variable at most once -- block column j holds one circulant of the block row --, so its Z checks
// are independent and are strided over the threads; check r of layer i reads variable j Z + (r + s(i, j)) mod Z and R at
// [edge][r]: consecutive threads, consecutive LDS words (R) or a rotation of them (Q).  Two passes over a check's edges: the
// first finds the two smallest magnitudes of t = Q - R and the parity of the signs, the second forms t again and stores the new
// R and Q; t is not kept in registers (the degree is up to 24 and not a compile-time number).  A barrier ends every layer.
//   After the J layers the syndrome: every thread ORs the parities of its checks, the workgroup's OR (__syncthreads_or) is the
// stop decision of ALL threads -- the barriers and the iteration loop's trip count are workgroup-uniform; the strided loops
// between two barriers hold none.  |Q| <= 128 + 6 * 95: int16 never saturates.
//   The three kernels (wofdm_ldpc_kernel, wofdm_ldpc_coset_kernel, wofdm_ldpc_harq_kernel) differ in what they put into Q and
// in what they report; the decode between the two is ldpc_minsum, and the steps around it that they share are the helpers below.

// One decode on a Q and an R that the caller has filled, behind a barrier: up to max_iter iterations of the J layers and the
// syndrome.  Returns whether the syndrome vanished -- the workgroup's OR,
// so the answer, *iters and the barriers are workgroup-uniform -- and leaves behind a barrier: the last statement every thread
// ran is the __syncthreads_or, after which nobody reads Q or R of this decode any more.
__device__ __forceinline__ bool ldpc_minsum(int16_t *__restrict__ Q, int8_t *__restrict__ R, const int16_t *__restrict__ sh, int J, int L,
                                            int Z, int max_iter, int tid, int nt, int *iters)
{
    int it = 0;
    bool conv = false;
    while (it < max_iter) {
        int eb = 0;
        for (int i = 0; i < J; ++i) {
            const int deg = L - i;
            const int16_t *__restrict__ si = sh + i * L + i;
            for (int r = tid; r < Z; r += nt) {
                int m1 = 255, m2 = 255, par = 0;
                for (int e = 0; e < deg; ++e) {
                    int c = r + si[e];
                    c = c >= Z ? c - Z : c;
                    const int t = (int)Q[(i + e) * Z + c] - (int)R[(eb + e) * Z + r];
                    const int a = min(abs(t), 127);
                    par ^= t < 0 ? 1 : 0;
                    if (a < m1) {
                        m2 = m1;
                        m1 = a;
                    } else if (a < m2) {
                        m2 = a;
                    }
                }
                const int g1 = (3 * m1) >> 2, g2 = (3 * m2) >> 2;
                for (int e = 0; e < deg; ++e) {
                    int c = r + si[e];
                    c = c >= Z ? c - Z : c;
                    const int qi = (i + e) * Z + c, ri = (eb + e) * Z + r;
                    const int t = (int)Q[qi] - (int)R[ri];
                    const int a = min(abs(t), 127);
                    const int mag = a == m1 ? g2 : g1;
                    const int rn = (par ^ (t < 0 ? 1 : 0)) != 0 ? -mag : mag;
                    R[ri] = (int8_t)rn;
                    Q[qi] = (int16_t)(t + rn);
                }
            }
            eb += deg;
            __syncthreads();
        }
        ++it;
        // the syndrome of the hard decisions
        int bad = 0;
        for (int i = 0; i < J; ++i) {
            const int deg = L - i;
            const int16_t *__restrict__ si = sh + i * L + i;
            for (int r = tid; r < Z; r += nt) {
                int par = 0;
                for (int e = 0; e < deg; ++e) {
                    int c = r + si[e];
                    c = c >= Z ? c - Z : c;
                    par ^= (int)Q[(i + e) * Z + c] < 0 ? 1 : 0;
                }
                bad |= par;
            }
        }
        // (a barrier as well: nobody writes Q for the next layer before everybody has read it)
        if (__syncthreads_or(bad) == 0) {
            conv = true;
            break;
        }
    }
    *iters = it;
    return conv;
}

// R = 0 over the layers' edges, whole words (R ends on one)
__device__ __forceinline__ void ldpc_zero_R(int8_t *R, int J, int L, int Z, int tid, int nt)
{
    uint32_t *__restrict__ R4 = reinterpret_cast<uint32_t *>(R);
    const int words = ((J * L - J * (J - 1) / 2) * Z + 3) >> 2;
    for (int x = tid; x < words; x += nt) R4[x] = 0u;
}
// The wrong information bits -- variables J Z ... n - 1 whose decision is not the word's bit; WORD off: the all-zero word, xb
// is not read -- of the workgroup into cnt[0], which a thread may read behind the barrier this ends in
template <bool WORD>
__device__ __forceinline__ void ldpc_count_wrong(int *cnt, const int16_t *Q, const uint32_t *xb, int J, int Z, int n, int tid, int nt)
{
    int wrong = 0;
    for (int x = J * Z + tid; x < n; x += nt) wrong += (Q[x] < 0 ? 1u : 0u) != (WORD ? ldpc_bit(xb, x) : 0u) ? 1 : 0;
    if (wrong != 0) atomicAdd(&cnt[0], wrong);
    __syncthreads();
}

// wofdm_rx_profile_ldpc and wofdm_ldpc_decode: the all-zero word, the soft bits gathered straight into Q
__global__ void __launch_bounds__(256) wofdm_ldpc_kernel(const wofdm_ldpcparams lp)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lsm[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const uint64_t w = blockIdx.x;
    const int wi = blockIdx.y;
    int v = 0, pt = 0;
    if (lp.errs != nullptr) {
        pt = (int)(w % (uint64_t)lp.n_points);
        v = lp.pts[pt].post != 0 ? 1 : 0;
    }
    if (wi >= lp.W[v]) return;                                          // (workgroup-uniform, before the first barrier)
    const int J = lp.J, L = lp.L, n = lp.n[v], Z = lp.Z[v], n0 = L * Z;
    // (the carve-up of wofdm_ldpc_lds, by the functions that size it: cnt [4], sh [J L], Q [L Z], R [edge][Z])
    int *cnt = reinterpret_cast<int *>(lsm);
    int16_t *sh = reinterpret_cast<int16_t *>(lsm + 16);
    int16_t *Q = reinterpret_cast<int16_t *>(lsm + WOFDM_LDPC_LDS_HEAD);
    int8_t *R = reinterpret_cast<int8_t *>(lsm + WOFDM_LDPC_LDS_HEAD + wofdm_ldpc_q_bytes(n0));
    const int8_t *__restrict__ soft = lp.soft + (int64_t)w * lp.cw_stride;
    const int32_t *__restrict__ gather = lp.gather[v] + (size_t)wi * (size_t)n;

    if (tid < 4) cnt[tid] = 0;
    ldpc_shifts(sh, J, L, Z, tid, nt);
    for (int x = tid; x < n0; x += nt) Q[x] = x < n ? (int16_t)soft[gather[x]] : (int16_t)127;
    ldpc_zero_R(R, J, L, Z, tid, nt);
    __syncthreads();

    int it = 0;
    const bool conv = ldpc_minsum(Q, R, sh, J, L, Z, lp.max_iter, tid, nt, &it);

    if (lp.errs == nullptr) {
        uint8_t *__restrict__ out = lp.bits + w * (uint64_t)n;
        for (int x = tid; x < n; x += nt) out[x] = Q[x] < 0 ? 1 : 0;
        if (tid == 0) {
            if (lp.iters != nullptr) lp.iters[w] = it;
            if (lp.conv != nullptr) lp.conv[w] = conv ? 1 : 0;
        }
    } else {
        ldpc_count_wrong<false>(cnt, Q, nullptr, J, Z, n, tid, nt);
        if (tid == 0) {
            const uint64_t job = w / (uint64_t)lp.n_points, cell = (lp.item0 + job) / lp.frames;
            unsigned long long *e = lp.errs + (((uint64_t)pt * lp.cells + cell) * (uint64_t)lp.n_codes + (uint64_t)lp.code) * 4;
            const int info = cnt[0];
            if (info != 0) {
                atomicAdd(e, (unsigned long long)info);
                atomicAdd(e + 1, 1ull);
            }
            if (!conv) atomicAdd(e + 2, 1ull);
            atomicAdd(e + 3, (unsigned long long)it);
        }
    }
}

// wofdm_ldpc_kernel in the coset view (wofdm_rx_profile_coset): word wi of the frame carries the information stream's bits wi n
// ... wi n + K - 1 on variables J Z ... n - 1.  The workgroup draws them into LDS as bits (behind R: wofdm_ldpc_coset_lds),
// encodes them there (ldpc_encode_lds), flips the signs while it gathers into Q -- d' = x ? -d : d --, and compares the decisions
// with the kept word at the end.
__global__ void __launch_bounds__(256) wofdm_ldpc_coset_kernel(const wofdm_ldpcparams lp, const wofdm_cosetparams cs)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lsm[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const uint64_t w = blockIdx.x;
    const int wi = blockIdx.y;
    const int pt = (int)(w % (uint64_t)lp.n_points);
    const int v = lp.pts[pt].post != 0 ? 1 : 0;
    if (wi >= lp.W[v]) return;                                          // (workgroup-uniform, before the first barrier)
    const int J = lp.J, L = lp.L, n = lp.n[v], Z = lp.Z[v], n0 = L * Z;
    // (the carve-up of wofdm_ldpc_lds, by the functions that size it: cnt [4], sh [J L], Q [L Z], R [edge][Z])
    int *cnt = reinterpret_cast<int *>(lsm);
    int16_t *sh = reinterpret_cast<int16_t *>(lsm + 16);
    int16_t *Q = reinterpret_cast<int16_t *>(lsm + WOFDM_LDPC_LDS_HEAD);
    int8_t *R = reinterpret_cast<int8_t *>(lsm + WOFDM_LDPC_LDS_HEAD + wofdm_ldpc_q_bytes(n0));
    uint32_t *xb = reinterpret_cast<uint32_t *>(R + wofdm_ldpc_r_bytes(J, L, Z));   // [ceil(L Z / 32)], behind it: wofdm_ldpc_coset_lds
    const int8_t *__restrict__ soft = lp.soft + (int64_t)w * lp.cw_stride;
    const int32_t *__restrict__ gather = lp.gather[v] + (size_t)wi * (size_t)n;
    const uint64_t item = lp.item0 + w / (uint64_t)lp.n_points, cell = item / lp.frames;
    const uint64_t frame = cs.frame_offset + (item - cell * lp.frames);

    if (tid < 4) cnt[tid] = 0;
    ldpc_shifts(sh, J, L, Z, tid, nt);
    // the information bits: variable x >= J Z is bit wi n + x - J Z of the stream; a thread fills whole words, zeros elsewhere
    // (written out here and in wofdm_ldpc_harq_kernel: as a shared function the loop compiles differently in both)
    for (int x = tid; x < (n0 + 31) >> 5; x += nt) {
        const int lo = max(32 * x, J * Z) - 32 * x, hi = min(32 * x + 32, n) - 32 * x;
        uint32_t wv = 0u;
        if (lo < hi) {
            const uint32_t keep = (hi == 32 ? ~0u : (1u << hi) - 1u) & ~((1u << lo) - 1u);
            wv = coset_bits32(cs, (uint32_t)cell, frame, wi * n + 32 * x - J * Z) & keep;
        }
        xb[x] = wv;
    }
    ldpc_zero_R(R, J, L, Z, tid, nt);
    __syncthreads();
    ldpc_encode_lds(xb, sh, J, L, Z, tid, nt);
    for (int x = tid; x < n0; x += nt) {
        const int d = x < n ? (int)soft[gather[x]] : 127;                // (a shortened position is a sure 0 of the word)
        Q[x] = (int16_t)(ldpc_bit(xb, x) != 0u ? -d : d);
    }
    __syncthreads();

    int it = 0;
    const bool conv = ldpc_minsum(Q, R, sh, J, L, Z, lp.max_iter, tid, nt, &it);

    ldpc_count_wrong<true>(cnt, Q, xb, J, Z, n, tid, nt);
    if (tid == 0) {
        unsigned long long *e = lp.errs + (((uint64_t)pt * lp.cells + cell) * (uint64_t)lp.n_codes + (uint64_t)lp.code) * 4;
        const int info = cnt[0];
        if (info != 0) {
            atomicAdd(e, (unsigned long long)info);
            atomicAdd(e + 1, 1ull);
        }
        if (!conv) atomicAdd(e + 2, 1ull);
        atomicAdd(e + 3, (unsigned long long)it);
    }
}

// Retransmissions with soft combining (wofdm_rx_profile_harq, wofdm_ldpc_harq_decode; include/wofdm.h has the scheme): one
// workgroup per (group, point, word of the frame) and launch per code.  The word is drawn from the information stream of the
// group's FIRST frame and encoded once, as wofdm_ldpc_coset_kernel does; every round re-forms Q from the rows so far in device
// memory -- int32 sums of d' = x ? -d : d, clamped to +-127, no running sum in LDS --, zeroes R and decodes afresh (ldpc_minsum).
// The first round whose syndrome vanishes ends the word; that is the workgroup's OR, so the round loop's trip count and every
// barrier are workgroup-uniform.  A round's decode leaves behind a barrier, so the next round may write Q and R at once.
//   The decoder alone (lp.errs null): no word -- the caller's rows are the d' --, the decisions, the stop round, the iterations
// over all rounds and the ACK go out per word.  LDS: wofdm_ldpc_coset_lds in both uses.
__global__ void __launch_bounds__(256) wofdm_ldpc_harq_kernel(const wofdm_ldpcparams lp, const wofdm_cosetparams cs,
                                                              const wofdm_harqparams hq)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lsm[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const uint64_t w = blockIdx.x;
    const int wi = blockIdx.y;
    const bool profile = lp.errs != nullptr;
    const int rounds = hq.rounds;
    int v = 0, pt = 0;
    uint64_t row0 = w * (uint64_t)rounds, row_step = 1, cell = 0, frame = 0;
    if (profile) {
        const uint64_t grp = w / (uint64_t)lp.n_points;
        pt = (int)(w - grp * (uint64_t)lp.n_points);
        v = lp.pts[pt].post != 0 ? 1 : 0;
        row_step = (uint64_t)lp.n_points;
        row0 = grp * (uint64_t)rounds * row_step + (uint64_t)pt;
        const uint64_t item = lp.item0 + grp * (uint64_t)rounds;
        cell = item / lp.frames;
        frame = cs.frame_offset + (item - cell * lp.frames);
    }
    if (wi >= lp.W[v]) return;                                          // (workgroup-uniform, before the first barrier)
    const int J = lp.J, L = lp.L, n = lp.n[v], Z = lp.Z[v], n0 = L * Z;
    // (the carve-up of wofdm_ldpc_lds, by the functions that size it: cnt [4], sh [J L], Q [L Z], R [edge][Z])
    int *cnt = reinterpret_cast<int *>(lsm);
    int16_t *sh = reinterpret_cast<int16_t *>(lsm + 16);
    int16_t *Q = reinterpret_cast<int16_t *>(lsm + WOFDM_LDPC_LDS_HEAD);
    int8_t *R = reinterpret_cast<int8_t *>(lsm + WOFDM_LDPC_LDS_HEAD + wofdm_ldpc_q_bytes(n0));
    uint32_t *xb = reinterpret_cast<uint32_t *>(R + wofdm_ldpc_r_bytes(J, L, Z));   // [ceil(L Z / 32)], behind it: wofdm_ldpc_coset_lds
    const int32_t *__restrict__ gather = lp.gather[v] + (size_t)wi * (size_t)n;

    if (tid < 4) cnt[tid] = 0;
    ldpc_shifts(sh, J, L, Z, tid, nt);
    // the information bits as in wofdm_ldpc_coset_kernel; the decoder alone keeps the all-zero word, which flips nothing
    for (int x = tid; x < (n0 + 31) >> 5; x += nt) {
        const int lo = max(32 * x, J * Z) - 32 * x, hi = min(32 * x + 32, n) - 32 * x;
        uint32_t wv = 0u;
        if (profile && lo < hi) {
            const uint32_t keep = (hi == 32 ? ~0u : (1u << hi) - 1u) & ~((1u << lo) - 1u);
            wv = coset_bits32(cs, (uint32_t)cell, frame, wi * n + 32 * x - J * Z) & keep;
        }
        xb[x] = wv;
    }
    __syncthreads();
    if (profile) ldpc_encode_lds(xb, sh, J, L, Z, tid, nt);           // (workgroup-uniform; ends in a barrier)

    int total = 0, rd = 0;
    bool conv = false;
    for (rd = 0; rd < rounds; ++rd) {
        const int first = hq.combine != 0 ? 0 : rd;
        for (int x = tid; x < n0; x += nt) {
            int q = 127;                                                 // (a shortened position is a sure 0 of the word)
            if (x < n) {
                const int32_t at = gather[x];
                const bool flip = ldpc_bit(xb, x) != 0u;
                q = 0;
                for (int j = first; j <= rd; ++j) {
                    const int d = (int)lp.soft[(int64_t)(row0 + (uint64_t)j * row_step) * lp.cw_stride + at];
                    q += flip ? -d : d;
                }
                q = min(max(q, -127), 127);
            }
            Q[x] = (int16_t)q;
        }
        {
            // (R = 0 as ldpc_zero_R does it, written out: called here, the function changes the encoding of a scalar add in the
            // syndrome's loop -- profiles/code_unit.txt, section 3)
            uint32_t *__restrict__ R4 = reinterpret_cast<uint32_t *>(R);
            const int words = ((J * L - J * (J - 1) / 2) * Z + 3) >> 2;
            for (int x = tid; x < words; x += nt) R4[x] = 0u;
        }
        __syncthreads();
        int it = 0;
        conv = ldpc_minsum(Q, R, sh, J, L, Z, lp.max_iter, tid, nt, &it);
        total += it;
        if (conv) break;                                                 // (the ACK: workgroup-uniform)
    }
    const int stop = conv ? rd + 1 : rounds;

    if (!profile) {
        uint8_t *__restrict__ out = lp.bits + w * (uint64_t)n;
        for (int x = tid; x < n; x += nt) out[x] = Q[x] < 0 ? 1 : 0;
        if (tid == 0) {
            if (hq.round != nullptr) hq.round[w] = stop;
            if (lp.iters != nullptr) lp.iters[w] = total;
            if (lp.conv != nullptr) lp.conv[w] = conv ? 1 : 0;
        }
    } else {
        ldpc_count_wrong<true>(cnt, Q, xb, J, Z, n, tid, nt);
        if (tid == 0) {
            unsigned long long *e = lp.errs + (((uint64_t)pt * lp.cells + cell) * (uint64_t)lp.n_codes + (uint64_t)lp.code) * WOFDM_HARQ_NF;
            const int info = cnt[0];
            atomicAdd(e + (conv ? stop - 1 : 8), 1ull);
            if (info != 0) {
                atomicAdd(e + 9, 1ull);
                if (conv) atomicAdd(e + 10, 1ull);
                atomicAdd(e + 11, (unsigned long long)info);
            }
            atomicAdd(e + 12, (unsigned long long)total);
        }
    }
}

// ---- the host side: the checks in front of the device, the launches ----

// wofdm_viterbi_kernel's LDS: 11 bytes per step of the longest code
unsigned viterbi_lds(const wofdm_codeparams &cd)
{
    int T = 0;
    for (int i = 0; i < cd.n_codes; ++i) T = cd.steps[i] > T ? cd.steps[i] : T;
    return 11u * (unsigned)T;
}
// the streaming decoder: the variants in use (profile: both may be, and one without a codeword has steps 0), the history's room
bool viterbi_long_ok(const wofdm_longparams &lp, bool profile)
{
    if (lp.rate < 0 || lp.rate > 2 || lp.soft == nullptr || lp.hist == nullptr || lp.n_cw < 1 || lp.hist_blocks < 1) return false;
    for (int v = 0; v < (profile ? 2 : 1); ++v) {
        if (profile && lp.steps[v] == 0) continue;
        if (lp.steps[v] < 7 || lp.steps[v] > WOFDM_CODE_LONG_STEPS || lp.n_c[v] < 1 || lp.gather[v] == nullptr ||
            (lp.steps[v] + 63) / 64 > lp.hist_blocks)
            return false;
    }
    return profile ? lp.errs != nullptr && lp.pts != nullptr && lp.n_points >= 1 && lp.code >= 0 && lp.code < lp.n_codes &&
                         lp.bits == nullptr && lp.frames >= 1
                   : lp.errs == nullptr && lp.bits != nullptr;
}
// the LDPC decoder: the code, the variants in use (profile: both may be, one with W = 0 is unused), the LDS
bool ldpc_ok(const wofdm_ldpcparams &lp, bool profile)
{
    if (lp.J < 3 || lp.J > 6 || lp.L <= lp.J || lp.L > 24 || lp.max_iter < 1 || lp.max_iter > 64 || lp.soft == nullptr || lp.n_cw < 1)
        return false;
    for (int v = 0; v < (profile ? 2 : 1); ++v) {
        if (profile && lp.W[v] == 0) continue;
        if (lp.W[v] < 1 || lp.n[v] < 1 || lp.n[v] > WOFDM_LDPC_BITS || lp.gather[v] == nullptr || lp.Z[v] < lp.L ||
            (int64_t)lp.L * lp.Z[v] < lp.n[v] || lp.J * lp.Z[v] >= lp.n[v] || lp.Z[v] > 32767 ||
            wofdm_ldpc_lds(lp.J, lp.L, lp.Z[v]) > WOFDM_LDPC_LDS_MAX)
            return false;
    }
    return profile ? lp.errs != nullptr && lp.pts != nullptr && lp.n_points >= 1 && lp.code >= 0 && lp.code < lp.n_codes &&
                         lp.bits == nullptr && lp.frames >= 1
                   : lp.errs == nullptr && lp.bits != nullptr && lp.W[0] == 1;
}
// One launch of an LDPC kernel, whichever of the three: grid (n_cw, the most words per frame among the variants in use), Z
// rounded up to waves as the workgroup, at most 256 threads, and the LDS of the largest lift in use -- word: with the transmitted
// word's bits behind the decoder's (wofdm_ldpc_coset_lds) -- set as the kernel's attribute first.
template <class K, class... A>
hipError_t ldpc_enqueue_kernel(K kernel, bool word, const wofdm_ldpcparams &lp, bool profile, hipStream_t s, const A &...args)
{
    int Z = 0, W = 0;
    for (int v = 0; v < (profile ? 2 : 1); ++v) {
        if (lp.W[v] == 0) continue;
        Z = lp.Z[v] > Z ? lp.Z[v] : Z;
        W = lp.W[v] > W ? lp.W[v] : W;
    }
    if (W == 0) return hipSuccess;                                      // (no point carries a codeword)
    const uint64_t lds = word ? wofdm_ldpc_coset_lds(lp.J, lp.L, Z) : wofdm_ldpc_lds(lp.J, lp.L, Z);
    if (lds > WOFDM_LDPC_LDS_MAX) return hipErrorInvalidValue;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    const unsigned threads = (unsigned)(Z >= 256 ? 256 : ((Z + 63) / 64) * 64);
    hipLaunchKernelGGL(kernel, dim3(lp.n_cw, (unsigned)W), dim3(threads), (unsigned)lds, s, args...);
    return hipSuccess;
}

}  // namespace

// ---- what the per-N units call behind the receive kernel (wofdm_link.h) ----

// the per-symbol decoder: the codes, their steps (7 ... 4608: the decoder's LDS is 11 bytes per step) and the buffers
bool wofdm_viterbi_ok(const wofdm_codeparams &cd, bool profile)
{
    if (cd.n_codes < 1 || cd.n_codes > WOFDM_CODE_CODES || cd.n_c < 1 || cd.soft == nullptr || cd.gather == nullptr ||
        (profile && (cd.errs == nullptr || !(cd.llr_scale > 0.f))))
        return false;
    for (int i = 0; i < cd.n_codes; ++i)
        if (cd.rate[i] < 0 || cd.rate[i] > 2 || cd.steps[i] < 7 || cd.steps[i] > 4608) return false;
    return true;
}
void wofdm_viterbi_enqueue(const wofdm_codeparams &cd, hipStream_t s)
{
    hipLaunchKernelGGL(wofdm_viterbi_kernel, dim3(cd.n_cw, (unsigned)cd.n_codes), dim3(64), viterbi_lds(cd), s, cd);
}
hipError_t wofdm_viterbi_long_enqueue(const wofdm_longparams &lp, bool profile, hipStream_t s)
{
    if (!viterbi_long_ok(lp, profile)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wofdm_viterbi_long_kernel, dim3(lp.n_cw), dim3(64), 0, s, lp);
    return hipSuccess;
}
hipError_t wofdm_viterbi_coset_enqueue(const wofdm_longparams &lp, const wofdm_cosetparams &cs, hipStream_t s)
{
    if (!viterbi_long_ok(lp, true)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wofdm_viterbi_coset_kernel, dim3(lp.n_cw), dim3(64), 0, s, lp, cs);
    return hipSuccess;
}
hipError_t wofdm_ldpc_enqueue(const wofdm_ldpcparams &lp, bool profile, hipStream_t s)
{
    if (!ldpc_ok(lp, profile)) return hipErrorInvalidValue;
    return ldpc_enqueue_kernel(wofdm_ldpc_kernel, false, lp, profile, s, lp);
}
hipError_t wofdm_ldpc_coset_enqueue(const wofdm_ldpcparams &lp, const wofdm_cosetparams &cs, hipStream_t s)
{
    if (!ldpc_ok(lp, true)) return hipErrorInvalidValue;
    return ldpc_enqueue_kernel(wofdm_ldpc_coset_kernel, true, lp, true, s, lp, cs);
}
// (grid x: the words' first rows)
hipError_t wofdm_ldpc_harq_enqueue(const wofdm_ldpcparams &lp, const wofdm_cosetparams &cs, const wofdm_harqparams &hq, bool profile,
                                   hipStream_t s)
{
    if (!ldpc_ok(lp, profile) || hq.rounds < 1 || hq.rounds > WOFDM_HARQ_ROUNDS || (hq.combine != 0 && hq.combine != 1))
        return hipErrorInvalidValue;
    return ldpc_enqueue_kernel(wofdm_ldpc_harq_kernel, true, lp, profile, s, lp, cs, hq);
}

// ---- what the C ABI calls, on data of the caller's ----

// wofdm_viterbi_decode
hipError_t wofdm_viterbi_launch(const wofdm_codeparams *cd, hipStream_t s)
{
    if (!wofdm_viterbi_ok(*cd, false) || cd->n_codes != 1 || cd->bits == nullptr || cd->errs != nullptr || cd->n_cw < 1)
        return hipErrorInvalidValue;
    wofdm_viterbi_enqueue(*cd, s);
    return hipGetLastError();
}

// wofdm_viterbi_decode_long
hipError_t wofdm_viterbi_long_launch(const wofdm_longparams *lp, hipStream_t s)
{
    const hipError_t e = wofdm_viterbi_long_enqueue(*lp, false, s);
    return e != hipSuccess ? e : hipGetLastError();
}

// wofdm_ldpc_decode
hipError_t wofdm_ldpc_launch(const wofdm_ldpcparams *lp, hipStream_t s)
{
    const hipError_t e = wofdm_ldpc_enqueue(*lp, false, s);
    return e != hipSuccess ? e : hipGetLastError();
}

// wofdm_ldpc_harq_decode: no word is drawn, so no key
hipError_t wofdm_ldpc_harq_launch(const wofdm_ldpcparams *lp, const wofdm_harqparams *hq, hipStream_t s)
{
    const wofdm_cosetparams none{};
    const hipError_t e = wofdm_ldpc_harq_enqueue(*lp, none, *hq, false, s);
    return e != hipSuccess ? e : hipGetLastError();
}

// wofdm_conv_encode
hipError_t wofdm_conv_encode_launch(const wofdm_convencparams *ep, hipStream_t s)
{
    if (ep->info == nullptr || ep->coded == nullptr || ep->rate < 0 || ep->rate > 2 || ep->n_c < 1 || ep->steps < 7 ||
        ep->steps > WOFDM_CODE_LONG_STEPS || ep->n_cw < 1)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(wofdm_conv_encode_kernel, dim3(ep->n_cw, (unsigned)((ep->steps + 255) / 256)), dim3(256), 0, s, *ep);
    return hipGetLastError();
}

// wofdm_ldpc_encode
hipError_t wofdm_ldpc_encode_launch(const wofdm_ldpcencparams *ep, hipStream_t s)
{
    if (ep->info == nullptr || ep->word == nullptr || ep->J < 3 || ep->J > 6 || ep->L <= ep->J || ep->L > 24 || ep->n < 1 ||
        ep->n > WOFDM_LDPC_BITS || ep->Z < ep->L || (int64_t)ep->L * ep->Z < ep->n || ep->J * ep->Z >= ep->n || ep->Z > 32767 ||
        ep->n_cw < 1)
        return hipErrorInvalidValue;
    const unsigned lds = WOFDM_LDPC_ENC_HEAD + 4u * (unsigned)((ep->L * ep->Z + 31) / 32);
    const unsigned threads = (unsigned)(ep->Z >= 256 ? 256 : ((ep->Z + 63) / 64) * 64);
    hipLaunchKernelGGL(wofdm_ldpc_encode_kernel, dim3(ep->n_cw), dim3(threads), lds, s, *ep);
    return hipGetLastError();
}
