// bamd_matvec_b32.h — single-token mat-vec for the 32-weight block formats (bamd_formats.h): Q8_0 / Q4_0 / Q5_0 with the Q8_0 activation prologue, Q4_1 / Q5_1
// (the types with a minimum) with the Q8_1 one.  One wave per row-group (mode A) for both families and split-K (mode B) for the types without a minimum: it
// measured slower than one wave per row-group for the whole Q8_0 family (profiles/legacy_matvec.txt), so the types with a minimum never got one, and a request
// for it (mode 2) is refused by the caller in words.  The K-quant kernels (bamd_matvec.hip, bamd_matvec_fast_*.hip) are not touched by these types: a launch
// whose segments are all of one of the two families comes here (bamd_launch_mv, bamd_kernels.h), every other launch goes where it went before.
// IQ4_NL (Q8_0 activations, the Q4_0 record, two accumulators per lane) has mode A only; a request for split-K is refused in words like the one for Q4_1 / Q5_1.
// ONE source, THREE translation units: bamd_matvec_b32_q0.hip instantiates the kernels of the family without a minimum, bamd_matvec_b32_q1.hip those of the other,
// so each family keeps a code object of its own, as before the sources were one; bamd_matvec_b32_nl.hip holds a third kernel whose type list is Q8_0 / Q4_0 / Q5_0
// AND IQ4_NL, for the launches with at least one IQ4_NL segment (every other launch goes where it went before, its kernels instruction for instruction what they
// were).  Why a code object each: with both families in one, every instance was instruction for instruction what it had been and the Q4_1 qkv launch (6144 x 4096, RMSNorm) still measured 9.55 -> 10.29 us (profiles/b32_unify.txt).
//
// Numerics, records and the chains: bamd_b32_device.h.
#pragma once
#include "bamd_matvec_core.h"
#include "bamd_b32_device.h"

struct B32Lds { uint32_t * q8; float * ys; double * red; };
__device__ __forceinline__ B32Lds carve_lds_b32(const bamd_mv_args & a, unsigned char * smem) {
    const ProArgs pa = carve_lds(a, smem);
    B32Lds l; l.q8 = pa.q8; l.ys = (float *) pa.S; l.red = pa.red;
    return l;
}

// ---- MODE A: one wave per row-group (the streaming loop of stream_segment, bamd_matvec_core.h: a ring of D records, the loader one chunk ahead); with a minimum,
// beside the lane's chain the row's scalar chain ----
template <int TYPE, int D, int EPI, bool NORM>
__device__ __forceinline__ void b32_stream(const uint8_t * __restrict__ wA, const uint8_t * __restrict__ wB, int nb, int first, int count, int stride,
                                           float * __restrict__ out, const float * __restrict__ res, const bamd_mv_args & a, const B32Lds & L, bool do_pro,
                                           unsigned long long & best, int nvalid) {
    constexpr int RECB = BAMD_RECB_OF(TYPE);
    constexpr bool MIN = b32_has_min(TYPE);
    constexpr bool PAIR = EPI == BAMD_EPI_SILU_MUL;
    constexpr int NPARTS = PAIR ? 2 : 1;
    const int lane = threadIdx.x & 63;
    const bamd_rsrc rsA = weight_rsrc(wA), rsB = PAIR ? weight_rsrc(wB) : rsA, rsN = null_rsrc(wA);
    const int rgb = nb * RECB;
    const int rg_step = stride * rgb;
    const int chunks = nb / D;
    ActProQ0<NORM> ap;
    if (do_pro) ap.issue(a.x, a.normw, a.K, wave_id());     // activation loads go out first
    RecB32<TYPE> ring[D];
#pragma unroll
    for (int s = 0; s < D; ++s) load_rec(ring[s], rsA, first * rgb + s * RECB, lane);
    if (do_pro) ap.template finish_q0<MIN>(a.x, a.normw, a.eps, a.K, L.q8, L.ys, L.red);
    for (int r = 0; r < count; ++r) {
        const int rg = first + r * stride;
        const int row = rg * 8 + (lane >> 3);
        const int rowoff = rg * rgb;
        float gate_val = 0.f;
#pragma unroll
        for (int part = 0; part < NPARTS; ++part) {
            const bool last = !(PAIR && part == 0) && r + 1 >= count;
            const bool after_b = PAIR && part == 0;
            const int after_off = (PAIR && part == 0) ? rowoff : rowoff + rg_step;
            float resv = 0.f;
            if (EPI == BAMD_EPI_ADD && row < nvalid) resv = ik_ld(res + row);
            float acc = 0.f, acc2 = 0.f, summs = 0.f;        // (acc2: the odd blocks' accumulator of a type with two, b32_two_acc)
            for (int c = 0; c < chunks; ++c) {
                const bool inrow = c + 1 < chunks;
                const bool tail = !inrow && last;            // behind the wave's last chunk: the zero-record descriptor (returns 0, fetches nothing)
                const bamd_rsrc nrs = tail ? rsN : (inrow ? part == 1 : after_b) ? rsB : rsA;
                const int nxt = tail ? 0 : inrow ? rowoff + (c + 1) * (D * RECB) : after_off;
#pragma unroll
                for (int s = 0; s < D; ++s) {
                    pin_rec(ring[s]);
                    float sc[8], fd[8];                      // (declared here, not in a helper that takes acc and summs by reference: that costs 15 VGPRs)
                    if constexpr (MIN) {                     // (and no ms array where nothing writes it: see b32_terms)
                        float ms[8];
                        b32_terms(ring[s], c * D + s, lane, L.q8, L.ys, sc, fd, ms);
                        b32_chain8(acc, sc, fd);
                        b32_summs8(summs, ms);
                    } else {
                        b32_terms(ring[s], c * D + s, lane, L.q8, L.ys, sc, fd);
                        if constexpr (b32_two_acc(TYPE)) b32_chain8(acc, acc2, sc, fd);
                        else b32_chain8(acc, sc, fd);
                    }
                    load_rec(ring[s], nrs, nxt + s * RECB, lane);
                    if ((s & (BAMD_SCHED_GROUP - 1)) == BAMD_SCHED_GROUP - 1) __builtin_amdgcn_sched_barrier(0);
                }
            }
            const float val = b32_finish_row<MIN>(b32_two_acc(TYPE) ? acc + acc2 : acc, summs);
            if (PAIR) {
                if (part == 0) gate_val = val;
                else if ((lane & 7) == 0 && row < nvalid) ik_st(out + row, v_silu(gate_val) * val);
            } else if ((lane & 7) == 0 && row < nvalid) {
                float o = val;
                if (EPI == BAMD_EPI_ADD) o = val + resv;
                ik_st(out + row, o);
                if (EPI == BAMD_EPI_ARGMAX) { const unsigned long long k = argmax_key(o, row); best = k > best ? k : best; }
            }
        }
    }
}
template <int TYPE, int EPI, bool NORM>
__device__ __forceinline__ void b32_stream_depth(const uint8_t * wA, const uint8_t * wB, int nb, int first, int count, int stride, float * out, const float * res,
                                                 const bamd_mv_args & a, const B32Lds & L, bool do_pro, unsigned long long & best, int nvalid) {
    if ((nb & 3) == 0)      b32_stream<TYPE, 4, EPI, NORM>(wA, wB, nb, first, count, stride, out, res, a, L, do_pro, best, nvalid);
    else if ((nb & 1) == 0) b32_stream<TYPE, 2, EPI, NORM>(wA, wB, nb, first, count, stride, out, res, a, L, do_pro, best, nvalid);
    else                    b32_stream<TYPE, 1, EPI, NORM>(wA, wB, nb, first, count, stride, out, res, a, L, do_pro, best, nvalid);
}

// FAM: the type list of a launch (the weight type is a run-time property of a segment): without a minimum, with one, or the first with IQ4_NL beside it
enum { B32_FAM_Q0 = 0, B32_FAM_Q1 = 1, B32_FAM_NL = 2 };
// The translation unit names its mode A kernel and says whether the type list without a minimum holds IQ4_NL (bamd_matvec_b32_nl.hip: matvec_b32_nl_kernel, 1).
// A macro, not a body shared by two kernels: inlined from a function of its own, the same statements compile to other instructions (the workgroup size is then
// read the long way), and the kernels of the two earlier translation units are to stay what they are
#ifndef BAMD_B32_MV_KERNEL
#define BAMD_B32_MV_KERNEL matvec_b32_kernel
#define BAMD_B32_MV_NL 0
#endif
// MIN: the family of the launch
template <bool MIN, int PRO, int EPI>
__global__ void __launch_bounds__(512) BAMD_B32_MV_KERNEL(bamd_mv_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool NORM = PRO == BAMD_PRO_NORM;
    const int nb = a.K >> 8;
    const B32Lds L = carve_lds_b32(a, smem);
    const int wave = wave_id(), nwaves = blockDim.x >> 6;
    const int slot = blockIdx.x + gridDim.x * wave;          // consecutive row-groups land on different CUs
    const int stride = gridDim.x * nwaves;
    unsigned long long best = 0ull;
    constexpr bool PAIR = EPI == BAMD_EPI_SILU_MUL;
    bool pro_done = false;
    int off = 0;
    const int nseg = PAIR ? 1 : a.nseg;
    for (int s = 0; s < nseg; ++s) {
        const int nrg = a.seg[s].nrows >> 3;
        const int k0 = off <= slot ? 0 : (off - slot + stride - 1) / stride;
        const int g0 = slot + k0 * stride;
        const int count = g0 < off + nrg ? (off + nrg - 1 - g0) / stride + 1 : 0;
        if (count > 0) {
            const int t = a.seg[s].type;
            const uint8_t * wA = (const uint8_t *) a.seg[s].w;
            const uint8_t * wB = PAIR ? (const uint8_t *) a.seg[1].w : wA;
            const int nv = a.seg[s].nvalid > 0 ? a.seg[s].nvalid : a.seg[s].nrows;
#define BAMD_B32_SEG(TYPE_) b32_stream_depth<TYPE_, EPI, NORM>(wA, wB, nb, g0 - off, count, stride, a.seg[s].out, a.res, a, L, !pro_done, best, nv)
            if constexpr (MIN) {
                if (t == BAMD_Q4_1)      BAMD_B32_SEG(BAMD_Q4_1);
                else if (t == BAMD_Q5_1) BAMD_B32_SEG(BAMD_Q5_1);
                else __builtin_trap();                       // unreachable: bamd_launch_matvec_b32 refuses any other type on the host
            } else {
                if (t == BAMD_Q8_0)      BAMD_B32_SEG(BAMD_Q8_0);
                else if (t == BAMD_Q4_0) BAMD_B32_SEG(BAMD_Q4_0);
                else if (t == BAMD_Q5_0) BAMD_B32_SEG(BAMD_Q5_0);
                else if constexpr (BAMD_B32_MV_NL != 0) { if (t == BAMD_IQ4_NL) BAMD_B32_SEG(BAMD_IQ4_NL); else __builtin_trap(); }
                else __builtin_trap();
            }
#undef BAMD_B32_SEG
            pro_done = true;
        }
        off += nrg;
    }
    if (!pro_done) { ActProQ0<NORM> ap; ap.issue(a.x, a.normw, a.K, wave); ap.template finish_q0<MIN>(a.x, a.normw, a.eps, a.K, L.q8, L.ys, L.red); }   // idle waves still owe the block its barriers
    if (EPI == BAMD_EPI_ARGMAX) {
        for (int o = 32; o; o >>= 1) { const unsigned long long ob = __shfl_xor(best, o); best = ob > best ? ob : best; }
        __syncthreads();
        unsigned long long * wb = (unsigned long long *) smem;
        if ((threadIdx.x & 63) == 0) wb[wave] = best;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long b = 0ull;
            for (int w = 0; w < nwaves; ++w) b = wb[w] > b ? wb[w] : b;
            if (b) atomicMax(a.best_key, b);
        }
    }
}

// ---- MODE B: split-K, one 8-wave workgroup per row-group (the types without a minimum only) -------------------------------------------------------
// Wave w streams the records [i0, i0 + n_w) of the row-group (the shares of split_stream's UNEVEN form: the first nb % 8 waves take one more) and PARKS their
// terms in LDS; behind a workgroup barrier ONE wave runs the chain of all K / 32 blocks in block order.  A partial sum per wave would change the bits: the
// chain of an output is serial.  A parked record is 2304 bytes: f[c][lane] (8 x 64 floats) + s[r][c] (8 x 8 floats, the scale product is the same in a row's
// eight lanes).  Two term buffers where they fit the LDS (K <= 8192: the chain of row-group n overlaps the streaming of n + 1, and the chain moves from
// wave to wave), else one buffer and a second barrier.
constexpr int q0_term_floats = b32_term_floats(false);
constexpr int q0_split_nbuf(int nb) { return mv_terms_off(nb) + 2 * (size_t) nb * q0_term_floats * 4 <= (size_t) BAMD_LDS_CU_BYTES ? 2 : 1; }
constexpr size_t q0_split_lds(int nb) { return mv_terms_off(nb) + (size_t) q0_split_nbuf(nb) * nb * q0_term_floats * 4; }
constexpr bool q0_can_split(int nb) { return nb >= 8 && nb <= 56; }                     // at most 7 records per wave in registers
#define BAMD_Q0_NBW 7
template <int TYPE, int EPI, bool NORM>
__device__ __forceinline__ void q0_split(const uint8_t * __restrict__ w, int nb, int first, int count, int stride, float * __restrict__ out, const float * __restrict__ res,
                                         const bamd_mv_args & a, const B32Lds & L, bool do_pro, float * terms, int & ctr, int nvalid) {
    constexpr int RECB = BAMD_RECB_OF(TYPE);
    const int lane = threadIdx.x & 63, wave = wave_id(), r8 = lane >> 3;
    const bamd_rsrc rs = weight_rsrc(w);
    const int rem = nb & 7, nbw = (nb + 7) >> 3;
    const int n_w = rem ? (nbw - 1) + (wave < rem ? 1 : 0) : nbw;
    const int i0 = rem ? wave * (nbw - 1) + (wave < rem ? wave : rem) : wave * nbw;
    const int nbuf = q0_split_nbuf(nb);
    const int rgb = nb * RECB;
    ActProQ0<NORM> ap;
    if (do_pro) ap.issue(a.x, a.normw, a.K, wave);
    RecB32<TYPE> ring[BAMD_Q0_NBW];
#pragma unroll
    for (int j = 0; j < BAMD_Q0_NBW; ++j) if (j < n_w) load_rec(ring[j], rs, first * rgb + (i0 + j) * RECB, lane);
    if (do_pro) ap.finish_q0(a.x, a.normw, a.eps, a.K, L.q8, L.ys, L.red);
    for (int r = 0; r < count; ++r) {
        const int rg = first + r * stride;
        float * B = terms + (nbuf == 2 ? (size_t) (ctr & 1) * nb * q0_term_floats : (size_t) 0);
        const int cw = nbuf == 2 ? (ctr & 7) : 0;            // the wave that runs this row-group's chain
        const int crow = rg * 8 + r8;
        float resv = 0.f;
        if (EPI == BAMD_EPI_ADD && wave == cw && crow < nvalid) resv = ik_ld(res + crow);
#pragma unroll
        for (int j = 0; j < BAMD_Q0_NBW; ++j) {
            if (j < n_w) {                                   // wave-uniform
                const int ci = i0 + j;
                pin_rec(ring[j]);
                float sc[8], fd[8];
                b32_terms(ring[j], ci, lane, L.q8, L.ys, sc, fd);
                float * P = B + (size_t) ci * q0_term_floats;
#pragma unroll
                for (int c = 0; c < 8; ++c) P[c * 64 + lane] = fd[c];
                if ((lane & 7) == 0) {
                    *(float4 *) (P + 512 + r8 * 8) = make_float4(sc[0], sc[1], sc[2], sc[3]);
                    *(float4 *) (P + 512 + r8 * 8 + 4) = make_float4(sc[4], sc[5], sc[6], sc[7]);
                }
                if (r + 1 < count) load_rec(ring[j], rs, (rg + stride) * rgb + ci * RECB, lane);      // workgroup-uniform condition
            }
        }
        __syncthreads();
        if (wave == cw) {
            float acc = 0.f;
            for (int ib = 0; ib < nb; ++ib) {
                const float * P = B + (size_t) ib * q0_term_floats;
                const float4 s0 = *(const float4 *) (P + 512 + r8 * 8), s1 = *(const float4 *) (P + 512 + r8 * 8 + 4);
                const float sc[8] = { s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w };
                float fd[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) fd[c] = P[c * 64 + lane];
                b32_chain8(acc, sc, fd);
            }
            const float val = b32_finish_row(acc);
            if ((lane & 7) == 0 && crow < nvalid) ik_st(out + crow, EPI == BAMD_EPI_ADD ? val + resv : val);
        }
        ctr += 1;
        if (nbuf == 1) __syncthreads();                      // one buffer: the chain must be done before the next row-group parks
    }
}

template <int PRO, int EPI>
__global__ void __launch_bounds__(512) matvec_q0_split_kernel(bamd_mv_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool NORM = PRO == BAMD_PRO_NORM;
    const int nb = a.K >> 8;
    const B32Lds L = carve_lds_b32(a, smem);
    float * terms = (float *) (smem + mv_terms_off(nb));
    int ctr = 0;
    bool pro_done = false;
    int off = 0;
    const int slot = blockIdx.x, stride = gridDim.x;         // row-groups are dealt to workgroups
    for (int s = 0; s < a.nseg; ++s) {
        const int nrg = a.seg[s].nrows >> 3;
        const int k0 = off <= slot ? 0 : (off - slot + stride - 1) / stride;
        const int g0 = slot + k0 * stride;
        const int count = g0 < off + nrg ? (off + nrg - 1 - g0) / stride + 1 : 0;
        if (count > 0) {
            const int t = a.seg[s].type;
            const uint8_t * w = (const uint8_t *) a.seg[s].w;
            const int nv = a.seg[s].nvalid > 0 ? a.seg[s].nvalid : a.seg[s].nrows;
            if (t == BAMD_Q8_0)      q0_split<BAMD_Q8_0, EPI, NORM>(w, nb, g0 - off, count, stride, a.seg[s].out, a.res, a, L, !pro_done, terms, ctr, nv);
            else if (t == BAMD_Q4_0) q0_split<BAMD_Q4_0, EPI, NORM>(w, nb, g0 - off, count, stride, a.seg[s].out, a.res, a, L, !pro_done, terms, ctr, nv);
            else if (t == BAMD_Q5_0) q0_split<BAMD_Q5_0, EPI, NORM>(w, nb, g0 - off, count, stride, a.seg[s].out, a.res, a, L, !pro_done, terms, ctr, nv);
            else __builtin_trap();
            pro_done = true;
        }
        off += nrg;
    }
    if (!pro_done) { ActProQ0<NORM> ap; ap.issue(a.x, a.normw, a.K, wave_id()); ap.finish_q0(a.x, a.normw, a.eps, a.K, L.q8, L.ys, L.red); }
}

// test entry: standard block_q8_0 bytes {f16 d, i8 qs[32]} (34 per block) or, Q1, block_q8_1 bytes {f16 d, f16 s, i8 qs[32]} (36 per block) out of the prologue
// (parity with quantize_row_q8_0 / quantize_row_q8_1)
template <bool Q1>
__global__ void __launch_bounds__(512) quantize_q8_test_kernel(const float * x, const float * nw, float eps, int K, int norm, uint8_t * out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int BLK = Q1 ? 36 : 34, QS = Q1 ? 4 : 2;
    const int nb = K >> 8;
    uint32_t * q8 = (uint32_t *) smem; float * ys = (float *) (q8 + nb * 64);
    double * red = (double *) (smem + BAMD_ACT_RED_OFF(nb));
    if (norm) { ActProQ0<true> ap; ap.issue(x, nw, K, wave_id()); ap.template finish_q0<Q1>(x, nw, eps, K, q8, ys, red); }
    else { ActProQ0<false> ap; ap.issue(x, nw, K, wave_id()); ap.template finish_q0<Q1>(x, nw, eps, K, q8, ys, red); }
    for (int i = threadIdx.x; i < nb * 64; i += blockDim.x) {
        const int blk = i >> 6, e = (i >> 3) & 7, c = i & 7;
        const uint32_t w = q8[i];
        uint8_t * o = out + ((size_t) blk * 8 + c) * BLK;
        for (int t = 0; t < 4; ++t) o[QS + 4 * e + t] = (uint8_t) (w >> (8 * t));
    }
    for (int i = threadIdx.x; i < nb * 8; i += blockDim.x) {
        if (Q1) {
            const uint32_t ds = ((const uint32_t *) ys)[i];  // {f16 d, f16 s} as the block holds them
            for (int t = 0; t < 4; ++t) out[(size_t) i * BLK + t] = (uint8_t) (ds >> (8 * t));
        } else {
            const unsigned short h = f2h(ys[i]);             // exact: ys holds a widened f16
            out[(size_t) i * BLK] = (uint8_t) (h & 0xff); out[(size_t) i * BLK + 1] = (uint8_t) (h >> 8);
        }
    }
}

// ===========================================================================================================
// launchers, instantiated once per type list by the three .hip files
// ===========================================================================================================
template <bool Q1> void launch_quantize_q8_test(const float * x, const float * nw, float eps, int K, int norm, void * out, hipStream_t s) {
    BAMD_LAUNCH(quantize_q8_test_kernel<Q1>, dim3(1), dim3(512), act_lds_bytes(K), s, x, nw, eps, K, norm, (uint8_t *) out);
}

// every segment of the type list FAM (1 = a segment of another list, or of none).  Mode A for every shape; split-K only on request (mode 2) and only
// for Q8_0 / Q4_0 / Q5_0: why, and what was measured, is in DESIGN.md section 3.  2 = split-K was asked for (mode 2) for Q4_1 / Q5_1 or in a launch with IQ4_NL, which have none
template <int FAM> int launch_matvec_b32(const bamd_mv_args & a, int pro, int epi, int n_cu, hipStream_t s) {
    static_assert((FAM == B32_FAM_NL) == (BAMD_B32_MV_NL != 0), "the IQ4_NL type list is launched from the translation unit whose kernel has it");
    constexpr bool MIN = FAM == B32_FAM_Q1;
    for (int i = 0; i < a.nseg; ++i) if (!(MIN ? bamd_is_q1(a.seg[i].type) : FAM == B32_FAM_NL ? bamd_takes_q8_0(a.seg[i].type) : bamd_is_q0(a.seg[i].type))) return 1;
    if (FAM != B32_FAM_Q0 && (a.mode & 15) == 2) return 2;
    int nrg = 0;
    if (epi == BAMD_EPI_SILU_MUL) nrg = a.seg[0].nrows >> 3;
    else for (int i = 0; i < a.nseg; ++i) nrg += a.seg[i].nrows >> 3;
    const int cus = n_cu > 0 ? n_cu : 256;
    const int grid = nrg < 1 ? 1 : nrg < cus ? nrg : cus;
    typedef consts<BAMD_PRO_NORM, BAMD_PRO_PLAIN> pros;
    if constexpr (FAM == B32_FAM_Q0) {
        const int nb = a.K >> 8;
        const bool can_split = (epi == BAMD_EPI_STORE || epi == BAMD_EPI_ADD) && q0_can_split(nb);
        const bool split = (a.mode & 15) == 2 && can_split;      // mode 2: split-K where the shape has it
        if (split) return with_const(pros(), pro, [&](auto P) -> bool { return with_const(consts<BAMD_EPI_ADD, BAMD_EPI_STORE>(), epi, [&](auto E) -> bool {
            BAMD_LAUNCH((matvec_q0_split_kernel<decltype(P)::value, decltype(E)::value>), dim3(grid), dim3(512), q0_split_lds(nb), s, a); return true; }); }) ? 0 : 1;
    }
    return with_const(pros(), pro, [&](auto P) -> bool { return with_const(consts<BAMD_EPI_STORE, BAMD_EPI_ADD, BAMD_EPI_SILU_MUL, BAMD_EPI_ARGMAX>(), epi, [&](auto E) -> bool {
        BAMD_LAUNCH((BAMD_B32_MV_KERNEL<MIN, decltype(P)::value, decltype(E)::value>), dim3(grid), dim3(512), act_lds_bytes(a.K), s, a); return true; }); }) ? 0 : 1;
}
