// bamd_prefill_b32.h — the integer-dot batched prompt mat-mul of the 32-weight block formats (what it computes: bamd_prefill_b32.hip; numerics, records and the
// chains: bamd_b32_device.h).  ONE source, TWO translation units: bamd_prefill_b32.hip instantiates the kernels of the two families, bamd_prefill_b32_nl.hip the
// kernel whose type list is Q8_0 / Q4_0 / Q5_0 AND IQ4_NL, for the launches with at least one IQ4_NL segment; every other launch goes where it went before.
#pragma once
#include "bamd_b32_device.h"
#include "bamd_prefill_valu.h"

// the row policy of a 32-weight block type: b32_terms and the chains of bamd_b32_device.h over the image q8 | ys.  Accumulators: acc, acc2 (the odd blocks' of a
// type with two, b32_two_acc) and summs (with a minimum); temporaries: the eight scale products, dots and minimum terms of a record.  Behind a wave's last chunk:
// the zero-record descriptor
template <int TYPE> struct B32Row {
    typedef RecB32<TYPE> Rec;
    typedef float Acc;
    typedef float Work[8];
    static constexpr int RECB = BAMD_RECB_OF(TYPE);
    static constexpr bool NULL_TAIL = true;
    static constexpr bool MIN = b32_has_min(TYPE);
    static __device__ __forceinline__ void zero(float & acc, float & acc2, float & summs) { acc = 0.f; acc2 = 0.f; summs = 0.f; }
    static __device__ __forceinline__ void step(const Rec & R, int ci, int lane, const unsigned char * au, int nb, float & acc, float & acc2, float & summs,
                                                float (&sc)[8], float (&fd)[8], float (&ms)[8]) {
        const uint32_t * q8 = (const uint32_t *) au; const float * ys = (const float *) (q8 + nb * 64);
        b32_terms(R, ci, lane, q8, ys, sc, fd, ms);
        if constexpr (b32_two_acc(TYPE)) b32_chain8(acc, acc2, sc, fd);
        else b32_chain8(acc, sc, fd);
        if (MIN) b32_summs8(summs, ms);
    }
    static __device__ __forceinline__ float finish(const float & acc, const float & acc2, const float & summs) {
        return b32_finish_row<MIN>(b32_two_acc(TYPE) ? acc + acc2 : acc, summs);
    }
};

// The translation unit names its kernel and says whether the type list without a minimum holds IQ4_NL (bamd_prefill_b32_nl.hip: matmul_batch_b32_nl_kernel, 1): a
// macro for the reason bamd_matvec_b32.h gives for its own, so that the kernels of bamd_prefill_b32.hip stay what they are
#ifndef BAMD_B32_MM_KERNEL
#define BAMD_B32_MM_KERNEL matmul_batch_b32_kernel
#define BAMD_B32_MM_NL 0
#endif
// the type list of a kernel (BAMD_VALU_MM_KERNEL_BODY).  MIN: the family of the launch.
// Ring depth 2 where the record count is even — but, with a minimum, not in the gate/up instance at 8 tokens, whose gate values leave no room for a second record
// (with it the compiler spills: 8 bytes of scratch per lane), and not at 8 tokens in the kernel that has IQ4_NL, whose second accumulator per token leaves none
// either (64 to 144 bytes of scratch per lane with it)
#define BAMD_B32_TYPES_D(SEG, D) do { \
    if constexpr (MIN) { \
        if (t == BAMD_Q4_1)      SEG(D, B32Row<BAMD_Q4_1>); \
        else if (t == BAMD_Q5_1) SEG(D, B32Row<BAMD_Q5_1>); \
        else __builtin_trap();                   /* the launcher checks the types: never a silent read as another format */ \
    } else { \
        if (t == BAMD_Q8_0)      SEG(D, B32Row<BAMD_Q8_0>); \
        else if (t == BAMD_Q4_0) SEG(D, B32Row<BAMD_Q4_0>); \
        else if (t == BAMD_Q5_0) SEG(D, B32Row<BAMD_Q5_0>); \
        else if constexpr (BAMD_B32_MM_NL != 0) { if (t == BAMD_IQ4_NL) SEG(D, B32Row<BAMD_IQ4_NL>); else __builtin_trap(); } \
        else __builtin_trap(); \
    } } while (0)
#define BAMD_B32_TYPES(SEG) \
    if ((nb & 1) == 0 && !(MIN && PAIR && TT == 8) && !(BAMD_B32_MM_NL != 0 && TT == 8)) BAMD_B32_TYPES_D(SEG, 2); \
    else                                                                                BAMD_B32_TYPES_D(SEG, 1)
// grid and tile sizes: bamd_prefill_valu.h
template <bool MIN, int EPI, int TT>
__global__ void __launch_bounds__(512) BAMD_B32_MM_KERNEL(bamd_mm_args a) {
    BAMD_VALU_MM_KERNEL_BODY(BAMD_B32_TYPES)
}
// every segment of the family of segment 0 — without a minimum and in the translation unit whose kernel has it, IQ4_NL too; a.blob in that family's form
// (bamd_launch_quantize_batch_b32).  1 = shape not supported
// (a template for the sake of `if constexpr`: the translation unit of the IQ4_NL type list instantiates no kernel of the family with a minimum)
template <bool NL = (BAMD_B32_MM_NL != 0)> static int launch_matmul_batch_b32(const bamd_mm_args & a, int epi, int n_cu, hipStream_t s) {
    const bool has_min = a.nseg > 0 && bamd_is_q1(a.seg[0].type);
    if (NL && has_min) return 1;
    valu_mm_geom g;
    if (!valu_mm_geometry(a, epi, n_cu, g)) return 1;
    for (int i = 0; i < a.nseg; ++i) if (!(has_min ? bamd_is_q1(a.seg[i].type) : NL ? bamd_takes_q8_0(a.seg[i].type) : bamd_is_q0(a.seg[i].type))) return 1;
#define BAMD_MB32_(MIN_, EPI_) do { if (g.tt == BAMD_TT) hipLaunchKernelGGL((BAMD_B32_MM_KERNEL<MIN_, EPI_, BAMD_TT>), g.grid, dim3(512), g.lds, s, a); else hipLaunchKernelGGL((BAMD_B32_MM_KERNEL<MIN_, EPI_, 4>), g.grid, dim3(512), g.lds, s, a); } while (0)
#define BAMD_MB32(EPI_) do { if constexpr (!NL) { if (has_min) BAMD_MB32_(true, EPI_); else BAMD_MB32_(false, EPI_); } else BAMD_MB32_(false, EPI_); } while (0)
    switch (epi) {
        case BAMD_EPI_STORE:    BAMD_MB32(BAMD_EPI_STORE); break;
        case BAMD_EPI_ADD:      BAMD_MB32(BAMD_EPI_ADD); break;
        case BAMD_EPI_SILU_MUL: BAMD_MB32(BAMD_EPI_SILU_MUL); break;
        default: return 1;
    }
#undef BAMD_MB32
#undef BAMD_MB32_
    return 0;
}
