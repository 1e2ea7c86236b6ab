// bamd_prefill_b32.h — the integer-dot batched prompt mat-mul of the 32-weight block formats (what it computes: bamd_prefill_b32.hip; numerics, records and the
// chains: bamd_b32_device.h).  ONE source, TWO translation units: bamd_prefill_b32.hip instantiates the kernels of the two families, bamd_prefill_b32_nl.hip the
// kernel whose type list is Q8_0 / Q4_0 / Q5_0 AND IQ4_NL, for the launches with at least one IQ4_NL segment; every other launch goes where it went before.
#pragma once
#include "bamd_b32_device.h"

template <int TYPE, int D, int EPI, int TT>
__device__ __forceinline__ void batch_segment_b32(const uint8_t * __restrict__ wA, const uint8_t * __restrict__ wB, int nb, int first, int count, int stride,
                                                  float * __restrict__ out, const float * __restrict__ res, int ldo, int t0, int nt,
                                                  const unsigned char * acts, size_t bb, int nvalid) {
    constexpr int RECB = BAMD_RECB_OF(TYPE);
    constexpr bool MIN = b32_has_min(TYPE);
    constexpr bool PAIR = EPI == BAMD_EPI_SILU_MUL;
    constexpr int NPARTS = PAIR ? 2 : 1;
    const int lane = threadIdx.x & 63;
    const bamd_rsrc rsA = weight_rsrc(wA), rsB = PAIR ? weight_rsrc(wB) : rsA, rsN = null_rsrc(wA);
    const int rgb = nb * RECB, rg_step = stride * rgb;
    const int chunks = nb / D;
    RecB32<TYPE> ring[D];
#pragma unroll
    for (int s = 0; s < D; ++s) load_rec(ring[s], rsA, first * rgb + s * RECB, lane);
    for (int r = 0; r < count; ++r) {
        const int rg = first + r * stride;
        const int row = rg * 8 + (lane >> 3);
        const int rowoff = rg * rgb;
        float gate_val[TT];
#pragma unroll
        for (int part = 0; part < NPARTS; ++part) {
            const bool last = !(PAIR && part == 0) && r + 1 >= count;
            const bool after_b = PAIR && part == 0;
            const int after_off = (PAIR && part == 0) ? rowoff : rowoff + rg_step;
            float acc[TT], acc2[TT], summs[TT];              // (acc2: the odd blocks' accumulators of a type with two, b32_two_acc)
#pragma unroll
            for (int u = 0; u < TT; ++u) { acc[u] = 0.f; acc2[u] = 0.f; summs[u] = 0.f; }
            for (int c = 0; c < chunks; ++c) {
                const bool inrow = c + 1 < chunks;
                const bool tail = !inrow && last;                // behind the wave's last chunk: the zero-record descriptor
                const bamd_rsrc nrs = tail ? rsN : (inrow ? part == 1 : after_b) ? rsB : rsA;
                const int nxt = tail ? 0 : inrow ? rowoff + (c + 1) * (D * RECB) : after_off;
#pragma unroll
                for (int s = 0; s < D; ++s) {
                    pin_rec(ring[s]);
#pragma unroll
                    for (int u = 0; u < TT; ++u) {               // tokens beyond nt read the last token's copy and are never stored
                        const unsigned char * au = acts + (size_t) u * bb;
                        const uint32_t * q8 = (const uint32_t *) au; const float * ys = (const float *) (q8 + nb * 64);
                        float sc[8], fd[8], ms[8];
                        b32_terms(ring[s], c * D + s, lane, q8, ys, sc, fd, ms);
                        if constexpr (b32_two_acc(TYPE)) b32_chain8(acc[u], acc2[u], sc, fd);
                        else b32_chain8(acc[u], sc, fd);
                        if (MIN) b32_summs8(summs[u], ms);
                    }
                    load_rec(ring[s], nrs, nxt + s * RECB, lane);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
#pragma unroll
            for (int u = 0; u < TT; ++u) {
                const float val = b32_finish_row<MIN>(b32_two_acc(TYPE) ? acc[u] + acc2[u] : acc[u], summs[u]);
                if (PAIR && part == 0) { gate_val[u] = val; continue; }
                if ((lane & 7) == 0 && row < nvalid && u < nt) {
                    const size_t o = (size_t) (t0 + u) * ldo + row;
                    float y = val;
                    if (PAIR) y = v_silu(gate_val[u]) * val;
                    if (EPI == BAMD_EPI_ADD) y = val + res[o];
                    out[o] = y;
                }
            }
        }
    }
}

// The translation unit names its kernel and says whether the type list without a minimum holds IQ4_NL (bamd_prefill_b32_nl.hip: matmul_batch_b32_nl_kernel, 1): a
// macro for the reason bamd_matvec_b32.h gives for its own, so that the kernels of bamd_prefill_b32.hip stay what they are
#ifndef BAMD_B32_MM_KERNEL
#define BAMD_B32_MM_KERNEL matmul_batch_b32_kernel
#define BAMD_B32_MM_NL 0
#endif
// grid (token tiles, row slots) and the tile sizes of matmul_batch_kernel: the blob has its stride, so TT tokens take the same LDS.  MIN: the family of the launch
template <bool MIN, int EPI, int TT>
__global__ void __launch_bounds__(512) BAMD_B32_MM_KERNEL(bamd_mm_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nb = a.K >> 8;
    const size_t bb = BAMD_BLOB_BYTES(nb);
    const int t0 = blockIdx.x * TT;
    const int nt = a.T - t0 < TT ? a.T - t0 : TT;
    {   // this tile's activations -> LDS (rows past T: repeat the last token; results discarded)
        const int n16 = (int) (bb / 16);
        for (int i = threadIdx.x; i < n16 * TT; i += blockDim.x) {
            const int u = i / n16, k = i - u * n16;
            const int tu = t0 + (u < nt ? u : nt - 1);
            ((uint4 *) smem)[(size_t) u * n16 + k] = ((const uint4 *) (a.blob + (size_t) tu * bb))[k];
        }
    }
    __syncthreads();
    const int wave = wave_id(), nwaves = blockDim.x >> 6;
    const int slot = blockIdx.y + gridDim.y * wave, stride = gridDim.y * nwaves;
    constexpr bool PAIR = EPI == BAMD_EPI_SILU_MUL;
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
            // ring depth 2 where the record count is even — but, with a minimum, not in the gate/up instance at 8 tokens, whose gate values leave no room for a
            // second record (with it the compiler spills: 8 bytes of scratch per lane), and not at 8 tokens in the kernel that has IQ4_NL, whose second accumulator
            // per token leaves none either (64 to 144 bytes of scratch per lane with it)
#define BAMD_B32_SEG(TYPE_, D_) batch_segment_b32<TYPE_, D_, EPI, TT>(wA, wB, nb, g0 - off, count, stride, a.seg[s].out, a.res, a.ldo, t0, nt, smem, bb, nv)
#define BAMD_B32_TYPES(D_) do { \
                if constexpr (MIN) { \
                    if (t == BAMD_Q4_1)      BAMD_B32_SEG(BAMD_Q4_1, D_); \
                    else if (t == BAMD_Q5_1) BAMD_B32_SEG(BAMD_Q5_1, D_); \
                    else __builtin_trap();                   /* the launcher checks the types: never a silent read as another format */ \
                } else { \
                    if (t == BAMD_Q8_0)      BAMD_B32_SEG(BAMD_Q8_0, D_); \
                    else if (t == BAMD_Q4_0) BAMD_B32_SEG(BAMD_Q4_0, D_); \
                    else if (t == BAMD_Q5_0) BAMD_B32_SEG(BAMD_Q5_0, D_); \
                    else if constexpr (BAMD_B32_MM_NL != 0) { if (t == BAMD_IQ4_NL) BAMD_B32_SEG(BAMD_IQ4_NL, D_); else __builtin_trap(); } \
                    else __builtin_trap(); \
                } } while (0)
            if ((nb & 1) == 0 && !(MIN && PAIR && TT == 8) && !(BAMD_B32_MM_NL != 0 && TT == 8)) BAMD_B32_TYPES(2);
            else                                            BAMD_B32_TYPES(1);
#undef BAMD_B32_TYPES
#undef BAMD_B32_SEG
        }
        off += nrg;
    }
}
// every segment of the family of segment 0 — without a minimum and in the translation unit whose kernel has it, IQ4_NL too; a.blob in that family's form
// (bamd_launch_quantize_batch_b32).  1 = shape not supported
// (a template for the sake of `if constexpr`: the translation unit of the IQ4_NL type list instantiates no kernel of the family with a minimum)
template <bool NL = (BAMD_B32_MM_NL != 0)> static int launch_matmul_batch_b32(const bamd_mm_args & a, int epi, int n_cu, hipStream_t s) {
    const bool has_min = a.nseg > 0 && bamd_is_q1(a.seg[0].type);
    if (NL && has_min) return 1;
    int nrg = 0;
    if (epi == BAMD_EPI_SILU_MUL) nrg = a.seg[0].nrows >> 3; else for (int i = 0; i < a.nseg; ++i) nrg += a.seg[i].nrows >> 3;
    const int tt = (size_t) BAMD_TT * BAMD_BLOB_BYTES(a.K >> 8) <= 160 * 1024 ? BAMD_TT : 4;
    const size_t lds = (size_t) tt * BAMD_BLOB_BYTES(a.K >> 8);
    if (lds > 160 * 1024) return 1;
    for (int i = 0; i < a.nseg; ++i) if (!(has_min ? bamd_is_q1(a.seg[i].type) : NL ? bamd_takes_q8_0(a.seg[i].type) : bamd_is_q0(a.seg[i].type))) return 1;
    const int tiles = (a.T + tt - 1) / tt;
    int gy = (4 * (n_cu > 0 ? n_cu : 256) + tiles - 1) / tiles;
    if (gy * 8 > nrg) gy = (nrg + 7) / 8;
    if (gy < 1) gy = 1;
    dim3 grid(tiles, gy);
#define BAMD_MB32_(MIN_, EPI_) do { if (tt == BAMD_TT) hipLaunchKernelGGL((BAMD_B32_MM_KERNEL<MIN_, EPI_, BAMD_TT>), grid, dim3(512), lds, s, a); else hipLaunchKernelGGL((BAMD_B32_MM_KERNEL<MIN_, EPI_, 4>), grid, dim3(512), lds, s, a); } while (0)
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
