// bamd_flt_device.h — device code of the unquantised weight family, F32 / F16 / BF16 (bamd_matvec_flt.hip: decode mat-vec; bamd_prefill_flt.hip: batched prompt).
// Records: bamd_formats.h.
//
// What is restated (the reference build defines GGML_USE_LLAMAFILE):
//   F32 / F16 weights — ggml_compute_forward_mul_mat hands the mat-mul to llamafile_sgemm (ggml.c:12318-12343; src1 is contiguous f32, k % 8 == 0), which runs
//   tinyBLAS<8, __m256, ...>::gemm (sgemm.cpp:408-432): per output ONE 8-lane accumulator, lane j: acc = fmaf(w[8i + j], x[8i + j], acc) for i = 0 .. K/8 - 1
//   (_mm256_fmadd_ps: one rounding per step), F16 weights widened exactly, the activations stay f32; then hsum(__m256) (sgemm.cpp:163-183).  This is NOT
//   ggml_vec_dot_f16 (32 lanes, activations rounded to f16).  The chain of an output is the same for any number of tokens: the batched prompt gives the bits
//   of token by token.
//   BF16 weights — llamafile_sgemm has no case for them: the activations are rounded to bf16 (ggml_compute_fp32_to_bf16, ggml-impl.h:88-101: integer
//   round-to-nearest-even, NaN quieted, subnormals kept) and ggml_vec_dot_bf16's AVX2 branch runs (ggml.c:2007-2026): four 8-lane accumulators, lane j of
//   accumulator a takes k = 32i + 8a + j with add(mul(w, x), c); then (c1 + c3) + (c2 + c4) and the same 8 -> 1 tree.
//
// A lane of a wave is one lane of those accumulators: wave lane (r, j) = row r of the row-group, SIMD lane j for F32 / F16; wave lane (h, a, j) = row 2q + h of
// the row-group in request q, accumulator a, SIMD lane j for BF16.  The activation vector is kept in the order the lanes read it:
//   f32 form   element k = 8i + j at float (i >> 2) * 32 + j * 4 + (i & 3): lane j reads four steps of its chain as one float4
//   bf16 form  element k = 256b + 32i + c (c = 8a + j) at half 256b + 8c + i: chain lane c reads the eight steps of a record as one uint4
#pragma once
#include "bamd_device.h"
#include "bamd_bf16_range.h"

// ggml_compute_fp32_to_bf16 (ggml-impl.h:88-101), in integer arithmetic
__device__ __forceinline__ uint32_t flt_bf16_bits(float f) {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 64u;          // NaN: quieted
    return (u + (0x7fffu + ((u >> 16) & 1u))) >> 16;
}

// LDS of a mat-vec workgroup: the activation vector, 16 f64 reduction slots, 16 arg-max slots
constexpr size_t flt_lds_bytes(bool bf, int K) { return (size_t) K * (bf ? 2 : 4) + 16 * sizeof(double) + 16 * sizeof(unsigned long long); }

// Activation prologue of one workgroup: x[K] (inter-kernel data: sc1 loads) -> dst in the form's order, NORM: (x * scale) * nw first (ggml_vec_scale_f32 then
// ggml_mul, llama.cpp:7940-7950; the sum of squares in f64 with the order guard of bamd_device.h).  Ends with a workgroup barrier.
// rng (BF only; null: none): two LDS words the caller set to { BAMD_BF16_RANGE_NONE & 0xffff, 0 } in front of a barrier — behind the final barrier they hold the
// lowest and the highest exponent of the bf16 patterns stored (bamd_bf16_range.h: the guard of bamd_prefill2_bf16.hip)
template <bool NORM, bool BF>
__device__ __forceinline__ void flt_act(const float * __restrict__ x, const float * __restrict__ nw, float eps, int K, unsigned char * dst, double * red, uint32_t * rng = nullptr) {
    const int lane = threadIdx.x & 63, wave = wave_id(), nwaves = (int) (blockDim.x >> 6), n4 = K >> 2;
    const bamd_ik_rsrc rx = ik_rsrc(x);
    float scale = 1.0f;
    if (NORM) {
        double s = 0.0;                                                    // ggml.c:11874-11877
        for (int k4 = threadIdx.x; k4 < n4; k4 += blockDim.x) {
            const float4 v = ik_ld128f(rx, (uint32_t) k4 * 16u);
            s += (double) (v.x * v.x); s += (double) (v.y * v.y); s += (double) (v.z * v.z); s += (double) (v.w * v.w);
        }
        s = wave_sum_f64(s);
        if (lane == 0) red[wave] = s;
        __syncthreads();
        double tot = 0.0;
        for (int w2 = 0; w2 < nwaves; ++w2) tot += red[w2];
        double md = tot / (double) K;                                      // ggml.c:11879
        float mean = (float) md;
        if (!f32_rounding_safe(md, BAMD_F64_GUARD_ULPS(K))) {              // workgroup-uniform, rare: the reference's order, one lane
            __syncthreads();
            if (threadIdx.x == 0) {
                double sq = 0.0;
                for (int i = 0; i < K; ++i) { const float xv = ik_ld(x + i); sq += (double) (xv * xv); }
                red[0] = sq;
            }
            __syncthreads();
            md = red[0] / (double) K;
            mean = (float) md;
        }
        scale = 1.0f / sqrtf(mean + eps);
    }
    uint32_t rlo = BAMD_BF16_RANGE_NONE & 0xffffu, rhi = 0u;
    for (int k4 = threadIdx.x; k4 < n4; k4 += blockDim.x) {
        float4 v = ik_ld128f(rx, (uint32_t) k4 * 16u);
        if (NORM) {
            const float4 w = *(const float4 *) (nw + 4 * k4);
            v.x = (v.x * scale) * w.x; v.y = (v.y * scale) * w.y; v.z = (v.z * scale) * w.z; v.w = (v.w * scale) * w.w;
        }
        const int k = k4 << 2;                                             // k .. k + 3: one chain step i, four neighbouring lanes
        if (BF) {
            unsigned short * d = (unsigned short *) dst + ((k >> 8) << 8) + ((k >> 5) & 7) + ((k & 31) << 3);
            d[0] = (unsigned short) flt_bf16_bits(v.x); d[8] = (unsigned short) flt_bf16_bits(v.y);
            d[16] = (unsigned short) flt_bf16_bits(v.z); d[24] = (unsigned short) flt_bf16_bits(v.w);
            if (rng) {                                                         // (the bits just stored)
                bamd_bf16_range_add(rlo, rhi, flt_bf16_bits(v.x)); bamd_bf16_range_add(rlo, rhi, flt_bf16_bits(v.y));
                bamd_bf16_range_add(rlo, rhi, flt_bf16_bits(v.z)); bamd_bf16_range_add(rlo, rhi, flt_bf16_bits(v.w));
            }
        } else {
            const int i = k >> 3;
            float * d = (float *) dst + ((i >> 2) << 5) + ((k & 7) << 2) + (i & 3);
            d[0] = v.x; d[4] = v.y; d[8] = v.z; d[12] = v.w;
        }
    }
    if (BF && rng) {
        for (int o = 32; o; o >>= 1) { const uint32_t l2 = __shfl_xor(rlo, o), h2 = __shfl_xor(rhi, o); rlo = l2 < rlo ? l2 : rlo; rhi = h2 > rhi ? h2 : rhi; }
        if (lane == 0) { atomicMin(rng, rlo); atomicMax(rng + 1, rhi); }
    }
    __syncthreads();
}

// ---- a chunk: four 16-byte requests per lane = 4 KiB of a row-group (F16 / BF16: a record, 256 weights per row; F32: half a record, 128) ----
#define BAMD_FLT_CHB 4096
#define BAMD_FLT_CHUNK_K(WT_) ((WT_) == BAMD_F32 ? 128 : 256)
struct FltChunk { uint4 q[4]; };
__device__ __forceinline__ void flt_load(FltChunk & C, bamd_rsrc rs, int soff, int lane) {
#pragma unroll
    for (int q = 0; q < 4; ++q) C.q[q] = bl128(rs, (uint32_t) lane * 16u, soff + q * 1024);
}
__device__ __forceinline__ float bf2f_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf2f_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }

// F32 / F16: one chain step per weight, in the order of i.  X: the chunk's activations of this lane, float4 g = steps 4g .. 4g + 3 (stride XS float4 between them)
template <int WT, int XS, typename XP>
__device__ __forceinline__ float flt_chain(float acc, const FltChunk & C, XP X) {
    if constexpr (WT == BAMD_F32) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 a = X[q * XS];
            acc = fmaf(__uint_as_float(C.q[q].x), a.x, acc); acc = fmaf(__uint_as_float(C.q[q].y), a.y, acc);
            acc = fmaf(__uint_as_float(C.q[q].z), a.z, acc); acc = fmaf(__uint_as_float(C.q[q].w), a.w, acc);
        }
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 a = X[(2 * q) * XS], b = X[(2 * q + 1) * XS];
            acc = fmaf(h2f(C.q[q].x & 0xffffu), a.x, acc); acc = fmaf(h2f(C.q[q].x >> 16), a.y, acc);
            acc = fmaf(h2f(C.q[q].y & 0xffffu), a.z, acc); acc = fmaf(h2f(C.q[q].y >> 16), a.w, acc);
            acc = fmaf(h2f(C.q[q].z & 0xffffu), b.x, acc); acc = fmaf(h2f(C.q[q].z >> 16), b.y, acc);
            acc = fmaf(h2f(C.q[q].w & 0xffffu), b.z, acc); acc = fmaf(h2f(C.q[q].w >> 16), b.w, acc);
        }
    }
    return acc;
}
// BF16: request q is row 2q + h; xa = the eight bf16 activations of this chain lane.  add(mul(w, x), c), two roundings: the recorded reference answers
// (tests/golden/float_kats.npz: products below 2^-126) are those of the separate multiply and add, not of an fma
__device__ __forceinline__ float bf_step(float acc, float w, float x) { return __fadd_rn(__fmul_rn(w, x), acc); }
__device__ __forceinline__ void flt_chain_bf(float (&acc)[4], const FltChunk & C, const uint4 xa) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float s = acc[q];
        s = bf_step(s, bf2f_lo(C.q[q].x), bf2f_lo(xa.x)); s = bf_step(s, bf2f_hi(C.q[q].x), bf2f_hi(xa.x));
        s = bf_step(s, bf2f_lo(C.q[q].y), bf2f_lo(xa.y)); s = bf_step(s, bf2f_hi(C.q[q].y), bf2f_hi(xa.y));
        s = bf_step(s, bf2f_lo(C.q[q].z), bf2f_lo(xa.z)); s = bf_step(s, bf2f_hi(C.q[q].z), bf2f_hi(xa.z));
        s = bf_step(s, bf2f_lo(C.q[q].w), bf2f_lo(xa.w)); s = bf_step(s, bf2f_hi(C.q[q].w), bf2f_hi(xa.w));
        acc[q] = s;
    }
}
// (c1 + c3) + (c2 + c4) across the four accumulators of a row (wave lanes 16 and 8 apart), then the 8 -> 1 tree: the row's value in its lane (a, j) = (0, 0)
__device__ __forceinline__ float flt_finish_bf(float v) {
    v = v + __shfl_xor(v, 16);
    v = v + __shfl_xor(v, 8);
    return hsum8_tinyblas(v);
}
