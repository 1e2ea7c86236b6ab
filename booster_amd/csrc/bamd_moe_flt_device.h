// bamd_moe_flt_device.h — device code of unquantised EXPERT matrices, F16 / F32 / BF16 (bamd_moe_flt.hip: the routed decode launches; bamd_moe_batch_flt.hip: the
// grouped prompt mat-muls).  The dense family's code (bamd_flt_device.h) does not fit them: the reference computes an expert row differently.
//
// What is restated: ggml_compute_forward_mul_mat_id (ggml.c:12494) never calls llamafile_sgemm.  It converts the activation row with from_float of the type's
// vec_dot_type and calls the type's vec_dot, one row at a time:
//   F16   activations rounded to f16 (ggml_fp32_to_fp16_row, F16C: round to nearest even, overflow to inf, subnormals kept); ggml_vec_dot_f16 (ggml.c:2038):
//         four 8-lane f32 accumulators, lane j of accumulator a takes k = 32i + 8a + j with ONE fma per step, both operands widened exactly
//   F32   activations as they are; ggml_vec_dot_f32 (ggml.c:1931): the same 4 x 8 fma structure
//   BF16  ggml_vec_dot_bf16: the chain bamd_flt_device.h restates for the dense BF16 matrices (multiply and add rounded separately), bf16 activations
// The tail of F16 / F32 is GGML_F32x8_REDUCE: (s0 + s2) + (s1 + s3), then lo + hi halves, then two hadd_ps, i.e. (t0 + t1) + (t2 + t3) — hsum8_vecdot, NOT the
// (t0 + t2) + (t1 + t3) of the sgemm hsum that ggml_vec_dot_bf16's own tail shares (flt_finish_bf).  Recorded answers: tests/golden/moe_flt_kats.npz.
//
// So a row is a chain of 32 lanes for all three types: chain lane c = 8a + j (accumulator a = c >> 3, SIMD lane j = c & 7).  A wave lane is (h, c): row 2q + h of
// the row-group in request q of a chunk, chain lane c — the geometry of the dense BF16 record, which the F16 expert record shares byte for byte; the F32 expert
// record has the same rows and lanes at four weights per request (bamd_moe_flt.hip: the repack).
// A chunk is the dense family's: four 16-byte requests per lane = 4 KiB of a row-group = 256 weights of each of its 8 rows (F32: 128).
// The activation image, in the order the chain lanes read it — chain lane c reads the steps of a chunk as ONE uint4, uint4 number chunk * 32 + c for every form:
//   16-bit forms  element k = 256b + 32i + c at half  256b + 8c + i   (bamd_flt_device.h's bf16 form)
//   f32 form      element k = 128n + 32i + c at float 128n + 4c + i
#pragma once
#include "bamd_flt_device.h"

constexpr int xf_steps(int wt) { return wt == BAMD_F32 ? 4 : 8; }                     // chain steps of a lane per chunk
constexpr int xf_chunk_k(int wt) { return wt == BAMD_F32 ? 128 : 256; }                // weights of a row per chunk
constexpr size_t xf_image_bytes(int wt, int K) { return (size_t) K * (wt == BAMD_F32 ? 4 : 2); }

// ggml_fp32_to_fp16_row rounds an f32 that is already rounded.  Where the value is a product, the compiler folds multiply and conversion into v_fma_mixlo_f16, which
// rounds the exact product ONCE, to f16 — other bits wherever the f32 rounding moves the product across an f16 tie (seen on a whole model, 8 layers deep, not on
// the op tests' few thousand values).  The empty asm makes the f32 a value of its own in front of the conversion
__device__ __forceinline__ unsigned short xf_f16_bits(float v) { asm volatile("" : "+v"(v)); return f2h(v); }

// four neighbouring elements k .. k + 3 (one step i, chain lanes c .. c + 3) into an image
template <int WT>
__device__ __forceinline__ void xf_store4(unsigned char * img, int k, const float4 v) {
    if constexpr (WT == BAMD_F32) {
        float * d = (float *) img + ((k >> 7) << 7) + ((k >> 5) & 3) + ((k & 31) << 2);
        d[0] = v.x; d[4] = v.y; d[8] = v.z; d[12] = v.w;
    } else {
        unsigned short * d = (unsigned short *) img + ((k >> 8) << 8) + ((k >> 5) & 7) + ((k & 31) << 3);
        if constexpr (WT == BAMD_F16) { d[0] = xf_f16_bits(v.x); d[8] = xf_f16_bits(v.y); d[16] = xf_f16_bits(v.z); d[24] = xf_f16_bits(v.w); }
        else { d[0] = (unsigned short) flt_bf16_bits(v.x); d[8] = (unsigned short) flt_bf16_bits(v.y); d[16] = (unsigned short) flt_bf16_bits(v.z); d[24] = (unsigned short) flt_bf16_bits(v.w); }
    }
}

// Activation prologue of an eight-wave workgroup: x[K] (inter-kernel data) -> the image of form WT, NORM: (x * scale) * nw first — the arithmetic of flt_act
// (bamd_flt_device.h), sum of squares in f64 behind the order guard of bamd_device.h.  In two halves so that a kernel can put its other requests between them:
// issue() sends the loads of a thread's first two float4 (all of x up to K = 4096) and finish() does the arithmetic; beyond them x is read in finish(), twice.
// finish() ends with a workgroup barrier and holds two more (NORM); every thread of the workgroup calls it
template <int WT>
struct XfActPro {
    float4 v[2];
    __device__ __forceinline__ void issue(const float * __restrict__ x, int K) {
        const bamd_ik_rsrc rx = ik_rsrc(x);
        const int n4 = K >> 2;
#pragma unroll
        for (int t = 0; t < 2; ++t) { const int k4 = (int) threadIdx.x + t * 512; v[t] = ik_ld128f(rx, (uint32_t) (k4 < n4 ? k4 : n4 - 1) * 16u); }
    }
    template <bool NORM>
    __device__ __forceinline__ void finish(const float * __restrict__ x, const float * __restrict__ nw, float eps, int K, unsigned char * img, double * red) {
        const int lane = threadIdx.x & 63, wave = wave_id(), n4 = K >> 2;
        const bamd_ik_rsrc rx = ik_rsrc(x);
        float scale = 1.0f;
        if (NORM) {
            double s = 0.0;                                                    // ggml.c:11874-11877
#pragma unroll
            for (int t = 0; t < 2; ++t) if ((int) threadIdx.x + t * 512 < n4) {
                s += (double) (v[t].x * v[t].x); s += (double) (v[t].y * v[t].y); s += (double) (v[t].z * v[t].z); s += (double) (v[t].w * v[t].w);
            }
            for (int k4 = threadIdx.x + 1024; k4 < n4; k4 += 512) {
                const float4 u = ik_ld128f(rx, (uint32_t) k4 * 16u);
                s += (double) (u.x * u.x); s += (double) (u.y * u.y); s += (double) (u.z * u.z); s += (double) (u.w * u.w);
            }
            s = wave_sum_f64(s);
            if (lane == 0) red[wave] = s;
            __syncthreads();
            double tot = 0.0;
            for (int w2 = 0; w2 < 8; ++w2) tot += red[w2];
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
        auto put = [&](int k4, float4 u) {
            if (NORM) {
                const float4 w = *(const float4 *) (nw + 4 * k4);
                u.x = (u.x * scale) * w.x; u.y = (u.y * scale) * w.y; u.z = (u.z * scale) * w.z; u.w = (u.w * scale) * w.w;
            }
            xf_store4<WT>(img, k4 << 2, u);
        };
#pragma unroll
        for (int t = 0; t < 2; ++t) if ((int) threadIdx.x + t * 512 < n4) put((int) threadIdx.x + t * 512, v[t]);
        for (int k4 = threadIdx.x + 1024; k4 < n4; k4 += 512) put(k4, ik_ld128f(rx, (uint32_t) k4 * 16u));
        __syncthreads();
    }
};

// the words of one request, or of a lane's uint4 of the image, as the f32 operands of the chain steps i = 0 .. xf_steps - 1 (every widening is exact)
template <int WT>
__device__ __forceinline__ void xf_widen(float (&o)[xf_steps(WT)], const uint4 u) {
    if constexpr (WT == BAMD_F32) { o[0] = __uint_as_float(u.x); o[1] = __uint_as_float(u.y); o[2] = __uint_as_float(u.z); o[3] = __uint_as_float(u.w); }
    else if constexpr (WT == BAMD_F16) {
        o[0] = h2f(u.x & 0xffffu); o[1] = h2f(u.x >> 16); o[2] = h2f(u.y & 0xffffu); o[3] = h2f(u.y >> 16);
        o[4] = h2f(u.z & 0xffffu); o[5] = h2f(u.z >> 16); o[6] = h2f(u.w & 0xffffu); o[7] = h2f(u.w >> 16);
    } else {
        o[0] = bf2f_lo(u.x); o[1] = bf2f_hi(u.x); o[2] = bf2f_lo(u.y); o[3] = bf2f_hi(u.y);
        o[4] = bf2f_lo(u.z); o[5] = bf2f_hi(u.z); o[6] = bf2f_lo(u.w); o[7] = bf2f_hi(u.w);
    }
}
// a chunk against a lane's activations: request q is row 2q + h, acc[q] its accumulator lane (a, j).  F16 / F32: one fma per step (GGML_F16_VEC_FMA /
// GGML_F32_VEC_FMA are _mm256_fmadd_ps); BF16: bf_step, the statements of flt_chain_bf
template <int WT>
struct XfChunkW { float w[4][xf_steps(WT)]; };
template <int WT>
__device__ __forceinline__ void xf_widen_chunk(XfChunkW<WT> & W, const FltChunk & C) {
#pragma unroll
    for (int q = 0; q < 4; ++q) xf_widen<WT>(W.w[q], C.q[q]);
}
template <int WT>
__device__ __forceinline__ void xf_chain(float (&acc)[4], const XfChunkW<WT> & W, const float (&x)[xf_steps(WT)]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float s = acc[q];
#pragma unroll
        for (int i = 0; i < xf_steps(WT); ++i) s = WT == BAMD_BF16 ? bf_step(s, W.w[q][i], x[i]) : fmaf(W.w[q][i], x[i], s);
        acc[q] = s;
    }
}
// The tail across the 32 chain lanes of a row, in registers: accumulators 16 lanes apart (s0 + s2, s1 + s3: ds_swizzle, an exchange inside each half-wave), then 8
// apart (a rotation of the DPP row), then the 8 -> 1 tree of the type.  Every add has the reference's two operands, and an f32 add is commutative, so the exchanges
// give all lanes the same bits; the row's value is read from its chain lane 0
__device__ __forceinline__ float xf_xor16(float v) { return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x401f)); }      // bit-mask mode: and 0x1f, or 0, xor 0x10
__device__ __forceinline__ float xf_xor8(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xf, 0xf, false)); }   // row_ror:8
template <int WT>
__device__ __forceinline__ float xf_finish(float v) {
    if constexpr (WT == BAMD_BF16) return flt_finish_bf(v);
    v = v + xf_xor16(v);
    v = v + xf_xor8(v);
    return hsum8_vecdot(v);
}
