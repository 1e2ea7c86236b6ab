// bamd_q1_device.h — device code shared by the kernels of the 32-weight block formats with a minimum, Q4_1 / Q5_1 (bamd_matvec_q1.hip: single-token mat-vec;
// bamd_prefill_q1.hip: batched prompt mat-mul on the integer-dot kernel; the matrix-core one, bamd_prefill2_q1.hip, restates the chains for its own lane layout): the wave-stream records (layout: bamd_formats.h), their block terms and the two chains.  The Q8_1 activation
// prologue is ActProQ0's with Q1 = true (bamd_q0_device.h): the Q8_0 image, with the block's {f16 d, f16 s} pair in the 4-byte slot that holds d widened there.
//
// NUMERICS (contract: bamd_device.h).  Reference functions restated here (cpp/ = the reference tree):
//   quantize_row_q8_1 (AVX2)         ggml/src/ggml-quants.c:1272-1333     d, id and the bytes are quantize_row_q8_0's; s = f16(d_f32 * (float) sum of the quants)
//   ggml_vec_dot_q4_1_q8_1 (AVX2)    ggml/src/ggml-quants.c:4344-4377     (llamafile_sgemm has no case for these types: one token and many go through vec_dot)
//   ggml_vec_dot_q5_1_q8_1 (AVX2)    ggml/src/ggml-quants.c:5009-5034
// One output = TWO accumulators over the 32-blocks l = 0 .. K/32 - 1 in order:
//   the 8-lane chain of the Q8_0 family: lane e: acc_e = fma(f32(f16 d_w) * f32(f16 d_x), (float) dot4_e, acc_e), dot4_e the exact dot of the UNSIGNED weights
//   (Q4_1: the nibble, 0..15; Q5_1: nibble | bit << 4, 0..31; both valid int8, so the signed dot serves) with the activation bytes 4e .. 4e+3;
//   one SCALAR chain per row: summs = summs + f32(f16 m_w) * f32(f16 s_x).  Whether the reference build contracts this statement into an fma cannot be told
//   from its outputs and does not matter: the product of two widened f16 values is exact in f32, so both forms give the same bits (tests/legacy1_ref.py;
//   the stored reference outputs, tests/golden/legacy1_kats.npz, are reproduced by either).  Here: a product, then a sum (-ffp-contract=off).
// Result: hsum(acc) + summs.  Wave lane r*8 + e is SIMD lane e of row r; every lane of a row carries the row's summs chain redundantly (K/32 dependent
// steps whose order must not change: nothing crosses lanes).
#pragma once
#include "bamd_q0_device.h"

template <int TYPE> struct RecQ1 { uint4 q0, q1, sd, sm; uint32_t qh; };  // q0 / q1: the lane's nibble dwords of blocks 0-3 / 4-7; sd / sm: the row's eight f16 d / m; qh: Q5_1 only
template <int TYPE> __device__ __forceinline__ void pin_rec(RecQ1<TYPE> & R) { pin(R.q0); pin(R.q1); pin(R.sd); pin(R.sm); if (TYPE == BAMD_Q5_1) pin(R.qh); }
template <int TYPE> __device__ __forceinline__ void load_rec(RecQ1<TYPE> & R, bamd_rsrc rs, int soff, int lane) {
    const uint32_t l = (uint32_t) lane;
    const uint32_t vo = ((l >> 3) * 4u + (l & 3u)) * 32u;                // lanes e and e + 4 share the nibble bytes
    R.q0 = bl128(rs, vo, soff); R.q1 = bl128(rs, vo + 16u, soff);
    const uint32_t dm = (TYPE == BAMD_Q5_1 ? 1280u : 1024u) + (l >> 3) * 32u;
    R.sd = bl128(rs, dm, soff); R.sm = bl128(rs, dm + 16u, soff);
    if (TYPE == BAMD_Q5_1) R.qh = bl32(rs, 1024u + l * 4u, soff); else R.qh = 0u;
}
// the four weights of block c for lane e, unsigned and without an offset (ggml-quants.c:4364, :5021-5024)
template <int TYPE> __device__ __forceinline__ uint32_t q1_weights(const RecQ1<TYPE> & R, int c, int e) {
    const uint32_t raw = c < 4 ? BAMD_Q0_COMP(R.q0, c) : BAMD_Q0_COMP(R.q1, c - 4);
    const uint32_t nib = (raw >> ((e >> 2) * 4)) & 0x0f0f0f0fu;
    if (TYPE == BAMD_Q4_1) return nib;
    return nib | (((R.qh >> c) & 0x01010101u) << 4);
}
__device__ __forceinline__ float q1_half(const uint4 & v, int c) {
    const uint32_t w = BAMD_Q0_COMP(v, c >> 1);
    return h2f((c & 1) ? w >> 16 : w & 0xffffu);
}
// the terms of one record for lane (r, e): s[c] = d_w * d_x, f[c] = (float) of the exact 4-byte dot, ms[c] = m_w * s_x (each one f32 product of two widened f16)
template <int TYPE> __device__ __forceinline__ void q1_terms(const RecQ1<TYPE> & R, int ci, int lane, const uint32_t * q8, const float * ys, float (&s)[8], float (&f)[8], float (&ms)[8]) {
    const int e = lane & 7;
    const uint4 a0 = *(const uint4 *) (q8 + ci * 64 + e * 8), a1 = *(const uint4 *) (q8 + ci * 64 + e * 8 + 4);
    const uint4 y0 = *(const uint4 *) (ys + ci * 8), y1 = *(const uint4 *) (ys + ci * 8 + 4);
    const uint32_t aq[8] = { a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w };
    const uint32_t yv[8] = { y0.x, y0.y, y0.z, y0.w, y1.x, y1.y, y1.z, y1.w };      // {f16 d, f16 s} of the eight activation blocks
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        s[c] = q1_half(R.sd, c) * h2f(yv[c] & 0xffffu);
        ms[c] = q1_half(R.sm, c) * h2f(yv[c] >> 16);
        f[c] = (float) sdot4(q1_weights(R, c, e), aq[c]);
    }
}
// eight steps of the row's scalar chain, in block order (the ONLY place its order is defined): ms[c] is an exact product, the sum rounds
__device__ __forceinline__ void q1_summs8(float & summs, const float (&ms)[8]) {
#pragma unroll
    for (int c = 0; c < 8; ++c) summs = summs + ms[c];
}
__device__ __forceinline__ float q1_finish_row(float acc, float summs) { return q0_finish_row(acc) + summs; }      // sumf = hsum_float_8(acc) + summs
