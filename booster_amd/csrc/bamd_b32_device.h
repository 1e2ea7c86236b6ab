// bamd_b32_device.h — device code shared by the kernels of the 32-weight block formats (bamd_matvec_b32.h: single-token mat-vec; bamd_prefill_b32.hip: batched
// prompt mat-mul on the integer-dot kernel; the matrix-core one, bamd_prefill2_b32.hip, restates the chains for its own lane layout): the Q8_0 / Q8_1 activation
// prologue, the wave-stream records (layout: bamd_formats.h), their block terms and the chains.  Two families, told apart by b32_has_min(TYPE):
//   without a minimum  Q8_0 / Q4_0 / Q5_0   weights {d, q}, Q8_0 activations {d, q}
//                      IQ4_NL               the Q4_0 record; a nibble indexes a table of 16 int8; TWO accumulators (b32_two_acc(TYPE)), see below
//   with a minimum     Q4_1 / Q5_1          weights {d, m, q}, Q8_1 activations {d, s, q}
//
// NUMERICS (contract: bamd_device.h).  Reference functions restated here (cpp/ = the reference tree):
//   quantize_row_q8_0 (AVX2)         ggml/src/ggml-quants.c:936-994
//   quantize_row_q8_1 (AVX2)         ggml/src/ggml-quants.c:1272-1333     d, id and the bytes are quantize_row_q8_0's; s = f16(d_f32 * (float) sum of the quants)
//   tinyBLAS_Q0_AVX::gemm            ggml/src/llamafile/sgemm.cpp:711-759 (Q8_0 and Q4_0 weights, one token and many), load :773-775, :797-
//   ggml_vec_dot_q5_0_q8_0 (AVX2)    ggml/src/ggml-quants.c:4644-4666     (the same chain; _q4_0_q8_0 :3900-3923 and _q8_0_q8_0 :5227- have its shape too)
//   ggml_vec_dot_q4_1_q8_1 (AVX2)    ggml/src/ggml-quants.c:4344-4377     (llamafile_sgemm has no case for these types: one token and many go through vec_dot)
//   ggml_vec_dot_q5_1_q8_1 (AVX2)    ggml/src/ggml-quants.c:5009-5034
//   ggml_vec_dot_iq4_nl_q8_0 (AVX2)  ggml/src/ggml-quants.c:11596-11670, AVX2 branch :11643-11670 (llamafile_sgemm has no case for the type either, sgemm.cpp:865-985)
// Without a minimum, one output = ONE 8-lane f32 accumulator: for the 32-blocks l = 0 .. K/32 - 1 in order, lane e: acc_e = fma(f32(f16 d_w) * f32(f16 d_x), (float) dot4_e,
// acc_e), with dot4_e the exact signed dot of bytes 4e .. 4e+3 of the weight block and the activation block (sign_epi8 / maddubs: |pair sum| <= 2 * 128 * 127, never
// saturates; activations never hold -128), then hsum (finish_row's tree).  Wave lane r*8 + e is SIMD lane e of row r.
// With a minimum, one output = TWO accumulators over the same blocks in order:
//   the 8-lane chain above, dot4_e now the exact dot of the UNSIGNED weights (Q4_1: the nibble, 0..15; Q5_1: nibble | bit << 4, 0..31; both valid int8, so the
//   signed dot serves) with the activation bytes 4e .. 4e+3;
//   one SCALAR chain per row: summs = summs + f32(f16 m_w) * f32(f16 s_x).  Whether the reference build contracts this statement into an fma cannot be told
//   from its outputs and does not matter: the product of two widened f16 values is exact in f32, so both forms give the same bits (tests/legacy1_ref.py;
//   the stored reference outputs, tests/golden/legacy1_kats.npz, are reproduced by either).  Here: a product, then a sum (-ffp-contract=off).
// Result: hsum(acc) + summs.  Every lane of a row carries the row's summs chain redundantly (K/32 dependent steps whose order must not change: nothing crosses lanes).
// IQ4_NL, one output = TWO 8-lane accumulators of the first shape (:11649-11668): the loop takes two blocks per iteration, accum1_e = fma(f32(d_x) * f32(d_w),
// (float) p_e, accum1_e) over the EVEN blocks l in order and accum2_e likewise over the ODD ones, p_e the exact dot of kvalues_iq4nl[nibble] (:3548) with the
// activation bytes 4e .. 4e+3 (mul_add_epi8 / madd: |pair sum| <= 2 * 127 * 127, never saturates); then accum1 + accum2 lane by lane and hsum_float_8 (:11670).
// K is a multiple of 256: the block count is even and the reference's scalar tail never runs.  A record is eight consecutive blocks, so a block's parity is the
// parity of its index c in the record.
#pragma once
#include <type_traits>
#include "bamd_device.h"
constexpr bool b32_has_min(int type) { return type == BAMD_Q4_1 || type == BAMD_Q5_1; }
constexpr bool b32_has_qh(int type) { return type == BAMD_Q5_0 || type == BAMD_Q5_1; }
constexpr bool b32_two_acc(int type) { return type == BAMD_IQ4_NL; }
// floats of a parked record of the split-K kernels: f[c][lane] (8 x 64 floats) + the scale products s[r][c] (8 x 8); with a minimum also the row's m * s products ms[r][c] (8 x 8)
constexpr int b32_term_floats(bool has_min) { return has_min ? 640 : 576; }

// ===========================================================================================================
// Activation prologue: f32 vector [K] -> Q8_0 blocks in LDS, optionally RMSNorm * weight first.  The image uses the K-quant prologue's area and offsets
// (carve_lds): q8[i*64 + e*8 + c] = the 4 int8 of elements 4e .. 4e+3 of 32-block c of the i-th group of 256; the S area holds, as f32, the f16-rounded
// scale d of block (i, c) at [i*8 + c] (the dots use the f16 value: ggml-quants.c:960-961); yd is unused.  292 bytes per 256 values, as before.
// Lane l of the wave that quantises group i holds elements 4l .. 4l+3: block c = l >> 3, so a block's maximum is a reduction over 8 consecutive lanes.
// ===========================================================================================================
template <bool NORM>
struct ActProQ0 : ActPro<NORM> {
    // Q1: the Q8_1 form of the weight types with a minimum — the same d, id and bytes, and the block's 4-byte slot of the S area holds the block's
    // pair {f16 d, f16 s} (d low) in place of d widened
    template <int NB = BAMD_ACT_BATCH, bool Q1 = false>
    __device__ __forceinline__ void quantize_batch_q0(float scale, int K, int i0, uint32_t * q8, float * ys, int bstride = 0, int blimit = 0) {
        const int lane = threadIdx.x & 63;
        const int nwaves = bstride ? bstride : (int) (blockDim.x >> 6), nb = bstride ? blimit : (K >> 8);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            float4 v = this->v[b];
            if (NORM) {                                  // y = (x*scale)*w : ggml_vec_scale_f32 then ggml_mul (llama.cpp:7940-7950)
                const float4 w = this->w[b];
                v.x = (v.x * scale) * w.x; v.y = (v.y * scale) * w.y; v.z = (v.z * scale) * w.z; v.w = (v.w * scale) * w.w;
            }
            uint32_t am = __float_as_uint(fmaxf(fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fabsf(v.z)), fabsf(v.w)));   // non-negative floats order like their bits
            am = umax_(am, (uint32_t) dpp_z<DPP_XOR1>((int) am)); am = umax_(am, (uint32_t) dpp_z<DPP_XOR2>((int) am));
            am = umax_(am, (uint32_t) dpp_z<DPP_HALF_MIRROR>((int) am));
            const float amax = __uint_as_float(am);      // max |x| of this lane's 32-block (:944-953: a max tree, any order)
            const float d = amax / 127.f;                // :956-958
            const float id = amax != 0.0f ? 127.f / amax : 0.0f;
            // _mm256_round_ps(x * id, NEAREST) then cvtps_epi32 (:962-976): x * id + 1.5 * 2^23 rounds the product to an integer, ties to even, and
            // leaves its two's-complement low byte in the low byte of the sum (|x * id| <= 127 (1 + 2^-23): the saturating packs never bind)
            const float t0 = id * v.x + 12582912.f, t1 = id * v.y + 12582912.f, t2 = id * v.z + 12582912.f, t3 = id * v.w + 12582912.f;
            const uint32_t p01 = __builtin_amdgcn_perm(__float_as_uint(t1), __float_as_uint(t0), 0x0c0c0400u);
            const uint32_t p23 = __builtin_amdgcn_perm(__float_as_uint(t3), __float_as_uint(t2), 0x0c0c0400u);
            const uint32_t packed = __builtin_amdgcn_perm(p23, p01, 0x05040100u);
            // quantize_row_q8_1 (ggml-quants.c:1319): s = f16(d * (float) sum of the block's 32 quants), d the UNROUNDED f32 quotient; the sum is exact (|sum| <= 4064)
            // The product is rounded to f32 FIRST and to f16 after (two roundings, as the reference's scalar code does): its bits pass through a register of
            // their own, or the compiler folds the multiply into the conversion (v_fma_mixlo_f16: ONE rounding of the exact product, another f16 for about
            // one block in a thousand — found by tests/test_gpu_legacy1_ops.py)
            const int qsum = Q1 ? group8_sum(sdot4(packed, 0x01010101u)) : 0;
            uint32_t sbits = Q1 ? __float_as_uint(d * (float) qsum) : 0u;
            if (Q1) pin(sbits);
            const int i = i0 + b * nwaves;
            if (i < nb) {                                // wave-uniform
                q8[i * 64 + (lane & 7) * 8 + (lane >> 3)] = packed;
                if ((lane & 7) == 0) {
                    if (Q1) ((uint32_t *) ys)[i * 8 + (lane >> 3)] = (uint32_t) f2h(d) | ((uint32_t) f2h(__uint_as_float(sbits)) << 16);
                    else ys[i * 8 + (lane >> 3)] = h2f(f2h(d));
                }
            }
        }
    }
    // ActPro::finish with the Q8_0 quantiser; the f64 sum of squares and its guard are the same code
    template <bool Q1 = false>
    __device__ __forceinline__ void finish_q0(const float * __restrict__ x, const float * __restrict__ nw, float eps, int K, uint32_t * q8, float * ys, double * red) {
        const int lane = threadIdx.x & 63, wave = wave_id(), nwaves = blockDim.x >> 6, nb = K >> 8;
        const int step = nwaves * BAMD_ACT_BATCH;
        float scale = 1.0f;
        if (NORM) {
            double s = 0.0;
#pragma unroll
            for (int b = 0; b < BAMD_ACT_BATCH; ++b) {
                const float4 v = this->v[b];
                if (this->okmask >> b & 1) { s += (double) (v.x * v.x); s += (double) (v.y * v.y); s += (double) (v.z * v.z); s += (double) (v.w * v.w); }
            }
            for (int i0 = wave + step; i0 < nb; i0 += step) {
                ActPro<NORM> t; t.issue(x, nw, K, i0);
#pragma unroll
                for (int b = 0; b < BAMD_ACT_BATCH; ++b) {
                    if (t.okmask >> b & 1) { s += (double) (t.v[b].x * t.v[b].x); s += (double) (t.v[b].y * t.v[b].y); s += (double) (t.v[b].z * t.v[b].z); s += (double) (t.v[b].w * t.v[b].w); }
                }
            }
            s = wave_sum_f64(s);
            if (lane == 0) red[wave] = s;
            __syncthreads();
            double tot = 0.0;
            for (int w2 = 0; w2 < nwaves; ++w2) tot += red[w2];
            double md = (K & (K - 1)) == 0 ? tot * (1.0 / (double) K) : tot / (double) K;      // ggml.c:11879; see ActPro::finish
            float mean = (float) md;
            if (!f32_rounding_safe(md, BAMD_F64_GUARD_ULPS(K))) {
                __syncthreads();
                if (threadIdx.x == 0) {                                     // the reference's order, one lane (ggml.c:11874-11877)
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
        this->template quantize_batch_q0<BAMD_ACT_BATCH, Q1>(scale, K, wave, q8, ys);
        for (int i0 = wave + step; i0 < nb; i0 += step) {
            ActProQ0<NORM> t; t.issue(x, nw, K, i0);
            t.template quantize_batch_q0<BAMD_ACT_BATCH, Q1>(scale, K, i0, q8, ys);
        }
        __syncthreads();
    }
};

// ===========================================================================================================
// Records (layout: bamd_formats.h) and the chains
// ===========================================================================================================
// q0 / q1: the lane's dwords (nibble dwords but for Q8_0) of blocks 0-3 / 4-7; sd: the row's eight f16 d; qh: Q5_0 / Q5_1 only; sm: the row's eight f16 m, a member only
// of the types with a minimum (an unused uint4 in a ring is four VGPRs per record).  A specialisation, not a base class that holds sm: the members' order is the order
// in which a ring's registers are copied at the loop's edge, and with sm in front the Q4_1 stream waited for a record's fourth load (s_waitcnt vmcnt(12)) before
// it touched the first, where this order waits for them one by one
template <int TYPE, bool MIN = b32_has_min(TYPE)> struct RecB32 { uint4 q0, q1, sd; uint32_t qh; };
template <int TYPE> struct RecB32<TYPE, true> { uint4 q0, q1, sd, sm; uint32_t qh; };
template <int TYPE> __device__ __forceinline__ void pin_rec(RecB32<TYPE> & R) {
    pin(R.q0); pin(R.q1); pin(R.sd);
    if constexpr (b32_has_min(TYPE)) pin(R.sm);
    if (b32_has_qh(TYPE)) pin(R.qh);
}
template <int TYPE> __device__ __forceinline__ void load_rec(RecB32<TYPE> & R, bamd_rsrc rs, int soff, int lane) {
    const uint32_t l = (uint32_t) lane;
    if (TYPE == BAMD_Q8_0) {
        R.q0 = bl128(rs, l * 16u, soff); R.q1 = bl128(rs, 1024u + l * 16u, soff);
        R.sd = bl128(rs, 2048u + (l >> 3) * 16u, soff);
        R.qh = 0u;
        return;
    }
    const uint32_t vo = ((l >> 3) * 4u + (l & 3u)) * 32u;                // lanes e and e + 4 share the nibble bytes
    R.q0 = bl128(rs, vo, soff); R.q1 = bl128(rs, vo + 16u, soff);
    constexpr uint32_t so = b32_has_qh(TYPE) ? 1280u : 1024u;            // the scales sit behind the fifth bits
    if constexpr (b32_has_min(TYPE)) {                                   // (the request order of each family is the one its kernels were tuned with)
        R.sd = bl128(rs, so + (l >> 3) * 32u, soff); R.sm = bl128(rs, so + (l >> 3) * 32u + 16u, soff);
        R.qh = b32_has_qh(TYPE) ? bl32(rs, 1024u + l * 4u, soff) : 0u;
    } else {
        R.qh = b32_has_qh(TYPE) ? bl32(rs, 1024u + l * 4u, soff) : 0u;
        R.sd = bl128(rs, so + (l >> 3) * 16u, soff);
    }
}
#define BAMD_B32_COMP(v, k) ((k) == 0 ? (v).x : (k) == 1 ? (v).y : (k) == 2 ? (v).z : (v).w)
// the four weights of block c for lane e as int8.  Without a minimum: Q8_0 as stored (-128 included); Q4_0 nibble - 8 = (n + 0x78) ^ 0x80 per byte (sgemm.cpp:773-775,
// low nibbles = elements 0-15, high = 16-31); Q5_0 (nibble | bit 4) - 16 = (x + 0x70) ^ 0x80 (ggml-quants.c:4655-4658: a clear qh bit ORs 0xF0 into the nibble).  No
// inter-byte carry.  With a minimum: unsigned and without an offset (ggml-quants.c:4364, :5021-5024).  IQ4_NL: kvalues_iq4nl[nibble] (_mm_shuffle_epi8, :11656-11659) as
// byte permutes of the table in registers: its halves 0-7 and 8-15 selected by the nibble's low three bits, then of each byte pair the half its bit 3 names
// (b32_iq4nl_values: bamd_device.h, where the table stands, beside its by-index spelling iq4nl_value; IQ4_XS and the matrix-core kernel, bamd_prefill2_b32.hip, call it too)
template <int TYPE> __device__ __forceinline__ uint32_t b32_weights(const RecB32<TYPE> & R, int c, int e) {
    const uint32_t raw = c < 4 ? BAMD_B32_COMP(R.q0, c) : BAMD_B32_COMP(R.q1, c - 4);
    if (TYPE == BAMD_Q8_0) return raw;
    const uint32_t nib = (raw >> ((e >> 2) * 4)) & 0x0f0f0f0fu;
    if (TYPE == BAMD_IQ4_NL) return b32_iq4nl_values(nib);
    const uint32_t u = b32_has_qh(TYPE) ? nib | (((R.qh >> c) & 0x01010101u) << 4) : nib;
    if (b32_has_min(TYPE)) return u;
    return (u + (b32_has_qh(TYPE) ? 0x70707070u : 0x78787878u)) ^ 0x80808080u;
}
__device__ __forceinline__ float b32_half(const uint4 & v, int c) {       // the c-th of eight f16, widened
    const uint32_t w = BAMD_B32_COMP(v, c >> 1);
    return h2f((c & 1) ? w >> 16 : w & 0xffffu);
}
// the terms of one record for lane (r, e): s[c] = d_w * d_x, f[c] = (float) of the exact 4-byte dot and, with a minimum, ms[c] = m_w * s_x (each one f32 product of
// two widened f16).  The activation block's 4-byte slot: d_x widened to f32 (Q8_0 form) or the pair {f16 d, f16 s} (Q8_1 form).
// ms: eight floats, REQUIRED for a type with a minimum (written without a check: the default is only for callers that serve no such type) and never touched
// for the others.  The mat-vec kernels pass nothing there: an array that nobody writes costs no register, but it renames the registers of the RMSNorm
// instances (matvec_q0_split_kernel, matvec_b32_kernel<false, ..>), which are instruction for instruction what they were only without it.  The batched and
// co-launch kernels are that with a dead array too, and keep the shorter call
template <int TYPE> __device__ __forceinline__ void b32_terms(const RecB32<TYPE> & R, int ci, int lane, const uint32_t * q8, const float * ys, float (&s)[8], float (&f)[8], float * ms = nullptr) {
    const int e = lane & 7;
    const uint4 a0 = *(const uint4 *) (q8 + ci * 64 + e * 8), a1 = *(const uint4 *) (q8 + ci * 64 + e * 8 + 4);
    typedef typename std::conditional<b32_has_min(TYPE), uint4, float4>::type Y4;      // the eight slots of the record's activation blocks, as their form holds them
    const Y4 y0 = *(const Y4 *) (ys + ci * 8), y1 = *(const Y4 *) (ys + ci * 8 + 4);
    const uint32_t aq[8] = { a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w };
    const decltype(y0.x) yv[8] = { y0.x, y0.y, y0.z, y0.w, y1.x, y1.y, y1.z, y1.w };
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        if constexpr (b32_has_min(TYPE)) {
            s[c] = b32_half(R.sd, c) * h2f(yv[c] & 0xffffu);
            ms[c] = b32_half(R.sm, c) * h2f(yv[c] >> 16);
        } else {
            s[c] = b32_half(R.sd, c) * yv[c];
        }
        f[c] = (float) sdot4(b32_weights(R, c, e), aq[c]);
    }
}
// eight steps of the lane's chain, in block order (the ONLY place its order is defined for these types)
__device__ __forceinline__ void b32_chain8(float & acc, const float (&s)[8], const float (&f)[8]) {
#pragma unroll
    for (int c = 0; c < 8; ++c) acc = fmaf(s[c], f[c], acc);
}
// the two-accumulator shape (b32_two_acc: IQ4_NL, ggml-quants.c:11651-11668): the even blocks of the record into acc1, the odd ones into acc2, each in block order
// (the ONLY place this order is defined); the row ends with b32_finish_row(acc1 + acc2) (:11670)
__device__ __forceinline__ void b32_chain8(float & acc1, float & acc2, const float (&s)[8], const float (&f)[8]) {
#pragma unroll
    for (int c = 0; c < 8; c += 2) { acc1 = fmaf(s[c], f[c], acc1); acc2 = fmaf(s[c + 1], f[c + 1], acc2); }
}
// eight steps of the row's scalar chain, in block order (the ONLY place its order is defined): ms[c] is an exact product, the sum rounds
__device__ __forceinline__ void b32_summs8(float & summs, const float (&ms)[8]) {
#pragma unroll
    for (int c = 0; c < 8; ++c) summs = summs + ms[c];
}
__device__ __forceinline__ float b32_finish_row(float acc) { const RowAcc A = { acc, 0.f }; return finish_row<BAMD_Q8_0>(A); }      // hsum: sgemm.cpp:63-76 = hsum_float_8's tree
// with a minimum: sumf = hsum_float_8(acc) + summs
template <bool MIN> __device__ __forceinline__ float b32_finish_row(float acc, float summs) { return MIN ? b32_finish_row(acc) + summs : b32_finish_row(acc); }
