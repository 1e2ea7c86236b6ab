// bamd_prefill2_lowbit.h — the Q3_K / Q2_K policy of the eight-wave matrix-core body (bamd_prefill2_body.h) and the sizes of its side table, shared by the dense
// kernels (bamd_prefill2.hip, where the table's kernel stands) and the grouped mixture-of-experts ones (bamd_moe_batch_kq_mfma.hip).
// ---- Q3_K / Q2_K: ONE fragment and ONE MFMA per (e, token tile) ---------------------------------------------------------------------------------
// Reference: ggml_vec_dot_q3_K_q8_K / ggml_vec_dot_q2_K_q8_K (ggml-quants.c:6161-6263, :5553-5617).  SIMD lane e owns bytes 4e..4e+3 of the eight chunks c,
// its scale is that of the 16-element sub-block 2c + (e >= 4): e-half h and chunk pairs (2g, 2g+1) per MFMA lane group g, as for Q6_K.  (sc - 32) x q with
// q = low2 + 4 hbit - 4 (Q3_K, |.| <= 128) and sc x q (Q2_K, <= 45) are exact f16, so one v_mfma_f32_16x16x32_f16 gives the exact isum_e (|isum_e| <= 2^19,
// every partial sum an integer): no split scale, no chained second MFMA.  Wave-stream lane (r, e) holds two qs dwords j (fields k = 0..3 = chunk 4j + k) and,
// Q3_K, the hmask dword (bit c of byte u = element 32c + 4e + u): the pieces of MFMA lanes (row, g = 2p + j') come from qs dword p, fields 2j', 2j'+1, and
// hmask bits 2g, 2g+1.  Fragment ring: the second fragment slot of every pair unused (the 2 x X_FR pitch keeps the builders' stores
// of eight lanes on eight bank quads).
// Q2_K's min term goes into the same accumulator in front of the dot term (chain_step; X2Hdr::chain): prod_e = mins[2e] bsum16[2e] + mins[2e+1] bsum16[2e+1] is one
// v_dot2_f32_f16 per row and token on packed pairs — the mins of a row as sixteen f16 in the consumer header, the sums of sixteen activations as sixteen f16 at
// bytes 576..607 of the token record (quantize_batch_kernel); |prod_e| <= 61 440, exact in f32 in any order.
#pragma once
#include "bamd_prefill2_body.h"

#define XL_CH2_RT 640                                      /* Q2_K consumer header of a row tile: 16 x d f32 | 16 x dmin f32 | 16 rows x 16 f16 mins */
#define XL_CH3_RT 64                                       /* Q3_K: 16 x d f32 */
#define XL_PH_SB 4096                                      /* builder operands of a row block and super-block: [e-half][4 row tiles][64 MFMA lanes][{s, s}, {s', s'}] */

template <bool Q2>
struct X2LowBit {
    static constexpr uint32_t RECB = Q2 ? BAMD_RECB_Q2K : BAMD_RECB_Q3K;
    static constexpr int CHRT = Q2 ? XL_CH2_RT : XL_CH3_RT, PH_SB = XL_PH_SB, PH_RT = 512, NFRAG = 1;
    static constexpr bool LATE_CHAIN = true;                   // one iteration behind: no MFMA -> VALU wait states in front of the chain
    typedef X2Hdr<Q2> Hdr;
    // where a builder lane (p, r, el) finds its weight sets: per half step qs dword p and the hmask dword of stream lane (r, e)
    static __device__ __forceinline__ void lane_ptrs(const uint8_t * w, size_t rec0, int bp, int br, int bel, const uint8_t * & wqs, const uint8_t * & whm) {
        wqs = w + rec0 + (size_t) ((br * 8 + bel) * 8 + bp * 4);
        whm = w + rec0 + 512 + (size_t) ((br * 8 + bel) * 4);
    }
    uint32_t hm[2], qs[2]; uint2 sc[2][2];                     // (hm in front of qs: the order of the ring loop's phi nodes, and with it the register assignment, follows the members)
    bamd_h2u v0, v1, v2, v3;
    template <int S> __device__ __forceinline__ void load_set(int hs, const uint8_t * wqs, const uint8_t * whm, const uint8_t * phb, int bp) {  // operands of half step hs = 2 ci + h
        const int ci = hs >> 1, h = hs & 1;
        qs[S] = *(const uint32_t *) (wqs + (size_t) ci * RECB + h * 32);
        if (!Q2) hm[S] = *(const uint32_t *) (whm + (size_t) ci * RECB + h * 16) >> (4 * bp);      // bits 2g, 2g+1 of every byte at bits 2j, 2j+1
        sc[S][0] = *(const uint2 *) (phb + (size_t) hs * (PH_SB / 2)); sc[S][1] = *(const uint2 *) (phb + (size_t) hs * (PH_SB / 2) + 128);
    }
    __device__ __forceinline__ void build_a(int S, int j) {
        const _Float16 kz = Q2 ? (_Float16) -1024.f : (_Float16) -1028.f;
        const bamd_h2 kzero = { kz, kz };
        const uint32_t q = qs[S], hq = Q2 ? 0u : hm[S];
        uint32_t uA = (q >> (4 * j)) & 0x03030303u, uB = (q >> (4 * j + 2)) & 0x03030303u;
        if (!Q2) { uA |= ((hq >> (2 * j)) & 0x01010101u) << 2; uB |= ((hq >> (2 * j + 1)) & 0x01010101u) << 2; }
        bamd_h2u c;
        c.u = __builtin_amdgcn_perm(0x64646464u, uA, 0x04010400u); v0.h = c.h + kzero;      // Q3_K: (1024 + low2 + 4 hbit) - 1028 = q; Q2_K: (1024 + q) - 1024, exact
        c.u = __builtin_amdgcn_perm(0x64646464u, uA, 0x04030402u); v1.h = c.h + kzero;
        c.u = __builtin_amdgcn_perm(0x64646464u, uB, 0x04010400u); v2.h = c.h + kzero;
        c.u = __builtin_amdgcn_perm(0x64646464u, uB, 0x04030402u); v3.h = c.h + kzero;
    }
    __device__ __forceinline__ void build_b(int S, int j, unsigned char * dst) const {
        const uint2 s = sc[S][j];
        bamd_h2u s0, s1, x0, x1, x2, x3; s0.u = s.x; s1.u = s.y;
        x0.h = v0.h * s0.h; x1.h = v1.h * s0.h; x2.h = v2.h * s1.h; x3.h = v3.h * s1.h;
        *(uint4 *) dst = (uint4) { x0.u, x1.u, x2.u, x3.u };
    }
};
