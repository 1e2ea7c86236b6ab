// bamd_prefill2_xs.h — the IQ4_XS policy of the eight-wave matrix-core body (bamd_prefill2_body.h) and the sizes of its side table, shared by the dense kernel
// (bamd_prefill2_xs.hip: the reasons, and the table's kernel) and the grouped mixture-of-experts one (bamd_moe_batch_xs_mfma.hip).
#pragma once
#include "bamd_prefill2_body.h"

#define XS_CH_RT 64                                        /* consumer header of a row tile: 16 x d f32 */
#define XS_PH_SB 4096                                      /* builder operands of a row block and super-block: [4 row tiles][64 MFMA lanes][{sa, sa}, {sl, sl}, {sa', sa'}, {sl', sl'}] */

struct X2IQ4XS {
    static constexpr uint32_t RECB = BAMD_RECB_IQ4XS;
    static constexpr int CHRT = XS_CH_RT, PH_SB = XS_PH_SB, PH_RT = 1024, NFRAG = 2;
    static constexpr bool LATE_CHAIN = true;                   // measured both ways in one job, 2048-token prompts of the 8B shape: 15 242 tok/s against 14 970 with the chain behind its own MFMAs
    typedef X2Hdr<false> Hdr;
    // where a builder lane (p, r, el) finds its weight set: dwords 4p .. 4p+3 of stream lane (r, el) (the second pointer is not used)
    static __device__ __forceinline__ void lane_ptrs(const uint8_t * w, size_t rec0, int bp, int br, int bel, const uint8_t * & wqs, const uint8_t * & wnone) {
        wqs = w + rec0 + (size_t) ((br * 4 + bel) * 32 + bp * 16);
        wnone = wqs;
    }
    uint4 qs[2] = { { 0u, 0u, 0u, 0u }, { 0u, 0u, 0u, 0u } }, sc[2][2] = { { { 0u, 0u, 0u, 0u }, { 0u, 0u, 0u, 0u } }, { { 0u, 0u, 0u, 0u }, { 0u, 0u, 0u, 0u } } };
    bamd_h2u v0, v1, v2, v3;
    template <int S> __device__ __forceinline__ void load_set(int hs, const uint8_t * wqs, const uint8_t *, const uint8_t * phb, int) {      // S = 0: set 0 -> set 1, then super-block hs >> 1 into set 0
        if (S == 0) {
            const int ci = hs >> 1;
            qs[1] = qs[0]; sc[1][0] = sc[0][0]; sc[1][1] = sc[0][1];
            qs[0] = *(const uint4 *) (wqs + (size_t) ci * RECB);
            sc[0][0] = *(const uint4 *) (phb + (size_t) ci * PH_SB); sc[0][1] = *(const uint4 *) (phb + (size_t) ci * PH_SB + 256);
        }
    }
    __device__ __forceinline__ void build_a(int S, int j) {       // set S feeds half step H = S: nibble S of blocks 2g, 2g + 1, g = 2p + j
        const bamd_h2 k1152 = { (_Float16) -1152.f, (_Float16) -1152.f };
        const uint4 q = qs[S]; const uint32_t sh = 4u * (uint32_t) S;
        const uint32_t uA = b32_iq4nl_values(((j ? q.z : q.x) >> sh) & 0x0f0f0f0fu) ^ 0x80808080u, uB = b32_iq4nl_values(((j ? q.w : q.y) >> sh) & 0x0f0f0f0fu) ^ 0x80808080u;
        bamd_h2u c;
        c.u = __builtin_amdgcn_perm(0x64646464u, uA, 0x04010400u); v0.h = c.h + k1152;      // (1024 + value + 128) - 1152 = value, exact
        c.u = __builtin_amdgcn_perm(0x64646464u, uA, 0x04030402u); v1.h = c.h + k1152;
        c.u = __builtin_amdgcn_perm(0x64646464u, uB, 0x04010400u); v2.h = c.h + k1152;
        c.u = __builtin_amdgcn_perm(0x64646464u, uB, 0x04030402u); v3.h = c.h + k1152;
    }
    __device__ __forceinline__ void build_b(int S, int j, unsigned char * dst) const {  // dst: the A_a fragment (v x sa); A_l (v x sl) X_FR bytes behind it
        const uint4 s = sc[S][j];
        bamd_h2u sa0, sl0, sa1, sl1, x0, x1, x2, x3; sa0.u = s.x; sl0.u = s.y; sa1.u = s.z; sl1.u = s.w;
        x0.h = v0.h * sa0.h; x1.h = v1.h * sa0.h; x2.h = v2.h * sa1.h; x3.h = v3.h * sa1.h;
        *(uint4 *) dst = (uint4) { x0.u, x1.u, x2.u, x3.u };
        x0.h = v0.h * sl0.h; x1.h = v1.h * sl0.h; x2.h = v2.h * sl1.h; x3.h = v3.h * sl1.h;
        *(uint4 *) (dst + X_FR) = (uint4) { x0.u, x1.u, x2.u, x3.u };
    }
};
