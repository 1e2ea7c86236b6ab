// bamd_prefill2_xs.hip — the exact matrix-core prompt mat-mul for IQ4_XS weights (x Q8_K): an IQ4_XS policy of the eight-wave body (bamd_prefill2_body.h) and its
// load-time side table, behind the switch BAMD_PREFILL_XS / bamd_set_prefill_xs (default off: bamd_prefill_family.h).  Reached through the launchers of
// bamd_prefill2.hip (bamd_launch_prefill_aux, bamd_launch_matmul_mfma2).  A translation unit of its own, built without packed-f32 instructions (booster_amd/build.py);
// the kernels of bamd_prefill2.hip keep their flags and their code objects.
//
// Reference: ggml_vec_dot_iq4_xs_q8_K, AVX2 branch (ggml-quants.c:11855-11890; restated above block_terms(RecIQ4XS), bamd_device.h).  Per output one f32 chain per
// SIMD lane e, acc_e = fma(d_w d_y, (float) isum_e, acc_e) per super-block, closed by hsum_float_8; isum_e sums (ls_ib - 32) x value[nibble] x q8 over weights
// 32 ib + 4 e + u: the chunk geometry of the K-quants, chunk c = block ib, so the Q8_K f16 token records are the B operand as they stand.
//   * Scale.  The scale of a chunk is the same for all eight e (Q6_K / Q3_K / Q2_K pick sub-block 2c + (e >= 4)): ONE set of builder operands per super-block,
//     4 KiB, serves both half steps.  s x v with s = ls - 32 in -32 .. 31 and v in -127 .. 113 reaches 4064 and is no exact f16 in general (31 x 113), so the
//     scale is split as Q6_K's is: s = sa + sl, sa = s & ~15 in {-32, -16, 0, 16}, sl = s & 15 in 0 .. 15.  sl x v (|.| <= 1905 < 2048) and sa x v (16 k v,
//     |k v| <= 254) are exact f16.
//   * Two MFMAs per (e, token tile), chained through the accumulator: S = A_l.B + (A_a.B + 0) = isum_e.  Every partial sum, in any internal order, is an integer,
//     and per element max(|sa x|, |(sa + sl) x|) <= 32 x 127 x 127, so every partial sum stays at or below 32 x 32 x 127 x 127 = 16 516 096 < 2^24: exact.
//     (No Q8_K byte is -128: the note at block_terms(RecIQ4XS).)
//   * Loads.  A builder lane (p, r, el) reads ONE 16-byte piece of the record per SUPER-BLOCK — dwords c = 4p .. 4p+3 of stream lane (r, el): blocks 2g, 2g + 1
//     of its MFMA lanes g = 2p + j — for BOTH half steps: half step H takes nibble H of the same bytes (lanes e and e + 4 of the reference share bytes).  Set 0
//     is requested while half step 2 ci runs and holds super-block ci + 1; just before that request its registers (super-block ci, waited for a half step ago)
//     are copied to set 1, from which the same half step builds the H = 1 fragments of ci.  load_set<1> has nothing to fetch.
//   * Nibbles to f16.  b32_iq4nl_values (bamd_device.h, where the table stands) ^ 0x80808080 is u = value + 128 (1 .. 241) per byte, v_perm with 0x64 widens it
//     to the f16 1024 + u, and - 1152 leaves the value, exact (the trick of bamd_prefill2_b32.hip for IQ4_NL).
//   * Consumer: X2Hdr<false> — d as f32 per row, d_y from the stage, one fma per (e, row, token).
// 199 VGPRs at 512 threads (two waves per SIMD, as the other policies), no scratch, LDS = X_LDS_BYTES (149 056 B).
// The policy X2IQ4XS and the XS_* sizes of the side table: bamd_prefill2_xs.h (shared with the grouped kernel of bamd_moe_batch_xs_mfma.hip).
#include "bamd_prefill2_xs.h"

size_t bamd_prefill_xs_ph_sb(void) { return XS_PH_SB; }
size_t bamd_prefill_xs_ch_sb(void) { return 4 * XS_CH_RT; }

// ---- load-time side table: grid (super-blocks, row tiles incl. the padding tiles of the last row block), 64 threads = the MFMA lanes (m = row of the tile, g).
// Per lane the split scales of blocks 2g (sa, sl) and 2g + 1 (sa', sl') of row m as packed f16 pairs, stored once for both e-halves; ls as iq4xs_scales decodes it
// (scales_l nibble | scales_h bit pair << 4, then - 32); d as f32 per row.  (4096 + 256) / 64 = 68 B per row and super-block; the kernel clamps its last loads: no slack
__global__ void __launch_bounds__(64) prefill_aux_iq4xs_kernel(const uint8_t * __restrict__ w, int nrows_pad, int nb, uint8_t * __restrict__ ph, uint8_t * __restrict__ ch) {
    const int ci = blockIdx.x, rtile = blockIdx.y, lane = threadIdx.x, m = lane & 15, g = lane >> 4;
    const int row = rtile * 16 + m;
    const size_t sb = (size_t) (rtile >> 2) * nb + ci;
    int s0 = 0, s1 = 0; uint32_t d16 = 0u;
    if (row < nrows_pad) {
        const uint2 hd = *(const uint2 *) (w + ((size_t) (row >> 3) * nb + ci) * BAMD_RECB_IQ4XS + 1024 + (row & 7) * 8);     // {d | scales_h << 16, scales_l[4]}
        const uint32_t sh = hd.x >> 16, lb = (hd.y >> (8 * g)) & 0xffu;                                                       // scales_l[g]: blocks 2g (low nibble) and 2g + 1
        s0 = (int) ((lb & 15u) | (((sh >> (4 * g)) & 3u) << 4)) - 32;
        s1 = (int) ((lb >> 4) | (((sh >> (4 * g + 2)) & 3u) << 4)) - 32;
        d16 = hd.x & 0xffffu;
    }
    const _Float16 a0 = (_Float16) (float) (s0 & ~15), l0 = (_Float16) (float) (s0 & 15), a1 = (_Float16) (float) (s1 & ~15), l1 = (_Float16) (float) (s1 & 15);
    bamd_h2u o0, o1, o2, o3; o0.h = (bamd_h2) { a0, a0 }; o1.h = (bamd_h2) { l0, l0 }; o2.h = (bamd_h2) { a1, a1 }; o3.h = (bamd_h2) { l1, l1 };
    *(uint4 *) (ph + sb * XS_PH_SB + (size_t) (rtile & 3) * 1024 + lane * 16) = (uint4) { o0.u, o1.u, o2.u, o3.u };
    if (g == 0) *(float *) (ch + sb * (4 * XS_CH_RT) + (rtile & 3) * XS_CH_RT + m * 4) = h2f(d16);
}

// ---- host side: what bamd_prefill2.hip's launchers call for the type ------------------------------------------------------------------------------
void bamd_launch_prefill_aux_xs(const void * w_stream, int nrows_pad, int K, void * ph, void * ch, hipStream_t s) {
    const int nb = K >> 8;
    hipLaunchKernelGGL(prefill_aux_iq4xs_kernel, dim3(nb, (nrows_pad + 63) / 64 * 4), dim3(64), 0, s, (const uint8_t *) w_stream, nrows_pad, nb, (uint8_t *) ph, (uint8_t *) ch);
}
int bamd_prefill_mfma_supported_xs(void) {
    return hipFuncSetAttribute((const void *) matmul_mfma2_kernel<BAMD_EPI_STORE, X2IQ4XS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) X_LDS_BYTES) == hipSuccess;
}
void bamd_launch_matmul_mfma_xs(const bamd_mma2_args & a, int epi, dim3 grid, hipStream_t s) {
    with_const(consts<BAMD_EPI_ADD, BAMD_EPI_SILU_MUL, BAMD_EPI_STORE>(), epi, [&](auto E) -> bool {
        hipLaunchKernelGGL((matmul_mfma2_kernel<decltype(E)::value, X2IQ4XS>), grid, dim3(512), X_LDS_BYTES, s, a);
        return true; });
}
