// bamd_moe_batch_kq_mfma.h — the grouped eight-wave matrix-core kernel moe_mfma2_kernel<MODE, F> behind a policy F of the dense eight-wave body, and its launch.
// Two translation units instantiate it, each with the build flags of the dense kernels of its policy: bamd_moe_batch_kq_mfma.hip (X2LowBit: Q3_K / Q2_K; the
// design is recorded at its head) and bamd_moe_batch_xs_mfma.hip (X2IQ4XS, built without packed-f32 instructions as bamd_prefill2_xs.hip is).
#pragma once
#include "bamd_prefill2_body.h"
#include "bamd_moe_batch_mfma.h"
#include "bamd_mv_select.h"

// wave (rt, tp) = row tile rt x slot tiles 2 tp, 2 tp + 1 of a tile of up to 64 pairs of ONE expert.  A step is HALF a super-block (four e); the fragment ring
// holds two half steps x 4 row tiles x 4 e x 2 fragment slots, the activation stage (whole super-blocks) is refilled every second half step
template <int MODE, class F>
__global__ void __launch_bounds__(512) moe_mfma2_kernel(bamd_moe_mma_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int ex, first, nt;
    if (!moe_tile(a, blockIdx.x, ex, first, nt)) return;          // past tiles[0]: out before the first barrier (workgroup-uniform)
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id(), m = lane & 15, g = lane >> 4;
    const int rt = wave >> 1, tp = wave & 1;
    const int nb = a.K >> 8;
    const int rb = blockIdx.y, rtg = rb * 4 + rt;
    const size_t b16 = BAMD_BLOB16_BYTES(nb);
    const uint8_t * wex = a.w + (size_t) ex * a.wstride, * ph = a.aux + (size_t) ex * a.astride, * ch = ph + a.ch_off;
    const uint32_t lds0 = (uint32_t) (size_t) (bamd_lds_vp) smem;
    // XStage::plan with the record sources gathered through the pair list: rounds 0..3 (and round 4 of waves 0..5) are the 38 chunks of 64 slot records (bytes
    // 576..607, Q2_K's bsum16, are chunks 36 and 37 of a record); round 4 of waves 6, 7 and, past 128 chunks (Q2_K: 160), half an instruction on wave 0 the consumer
    // headers; the 64 block scales d_y (behind a row's records) one 4-byte instruction on wave 1
    constexpr int NCH = 4 * F::CHRT / 16;
    XStage<NCH> stg;
#pragma unroll
    for (int r = 0; r < 4; ++r) stg.off[r] = moe_rec_off<MODE>(a, first, nt, r * 512 + tid, b16);
    stg.off[4] = wave < 6 ? moe_rec_off<MODE>(a, first, nt, 2048 + tid, b16) : (uint32_t) (tid - 384) * 16u;
    stg.offx = NCH > 128 && wave == 0 ? (uint32_t) (128 + lane) * 16u : 0u; stg.x_on = NCH > 128 && wave == 0 && lane < NCH - 128;
    if (wave == 1) stg.offx = moe_rec_off<MODE>(a, first, nt, lane * BAMD_B16_Q, b16) + (uint32_t) nb * BAMD_B16_REC;
    const uint8_t * chb = ch + (size_t) rb * nb * (4 * F::CHRT);
    auto stage = [&](int ci, int b) { stg.issue(a.blob16 + (size_t) ci * BAMD_B16_REC, chb + (size_t) ci * (4 * F::CHRT), a.blob16 + (size_t) ci * 4, lds0 + X_BLK0 + (uint32_t) b * X_BLK, wave, lane); };
    // builder (the expert stream's own rows, one record group per wave): wave (rt, q = tp), lane (p = lane >> 5, r = (lane >> 2) & 7, el = lane & 3), as the dense body.
    // nrows is a multiple of 256: every record group exists
    const int bp = lane >> 5, br = (lane >> 2) & 7, bel = lane & 3;
    const uint8_t * w0, * w1; F::lane_ptrs(wex, (size_t) (2 * rtg + tp) * nb * F::RECB, bp, br, bel, w0, w1);
    const uint8_t * phb = ph + (size_t) rb * nb * F::PH_SB + (size_t) rt * F::PH_RT + (size_t) (((2 * bp) * 16 + 8 * tp + br) * (F::PH_RT / 64));
    F f;
    unsigned char * afw = smem + X_AF0 + (rt * 4 + bel) * (2 * X_FR) + ((2 * bp) * 16 + 8 * tp + br) * 16;     // [row tile][e' = 0..3][2 x X_FR]: MFMA lane (8 tp + br, 2 bp + j) at + j * 256
    const unsigned char * afr = smem + X_AF0 + rt * 8 * X_FR + lane * 16;
    const unsigned char * tok = smem + X_BLK0 + (size_t) ((2 * tp) * 16 + m) * BAMD_B16_REC;       // this lane's slot record of tile n = 0; n = 1: 16 records on
    const unsigned char * bop = tok + g * 16;
    typename F::Hdr hdr; hdr.init(tok, smem + X_BLK0, rt * F::CHRT, (2 * tp) * 16 + m, g);
    bamd_f4 acc[2][8];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[n][e] = (bamd_f4) { 0.f, 0.f, 0.f, 0.f };
    }
    stage(0, 0);
    f.template load_set<0>(0, w0, w1, phb, bp);
    f.template load_set<1>(1, w0, w1, phb, bp);
#pragma unroll
    for (int j = 0; j < 2; ++j) { f.build_a(0, j); f.build_b(0, j, afw + j * 256); }
    lds_dma_wait();
    __syncthreads();
    const int nhs = 2 * nb;
    // the K loop with NL live slot tiles of this wave (a tile whose first slot is at or past nt is dead: its slots are never stored).  NL is a compile-time
    // constant of three copies of the loop, chosen once per wave below, so that the full copy is the dense body's straight-line half step.  What a wave does for
    // the others — staging, the weight loads, the fragment build — and every barrier stand in all three copies alike; what is gone from a dead tile are its B
    // operand reads, its MFMAs and its chain, and with NL = 0 the A fragment and header reads too.
    auto run = [&](auto nl_tag) {
        constexpr int NL = decltype(nl_tag)::value;
        // half step hs = 2 ci + H: fragments in ring slot H, activation block ci & 1 = BLK
        auto step = [&](const int hs, auto h_tag, auto blk_tag) {
            constexpr int H = decltype(h_tag)::value, BLK = decltype(blk_tag)::value, NXT = H ^ 1;
            const int ci = hs >> 1;
            // both clamped at the end of K: an expert's side table and stream have nothing of their own behind them (no slack: x_slack, bamd_prefill2.hip)
            if (H == 0) stage(ci + 1 < nb ? ci + 1 : nb - 1, BLK ^ 1);                             // the next super-block's records: a whole step ahead
            f.template load_set<H>(hs + 2 < nhs ? hs + 2 : nhs - 2 + H, w0, w1, phb, bp);
            __builtin_amdgcn_sched_barrier(0);
            float D[2][4];
            if (NL > 0) hdr.read(BLK, H, D);
            bamd_h8 Aq[2][F::NFRAG], Bq[2][2]; bamd_f4 sp[2];
            auto load_ops = [&](int e) {                           // A fragments and B operands of e, double-buffered
                if (NL > 0) {
#pragma unroll
                    for (int p = 0; p < F::NFRAG; ++p) Aq[e & 1][p] = *(const bamd_h8 *) (afr + H * X_AF_BYTES + e * (2 * X_FR) + p * X_FR);
                }
#pragma unroll
                for (int n = 0; n < NL; ++n) Bq[e & 1][n] = *(const bamd_h8 *) (bop + BLK * X_BLK + n * (16 * BAMD_B16_REC) + (4 * H + e) * 64);
            };
            auto chain = [&](int e, int n, const bamd_f4 & s) {
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[n][4 * H + e][i] = fmaf(D[n][i], s[i], hdr.mins(acc[n][4 * H + e][i], n, e, i));
            };
            load_ops(0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (e + 1 < 4) load_ops(e + 1);
                if ((e & 1) == 0) f.build_a(NXT, e >> 1);
                bamd_f4 s[2];
#pragma unroll
                for (int n = 0; n < NL; ++n) {                     // NFRAG MFMAs chained through the accumulator: the exact integer isum_e of the tile
                    s[n] = (bamd_f4) { 0.f, 0.f, 0.f, 0.f };
#pragma unroll
                    for (int p = 0; p < F::NFRAG; ++p) s[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Aq[e & 1][p], Bq[e & 1][n], s[n], 0, 0, 0);
                    if (!F::LATE_CHAIN) chain(e, n, s[n]);
                }
                if (F::LATE_CHAIN && e > 0) {
#pragma unroll
                    for (int n = 0; n < NL; ++n) chain(e - 1, n, sp[n]);
                }
                if (e & 1) f.build_b(NXT, e >> 1, afw + NXT * X_AF_BYTES + (e >> 1) * 256);
#pragma unroll
                for (int n = 0; n < NL; ++n) sp[n] = s[n];
                __builtin_amdgcn_sched_barrier(0);
            }
            if (F::LATE_CHAIN) {
#pragma unroll
                for (int n = 0; n < NL; ++n) chain(3, n, sp[n]);
            }
            if (H == 1) lds_dma_wait();
            __syncthreads();
        };
        for (int ci = 0; ci < nb; ci += 2) {
            step(2 * ci, std::integral_constant<int, 0>(), std::integral_constant<int, 0>());
            step(2 * ci + 1, std::integral_constant<int, 1>(), std::integral_constant<int, 0>());
            if (ci + 1 < nb) {
                step(2 * ci + 2, std::integral_constant<int, 0>(), std::integral_constant<int, 1>());
                step(2 * ci + 3, std::integral_constant<int, 1>(), std::integral_constant<int, 1>());
            }
        }
    };
    const int u0 = (2 * tp) * 16;                                  // the wave's first slot; nt and tp are wave-uniform (scalar registers)
    if (u0 + 16 < nt) run(std::integral_constant<int, 2>());
    else if (u0 < nt) run(std::integral_constant<int, 1>());
    else              run(std::integral_constant<int, 0>());
    // hsum_float_8 over e, then rows 4g .. 4g+3 of the slot's pair
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int u = u0 + n * 16 + m;
        if (u >= nt) continue;
        float val[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) val[i] = x_hsum8(acc[n], i);
        moe_store<MODE>(a, moe_pair(a, first, nt, u), rtg * 16 + 4 * g, val);
    }
}

// ---- host side, per policy -----------------------------------------------------------------------------------------------------------------------
template <class F>
static void moe_mfma2_launch(const bamd_moe_mma_args & a, int mode, int tile_bound, hipStream_t s) {
    const dim3 grid(tile_bound, a.nrows / 64);
    with_const(consts<MOE_GATE, MOE_UP, MOE_DOWN>(), mode, [&](auto M) -> bool {
        auto kernel = moe_mfma2_kernel<decltype(M)::value, F>;
        bamd_allow_lds(kernel, X_LDS_BYTES);
        hipLaunchKernelGGL(kernel, grid, dim3(512), X_LDS_BYTES, s, a);
        return true; });
}
template <class F>
static int moe_mfma2_supported(void) {
    return hipFuncSetAttribute((const void *) moe_mfma2_kernel<MOE_GATE, F>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) X_LDS_BYTES) == hipSuccess &&
           hipFuncSetAttribute((const void *) moe_mfma2_kernel<MOE_UP, F>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) X_LDS_BYTES) == hipSuccess &&
           hipFuncSetAttribute((const void *) moe_mfma2_kernel<MOE_DOWN, F>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) X_LDS_BYTES) == hipSuccess;
}
