// bamd_prefill2_body.h — what the matrix-core prompt mat-mul kernels with fragments built once per workgroup share (bamd_prefill2.hip: Q4_K / Q5_K / Q6_K / Q3_K / Q2_K;
// bamd_prefill2_xs.hip: IQ4_XS, a translation unit of its own): the launch arguments, the LDS map, the activation / header stage, the hsum tree, the consumer
// header X2Hdr and the eight-wave kernel body matmul_mfma2_kernel<EPI, F>, which a policy struct F per format completes.  The design: bamd_prefill2.hip's head.
#pragma once
#include "bamd_device.h"
#include "bamd_mfma_common.h"
#include "bamd_mv_select.h"
#include "bamd_prefill_family.h"
#include <type_traits>
#include <stdlib.h>

typedef _Float16 bamd_h2 __attribute__((ext_vector_type(2)));
union bamd_h2u { uint32_t u; bamd_h2 h; };

struct bamd_mma2_args {
    const uint8_t * w;               // wave-stream records of the matrix (bamd_formats.h)
    const uint8_t * ph;              // prefill aux, builder part:  [row block of 64][super-block]([e-half], Q6_K)[4 row tiles][64 MFMA lanes][16 B]
    const uint8_t * ch;              // prefill aux, consumer part: [row block of 64][super-block][4 row tiles][X_CH_RT B]
    float * out; const float * res;  // [T][ldo]
    const uint8_t * blob16;          // f16 activation records (quantize_batch_kernel)
    int K, T, nrows, nrows_pad, ldo;
    unsigned long long * dbg;        // -DX_TIMING builds: per-wave phase clocks of workgroup (0, 0) (tools/prefill_phase.py); else unused
};

// LDS map (byte offsets).  Both copies of every region lie within 64 KiB of the region's first copy, so one base register per region
// serves both buffers through the 16-bit offset field of the DS instructions (the buffer in use is a compile-time parity of the step).
#define X_FR 1040                                          /* bytes between fragments: 1 KiB + 16 — the builder's 16-byte stores of eight lanes (one row, e = 0..7) then fall on eight
                                                              different bank quads (260 dwords = 4 mod 64); a fragment itself stays contiguous (lane * 16) for the consumers' ds_read_b128 */
#define X_AF_BYTES (32 * X_FR)                             /* A fragments of one super-block: 4 row tiles x 8 fragments */
#define X_BS_BYTES (64 * BAMD_B16_REC)                     /* 64 token records of one super-block (38 912 B) */
#define X_CH4_RT 640                                       /* Q4_K / Q5_K consumer header of a row tile: 16 x d f32 | 16 x dmin f32 | 16 x 4 x 8 B of min operands */
#define X_CH6_RT 64                                        /* Q6_K: 16 x d f32 */
#define X_CH_MAX (4 * X_CH4_RT)
#define X3_CHS 3072                                        /* Q4_K / Q5_K consumer headers of a row block and super-block in the side table: 4 x 640 B, padded to three DMA instructions */
#define X_BLK (X_BS_BYTES + X_CH_MAX + 256 + 32)           /* records | headers | 64 d_y | 32 bytes of zeros: 41 760 B */
#define X_AF0 0
#define X_BLK0 (2 * X_AF_BYTES)
#define X_LDS_BYTES (X_BLK0 + 2 * X_BLK)                   /* 149 056 B */
#define X_CH_OFF X_BS_BYTES
#define X_YD_OFF (X_BS_BYTES + X_CH_MAX)
#define X_Z_OFF (X_YD_OFF + 256)

// ---- the activation / header stage: global -> LDS by DMA --------------------------------------------------------------------------
// chunk list of a step (16 B each): 2432 chunks of token records (64 tokens x 38), then the NCH chunks of the row block's consumer headers;
// wave-instruction k = 64 consecutive chunks; round r: instruction 8 r + wave.  Rounds 0..3 (and round 4 for waves 0..5) are records; round
// 4 of waves 6, 7 and the tail instructions are headers (NCH = 160 for Q4_K / Q5_K: a half instruction on wave 0; 16 for Q6_K: lanes 0..15 of
// wave 6); the 64 block scales d_y go as one 4-byte instruction on wave 1.
// byte offset into blob16 of record chunk idx of a token tile (token idx / 38 of the tile at t0, its chunk idx % 38); tokens past T read the last one
__device__ inline uint32_t x_rec_off(int idx, int t0, int T, size_t b16) {
    const int tok = idx / BAMD_B16_Q, q = idx - tok * BAMD_B16_Q; const int tg = t0 + tok < T ? t0 + tok : T - 1; return (uint32_t) ((size_t) tg * b16 + (size_t) q * 16);
}
template <int NCH>
struct XStage {
    uint32_t off[5]; uint32_t offx; bool x_on;
    __device__ __forceinline__ void plan(int tid, int wave, int lane, int t0, int T, size_t b16, int nb) {
        auto rec_off = [&](int idx) { return x_rec_off(idx, t0, T, b16); };
#pragma unroll
        for (int r = 0; r < 4; ++r) off[r] = rec_off(r * 512 + tid);
        off[4] = wave < 6 ? rec_off(2048 + tid) : (uint32_t) (tid - 384) * 16u;
        if (NCH > 128) { offx = wave == 0 ? (uint32_t) (128 + lane) * 16u : 0u; x_on = wave == 0 && lane < NCH - 128; } else { offx = 0u; x_on = false; }
        if (wave == 1) { const int tg = t0 + lane < T ? t0 + lane : T - 1; offx = (uint32_t) ((size_t) tg * b16 + (size_t) nb * BAMD_B16_REC); }
    }
    // recs = blob16 + ci * BAMD_B16_REC, hdrs = headers of (row block, ci), yds = blob16 + ci * 4; blk = LDS byte address of the block to fill
    __device__ __forceinline__ void issue(const uint8_t * recs, const uint8_t * hdrs, const uint8_t * yds, uint32_t blk, int wave, int lane) const {
        const uint32_t wdst = blk + (uint32_t) wave * 1024u;
#pragma unroll
        for (int r = 0; r < 4; ++r) lds_dma16_s(recs, off[r], wdst + (uint32_t) r * 8192u);
        if (wave < 6) lds_dma16_s(recs, off[4], wdst + 32768u);
        else if (NCH >= 128 || (wave == 6 && lane < NCH)) lds_dma16_s(hdrs, off[4], wdst + 32768u);
        if (NCH > 128 && x_on) lds_dma16_s(hdrs, offx, blk + X_CH_OFF + 2048u);
        if (wave == 1) lds_dma4_s(yds, offx, blk + X_YD_OFF);
    }
};

// ---- the reference's hsum_float_8 tree over the eight per-e accumulators of an output (component i of a 16 x 16 tile's lane), for both layouts
__device__ __forceinline__ float x_hsum8(const bamd_f4 (&acc)[8], int i) {
    return ((acc[0][i] + acc[4][i]) + (acc[2][i] + acc[6][i])) + ((acc[1][i] + acc[5][i]) + (acc[3][i] + acc[7][i]));
}

// ==== eight waves: ONE kernel body (matmul_mfma2_kernel, behind the policies) and a policy struct F per format ===============================================
// What the body asks of F: the sizes RECB (record), CHRT (consumer header of a row tile), PH_SB (builder operands of a row block and super-block: two half steps x
// 4 row tiles x 64 MFMA lanes; one set for both half steps where the scales do not depend on the e-half: X2IQ4XS) and PH_RT (those of one row tile), NFRAG
// (fragments = MFMAs per (e, token tile)), LATE_CHAIN (the chain FMAs of e behind the MFMAs of e + 1 instead of behind its own),
// Hdr (the consumer header values of a half step and the min term: X2Hdr, below), lane_ptrs (the builder lane's two pointers into its record group),
// and the registers of two weight sets with load_set<S>(hs, the two pointers, the lane's builder operands, bp), build_a(S, j), build_b(S, j, dst).
// Three things in this cut are there because the Q3_K / Q2_K and the sixteen-wave instances then compile to the code objects they had as separate kernels
// (profiles/prefill2_unify.txt): the lane's pointers are three locals of the body, not members of F (as members of one struct the prologue's address arithmetic
// is scheduled differently); D is a local of the step that Hdr fills; and the row-of-four store stands in each kernel, not in a shared function (inlined from
// one, the loop's phi nodes and with them the register assignment change).

// the consumer side's header values of a half step: D = d_y d of the lane's rows 4g + i and two tokens n; MINS (Q2_K): Dm = -d_y dmin, {mins[2e], mins[2e+1]} of the
// rows and {bsum16[2e], bsum16[2e+1]} of the tokens, e = 4 H + 0..3.  chain() is one link of acc_e: the min term first, into the same accumulator
template <bool MINS>
struct X2Hdr {
    const unsigned char * tok, * chd, * chm, * ydp;
    float Dm[2][4]; bamd_h2u mn[4][4], bs[2][4];
    // tok_: the lane's token record of tile n = 0 (token tl of the block) in LDS block 0 (blk), rto: byte offset of the row tile's consumer header (16 x d | 16 x dmin | 16 rows x 16 mins)
    __device__ __forceinline__ void init(const unsigned char * tok_, const unsigned char * blk, int rto, int tl, int g) {
        tok = tok_;
        chd = blk + X_CH_OFF + rto + g * 16;                   // d of rows 4g .. 4g+3 (MINS: their dmin 64 bytes on)
        chm = blk + X_CH_OFF + rto + 128 + g * 128;            // MINS: the mins of rows 4g .. 4g+3, 32 bytes each
        ydp = blk + X_YD_OFF + tl * 4;
    }
    __device__ __forceinline__ void read(int BLK, int H, float (&D)[2][4]) {
        const bamd_f4 dw = *(const bamd_f4 *) (chd + BLK * X_BLK);
        bamd_f4 dmw = { 0.f, 0.f, 0.f, 0.f };
        if (MINS) dmw = *(const bamd_f4 *) (chd + BLK * X_BLK + 64);
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const float ydv = *(const float *) (ydp + BLK * X_BLK + n * 64);
#pragma unroll
            for (int i = 0; i < 4; ++i) { D[n][i] = ydv * dw[i]; if (MINS) Dm[n][i] = (-ydv) * dmw[i]; }
            if (MINS) { const uint4 b = *(const uint4 *) (tok + BLK * X_BLK + n * (16 * BAMD_B16_REC) + 576 + 16 * H); bs[n][0].u = b.x; bs[n][1].u = b.y; bs[n][2].u = b.z; bs[n][3].u = b.w; }
        }
        if (MINS) {
#pragma unroll
            for (int i = 0; i < 4; ++i) { const uint4 v = *(const uint4 *) (chm + BLK * X_BLK + i * 32 + 16 * H); mn[i][0].u = v.x; mn[i][1].u = v.y; mn[i][2].u = v.z; mn[i][3].u = v.w; }
        }
    }
    __device__ __forceinline__ float mins(float av, int n, int e, int i) const {
        if (MINS) av = fmaf(Dm[n][i], __builtin_amdgcn_fdot2(mn[i][e].h, bs[n][e].h, 0.f, false), av);
        return av;
    }
};

// ---- the eight-wave body: a workgroup of 64 rows x 64 tokens, wave (rt, tp) = row tile rt x token tiles 2 tp, 2 tp + 1.  A step is HALF a super-block (four e);
//      the fragment ring holds two half steps x 4 row tiles x 4 e x 2 fragment slots (the second one unused where NFRAG = 1), the activation stage (whole
//      super-blocks) is refilled every second half step
template <int EPI, class F>
__global__ void __launch_bounds__(512) matmul_mfma2_kernel(bamd_mma2_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id(), m = lane & 15, g = lane >> 4;
    const int rt = wave >> 1, tp = wave & 1;
    const int nb = a.K >> 8;
    const int rb = blockIdx.y, t0 = blockIdx.x * 64;
    const int rtg = rb * 4 + rt;
    const bool live = rtg * 16 < a.nrows_pad;
    const size_t b16 = BAMD_BLOB16_BYTES(nb);
    const uint32_t lds0 = (uint32_t) (size_t) (bamd_lds_vp) smem;
    XStage<4 * F::CHRT / 16> stg; stg.plan(tid, wave, lane, t0, a.T, b16, nb);
    const uint8_t * chb = a.ch + (size_t) rb * nb * (4 * F::CHRT);
    auto stage = [&](int ci, int b) { stg.issue(a.blob16 + (size_t) ci * BAMD_B16_REC, chb + (size_t) ci * (4 * F::CHRT), a.blob16 + (size_t) ci * 4, lds0 + X_BLK0 + (uint32_t) b * X_BLK, wave, lane); };
    // builder (the stream's own rows, one record group per wave): wave (rt, q = tp), lane (p = lane >> 5, r = (lane >> 2) & 7, el = lane & 3) takes, per half step, chunk
    // e = 4 H + el of row 8q + r and builds the pieces of MFMA lanes (8q + r, g = 2p + j), j = 0, 1, of fragment e.  Eight consecutive lanes = two rows x four
    // fragments: their 16-byte stores fall on eight different bank quads (fragment pairs 2 x X_FR bytes apart).
    const int bp = lane >> 5, br = (lane >> 2) & 7, bel = lane & 3;
    const int rgq = 2 * (live ? rtg : rb * 4) + tp;
    const int rgc = rgq * 8 < a.nrows_pad ? rgq : rgq - 1;            // a last tile of 8 (padded) rows: its first record group twice (rows 8..15 are never stored)
    const uint8_t * w0, * w1; F::lane_ptrs(a.w, (size_t) rgc * nb * F::RECB, bp, br, bel, w0, w1);
    // builder operands: [row block][super-block]([e-half], where the scales differ between the halves)[4 row tiles (PH_RT bytes each)][64 MFMA lanes (PH_RT / 64 bytes each)]
    const uint8_t * phb = a.ph + (size_t) rb * nb * F::PH_SB + (size_t) rt * F::PH_RT + (size_t) (((2 * bp) * 16 + 8 * tp + br) * (F::PH_RT / 64));
    F f;
    unsigned char * afw = smem + X_AF0 + (rt * 4 + bel) * (2 * X_FR) + ((2 * bp) * 16 + 8 * tp + br) * 16;     // [row tile][e' = 0..3][2 x X_FR]: MFMA lane (8 tp + br, 2 bp + j) at + j * 256
    const unsigned char * afr = smem + X_AF0 + rt * 8 * X_FR + lane * 16;
    const unsigned char * tok = smem + X_BLK0 + (size_t) ((2 * tp) * 16 + m) * BAMD_B16_REC;       // this lane's token record of tile n = 0; n = 1: 16 records on
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
    // half step hs = 2 ci + H: fragments in ring slot H, activation block ci & 1 = BLK
    auto step = [&](const int hs, auto h_tag, auto blk_tag) {
        constexpr int H = decltype(h_tag)::value, BLK = decltype(blk_tag)::value, NXT = H ^ 1;
        const int ci = hs >> 1;
        if (H == 0) stage(ci + 1 < nb ? ci + 1 : nb - 1, BLK ^ 1);                                 // the next super-block's records: a whole step ahead
        f.template load_set<H>(hs + 2 < nhs ? hs + 2 : nhs - 2 + H, w0, w1, phb, bp);
        __builtin_amdgcn_sched_barrier(0);
        float D[2][4];
        hdr.read(BLK, H, D);
        bamd_h8 Aq[2][F::NFRAG], Bq[2][2]; bamd_f4 sp[2];
        auto load_ops = [&](int e) {                           // A fragments and B operands of e, double-buffered
#pragma unroll
            for (int p = 0; p < F::NFRAG; ++p) Aq[e & 1][p] = *(const bamd_h8 *) (afr + H * X_AF_BYTES + e * (2 * X_FR) + p * X_FR);
#pragma unroll
            for (int n = 0; n < 2; ++n) Bq[e & 1][n] = *(const bamd_h8 *) (bop + BLK * X_BLK + n * (16 * BAMD_B16_REC) + (4 * H + e) * 64);
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
            for (int n = 0; n < 2; ++n) {                      // NFRAG MFMAs chained through the accumulator: the exact integer isum_e of the tile
                s[n] = (bamd_f4) { 0.f, 0.f, 0.f, 0.f };
#pragma unroll
                for (int p = 0; p < F::NFRAG; ++p) s[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Aq[e & 1][p], Bq[e & 1][n], s[n], 0, 0, 0);
                if (!F::LATE_CHAIN) chain(e, n, s[n]);
            }
            if (F::LATE_CHAIN && e > 0) { chain(e - 1, 0, sp[0]); chain(e - 1, 1, sp[1]); }
            if (e & 1) f.build_b(NXT, e >> 1, afw + NXT * X_AF_BYTES + (e >> 1) * 256);
            sp[0] = s[0]; sp[1] = s[1];
            __builtin_amdgcn_sched_barrier(0);
        }
        if (F::LATE_CHAIN) { chain(3, 0, sp[0]); chain(3, 1, sp[1]); }
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
    if (!live) return;
    // hsum_float_8 over e, then rows 4g .. 4g+3 of token t — 16 consecutive bytes — as one 16-byte access where all four exist and the token rows are 16-byte aligned,
    // else one by one
    const int row0 = rtg * 16 + 4 * g;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int t = t0 + (2 * tp + n) * 16 + m;
        float val[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) val[i] = x_hsum8(acc[n], i);
        if (t < a.T && row0 < a.nrows) {
            const size_t o = (size_t) t * a.ldo + row0;
            if (row0 + 3 < a.nrows && (a.ldo & 3) == 0) {
                bamd_f4 y = { val[0], val[1], val[2], val[3] };
                if (EPI != BAMD_EPI_STORE) {
                    const bamd_f4 r = *(const bamd_f4 *) (a.res + o);
#pragma unroll
                    for (int i = 0; i < 4; ++i) y[i] = EPI == BAMD_EPI_ADD ? val[i] + r[i] : v_silu(r[i]) * val[i];
                }
                *(bamd_f4 *) (a.out + o) = y;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (row0 + i < a.nrows) a.out[o + i] = EPI == BAMD_EPI_ADD ? val[i] + a.res[o + i] : EPI == BAMD_EPI_SILU_MUL ? v_silu(a.res[o + i]) * val[i] : val[i];
            }
        }
    }
}
