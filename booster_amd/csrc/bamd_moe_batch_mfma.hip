// bamd_moe_batch_mfma.hip — the grouped, gathered expert mat-muls of a mixture-of-experts prompt micro-batch on the matrix cores, behind the switch BAMD_PREFILL_MOE /
// bamd_set_prefill_moe (default off: bamd_prefill_family.cpp): launches 4 and 6 of bamd_moe_batch.hip with the arithmetic of bamd_prefill2.hip, bit-identical per
// (row, pair) to the grouped integer-dot kernel (moe_group_mm_kernel), and so to the routed decode launches and to llm_build_moe_ffn.  Expert types Q4_K, Q5_K, Q6_K
// here; while their own family switch is on as well, Q3_K / Q2_K / IQ4_XS in bamd_moe_batch_kq_mfma.hip / bamd_moe_batch_xs_mfma.hip (the dense eight-wave body under
// its policies, with dead slot tiles skipped) and Q8_0 / Q4_0 / Q5_0 / Q4_1 / Q5_1 / IQ4_NL in bamd_moe_batch_b32_mfma.hip (the arithmetic of bamd_prefill2_b32.hip).
// The host side below routes PER TENSOR: gate / up and down pick their kernel independently and read one tile table (bamd_moe_batch_mfma.h: arguments, bounded reads).
//   * A tile is 64 weight rows x up to 64 pairs (token, slot) of ONE expert: moe_group_kernel run with tt = 64 writes the pair lists and the tile table.  Grid
//     (tile bound T n_used / 64 + n_expert, row blocks of 64); the tiles of an expert are adjacent in blockIdx.x, so the workgroups that build fragments from the
//     same expert rows run together and meet in L2.  A workgroup whose tile index is past tiles[0] exits before its first barrier; what the table and the lists
//     hold is bounded again where it becomes an address.  Rows (F for gate / up, E for down) are multiples of 256: there is no partial row block.
//   * Weights base + expert x stride, side table aux + expert x aux stride (one table of bamd_prefill_aux_bytes per expert, built by bamd_launch_prefill_aux).
//   * Activations: the 608-byte f16 records of bamd_launch_quantize_batch's blob16, global -> LDS by the per-lane DMA of the dense kernels; the lane's source
//     offset comes from the pair list instead of t0 + lane: gate / up read the record row of the pair's TOKEN (pair / n_used), down the pair's own row of h.
//     Slots past the tile's count read the tile's last pair again and are never stored.  Pair ids live in registers only.
//   * Epilogues scattered by pair id: gate stores h[pair]; up stores silu(h[pair]) x value in place (every lane reads and writes its own four elements);
//     down stores value x w[pair], rounded before any add (ggml_mul), to prod[pair] — moe_combine_kernel follows unchanged.
//   * Two kernel shapes, as the dense path: sixteen waves with one 16 x 16 tile each for Q4_K / Q5_K (the step of matmul_mfma3_q4k_kernel), eight waves with 16 x 32
//     each for Q6_K (the half step of matmul_mfma2_kernel under X2Q6K: split scale, two chained MFMAs).  The bodies are written out here, not shared: the dense
//     kernels keep the code objects they have (profiles/moe_batch_mfma_codeobj.txt).  What is shared are the headers' helpers: the LDS map, XStage's issue, X2Hdr,
//     x_hsum8, the DMA wrappers; moe_rec_off and moe_store (bamd_moe_batch_mfma.h) serve the eight-wave kernels of the other files as well.
#include "bamd_prefill2_body.h"
#include "bamd_moe_batch_mfma.h"

// ==== sixteen waves, Q4_K / Q5_K: the LDS map, staging plan, builder and step of matmul_mfma3_q4k_kernel (bamd_prefill2.hip has the reasons) ======================
#define X3_BLK (X_BS_BYTES + X3_CHS + 4096 + 32)           /* records (38 KiB) | headers (3 KiB) | operands (4 KiB) | 32 bytes of zeros: 46 112 B */
#define X3_BLK0 (2 * X_AF_BYTES)
#define X3_LDS_BYTES (X3_BLK0 + 2 * X3_BLK)                /* 158 784 B */
#define X3_CH_OFF X_BS_BYTES
#define X3_PH_OFF (X_BS_BYTES + X3_CHS)
#define X3_Z_OFF (X3_PH_OFF + 4096)
template <int MODE, bool Q5>
__global__ void __launch_bounds__(1024) moe_mfma3_q4k_kernel(bamd_moe_mma_args a) {
    constexpr uint32_t RECB = Q5 ? BAMD_RECB_Q5K : BAMD_RECB_Q4K;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int ex, first, nt;
    if (!moe_tile(a, blockIdx.x, ex, first, nt)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id(), m = lane & 15, g = lane >> 4;
    const int rt = wave >> 2, tt = wave & 3;
    const int nb = a.K >> 8;
    const int rb = blockIdx.y, rtg = rb * 4 + rt;
    const size_t b16 = BAMD_BLOB16_BYTES(nb);
    const uint8_t * wex = a.w + (size_t) ex * a.wstride, * ph = a.aux + (size_t) ex * a.astride, * ch = ph + a.ch_off;
    const uint32_t lds0 = (uint32_t) (size_t) (bamd_lds_vp) smem;
    // ---- stage plan.  A block = 45 KiB-instructions: k = 0..37 records (chunk 64 k + lane of 64 slots x 38), 38..40 consumer headers, 41..44 builder
    //      operands.  Wave w issues k = w, 16 + w and k2 = 32 + w (w <= 12; waves 13..15 repeat the operand copies 41..43: same bytes, same place).
    auto rec_off = [&](int idx) { return moe_rec_off<MODE>(a, first, nt, idx, b16); };
    const int k2 = wave <= 12 ? 32 + wave : 28 + wave;
    const bool rec2 = k2 <= 37, hdr2 = k2 >= 38 && k2 <= 40;
    uint32_t so0 = rec_off(tid), so1 = rec_off(1024 + tid);          // advance by one super-block per step (sources stay fixed scalar pointers)
    uint32_t so2 = rec2 ? rec_off(k2 * 64 + lane) : (uint32_t) (((hdr2 ? k2 - 38 : k2 - 41) * 64 + lane) * 16);
    const uint8_t * p01 = a.blob16;
    const uint8_t * p2 = rec2 ? a.blob16 : hdr2 ? ch + (size_t) rb * nb * X3_CHS : ph + (size_t) rb * nb * 4096 + 4096;
    const uint32_t st2 = rec2 ? (uint32_t) BAMD_B16_REC : hdr2 ? (uint32_t) X3_CHS : 4096u;
    // destinations by the parity of the step that issues the copies: records / headers of ci + 1 -> the OTHER block, operands of ci + 2 -> the block in use
    const uint32_t blk_a = lds0 + X3_BLK0, blk_b = blk_a + X3_BLK;
    const uint32_t d0_even = blk_b + (uint32_t) wave * 1024u, d0_odd = blk_a + (uint32_t) wave * 1024u;
    const uint32_t d2_even = (k2 <= 40 ? blk_b : blk_a) + (uint32_t) k2 * 1024u, d2_odd = (k2 <= 40 ? blk_a : blk_b) + (uint32_t) k2 * 1024u;
    // ---- builder: wave (rt, tt) = record group q = tt & 1 of the row tile, pieces g = 2 gh + j (gh = tt >> 1, j = 0, 1): lane (r, e) holds dwords 2 gh, 2 gh + 1
    //      of stream lane (r, e) = the halves of MFMA lanes (8 q + r, 2 gh + j) of fragment e
    const int br = lane >> 3, be = lane & 7, bq = tt & 1, gh = tt >> 1;
    const int rgq = 2 * rtg + bq;
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc((void *) uniform_ptr(wex + (size_t) rgq * nb * RECB), 0, 0x7fffffff, 0x00020000);
    const int vraw = lane * 16 + gh * 8, vqh = 1024 + lane * 4;
    uint2 raw[2]; uint32_t qh[2];
    auto load_set = [&](int ci, auto set_tag) {
        constexpr int S = decltype(set_tag)::value;
        const u32x2_t v = __builtin_amdgcn_raw_buffer_load_b64(wrs, vraw, ci * (int) RECB, 0); raw[S] = make_uint2(v.x, v.y);
        if (Q5) qh[S] = __builtin_amdgcn_raw_buffer_load_b32(wrs, vqh, ci * (int) RECB, 0);
    };
    bamd_h2u c0, c1, c2, c3;
    const uint32_t qs0 = 4u * (uint32_t) gh;
    auto build_a = [&](uint32_t wq, uint32_t q, int j) {
        uint32_t lo = wq & 0x0f0f0f0fu, hi = Q5 ? (wq >> 4) & 0x0f0f0f0fu : wq & 0xf0f0f0f0u;      // Q4_K: the high nibbles stay in place (16 n; the scale operand is s / 16)
        if (Q5) { lo |= ((q >> (qs0 + 2 * j)) & 0x01010101u) << 4; hi |= ((q >> (qs0 + 2 * j + 1)) & 0x01010101u) << 4; }
        c0.u = __builtin_amdgcn_perm(0x64646464u, lo, 0x04010400u); c1.u = __builtin_amdgcn_perm(0x64646464u, lo, 0x04030402u);
        c2.u = __builtin_amdgcn_perm(0x64646464u, hi, 0x04010400u); c3.u = __builtin_amdgcn_perm(0x64646464u, hi, 0x04030402u);
    };
    auto build_b = [&](const uint4 & s, unsigned char * dst) {
        bamd_h2u s0, n0, s1, n1, a0, a1, a2, a3; s0.u = s.x; n0.u = s.y; s1.u = s.z; n1.u = s.w;
        a0.h = __builtin_elementwise_fma(c0.h, s0.h, n0.h); a1.h = __builtin_elementwise_fma(c1.h, s0.h, n0.h);     // (1024 + n) s - 1024 s = n s, one rounding, exact
        a2.h = __builtin_elementwise_fma(c2.h, s1.h, n1.h); a3.h = __builtin_elementwise_fma(c3.h, s1.h, n1.h);
        *(uint4 *) dst = (uint4) { a0.u, a1.u, a2.u, a3.u };
    };
    // per-lane LDS addresses (first copy of each region)
    unsigned char * afw = smem + X_AF0 + (rt * 8 + be) * X_FR + ((2 * gh) * 16 + 8 * bq + br) * 16;
    const unsigned char * afr = smem + X_AF0 + rt * 8 * X_FR + lane * 16;
    const unsigned char * phl = smem + X3_BLK0 + X3_PH_OFF + rt * 1024 + (2 * gh) * 256 + (8 * bq + br) * 16;
    const unsigned char * tok = smem + X3_BLK0 + (size_t) (tt * 16 + m) * BAMD_B16_REC;                  // this lane's slot record
    const unsigned char * bop = tok + g * 16;
    const unsigned char * bmn = tok + 512 + (Q5 ? g * 8 : 0);
    const unsigned char * chd = smem + X3_BLK0 + X3_CH_OFF + rt * X_CH4_RT + g * 16;                // d of rows 4g .. 4g+3; their dmin 64 bytes on
    const unsigned char * cmn = Q5 ? smem + X3_BLK0 + X3_CH_OFF + rt * X_CH4_RT + 128 + m * 32 + g * 8
                                   : (g == 0 ? smem + X3_BLK0 + X3_CH_OFF + rt * X_CH4_RT + 128 + m * 32 : smem + X3_BLK0 + X3_Z_OFF);
    bamd_f4 acc[8], accm[4];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = (bamd_f4) { 0.f, 0.f, 0.f, 0.f };
#pragma unroll
    for (int l = 0; l < 4; ++l) accm[l] = (bamd_f4) { 0.f, 0.f, 0.f, 0.f };
    // prologue = the staging half of a step "-1" of odd parity: records / headers of super-block 0 into block a, operands of super-block 1 into block b;
    // the fragments of super-block 0 are built with operands straight from memory
    if (tid < 16) *(uint32_t *) (smem + X3_BLK0 + X3_Z_OFF + (tid >> 3) * X3_BLK + (tid & 7) * 4) = 0u;
    lds_dma16_s(p01, so0, d0_odd); lds_dma16_s(p01, so1, d0_odd + 16384u); lds_dma16_s(p2, so2, d2_odd);
    so0 += BAMD_B16_REC; so1 += BAMD_B16_REC; so2 += st2;
    load_set(0, std::integral_constant<int, 0>());
    load_set(1, std::integral_constant<int, 1>());               // (no clamping at the end of K: the expert streams are allocated with 4 KiB of slack, as the dense ones)
    {
        const uint8_t * p0 = ph + (size_t) rb * nb * 4096 + (size_t) rt * 1024 + (size_t) ((2 * gh) * 256 + (8 * bq + br) * 16);
        const uint4 s0 = *(const uint4 *) p0, s1 = *(const uint4 *) (p0 + 256);
        build_a(raw[0].x, Q5 ? qh[0] : 0u, 0); build_b(s0, afw);
        build_a(raw[0].y, Q5 ? qh[0] : 0u, 1); build_b(s1, afw + 256);
    }
    lds_dma_wait();
    __syncthreads();
    auto step = [&](const int ci, auto cur_tag) {
        constexpr int CUR = decltype(cur_tag)::value, NXT = CUR ^ 1;
        float D[4], Dm[4];
        const bamd_f4 h0 = *(const bamd_f4 *) (chd + CUR * X3_BLK), h1 = *(const bamd_f4 *) (chd + CUR * X3_BLK + 64);
        const float ydv = *(const float *) (tok + CUR * X3_BLK + 560);
        D[0] = ydv * h0[0]; D[1] = ydv * h0[1]; D[2] = ydv * h0[2]; D[3] = ydv * h0[3];
        Dm[0] = (-ydv) * h1[0]; Dm[1] = (-ydv) * h1[1]; Dm[2] = (-ydv) * h1[2]; Dm[3] = (-ydv) * h1[3];
        {
            // operand reads and MFMAs open the step; the three staging copies and the nibble load follow the MFMAs of e = 0..3 one by one, the fragment pieces of
            // the next super-block are built beside e = 4..7, the chain FMAs of e follow the MFMA of e + 2
            bamd_h8 Aq[3], Bq[3]; bamd_f4 sp[2];
#define X_LDA(e_) (*(const bamd_h8 *) (afr + CUR * X_AF_BYTES + (e_) * X_FR))
#define X_LDB(e_) (*(const bamd_h8 *) (bop + CUR * X3_BLK + (e_) * 64))
            Aq[0] = X_LDA(0); Bq[0] = X_LDB(0); Aq[1] = X_LDA(1); Bq[1] = X_LDB(1);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (e + 2 < 8) { Aq[(e + 2) % 3] = X_LDA(e + 2); Bq[(e + 2) % 3] = X_LDB(e + 2); }
                if (e >= 4 && (e & 1) == 0) build_a(e == 4 ? raw[NXT].x : raw[NXT].y, Q5 ? qh[NXT] : 0u, (e >> 1) & 1);
                const bamd_f4 z = { 0.f, 0.f, 0.f, 0.f };
                const bamd_f4 si = __builtin_amdgcn_mfma_f32_16x16x32_f16(Aq[e % 3], Bq[e % 3], z, 0, 0, 0);
                if (e == 0) lds_dma16_s(p01, so0, CUR ? d0_odd : d0_even);
                if (e == 1) lds_dma16_s(p01, so1, (CUR ? d0_odd : d0_even) + 16384u);
                if (e == 2) { lds_dma16_s(p2, so2, CUR ? d2_odd : d2_even); so0 += BAMD_B16_REC; so1 += BAMD_B16_REC; so2 += st2; }
                if (e == 3) load_set(ci + 2, std::integral_constant<int, CUR>());
                if (e > 1) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[e - 2][i] = fmaf(D[i], sp[e & 1][i], acc[e - 2][i]);
                }
                if (e >= 4 && (e & 1)) build_b(*(const uint4 *) (phl + NXT * X3_BLK + ((e >> 1) & 1) * 256), afw + NXT * X_AF_BYTES + ((e >> 1) & 1) * 256);
                sp[e & 1] = si;
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) { acc[6][i] = fmaf(D[i], sp[0][i], acc[6][i]); acc[7][i] = fmaf(D[i], sp[1][i], acc[7][i]); }
#undef X_LDA
#undef X_LDB
        }
        if (Q5) {
            union { uint2 u; bamd_h4 h; } av, bv; av.u = *(const uint2 *) (cmn + CUR * X3_BLK); bv.u = *(const uint2 *) (bmn + CUR * X3_BLK);
            const bamd_f4 z = { 0.f, 0.f, 0.f, 0.f };
            const bamd_f4 pm = __builtin_amdgcn_mfma_f32_16x16x16f16(av.h, bv.h, z, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) { const float t = Dm[i] * pm[i]; accm[0][i] = accm[0][i] + t; }
        } else {
            const uint4 ma = *(const uint4 *) (cmn + CUR * X3_BLK), mb = *(const uint4 *) (cmn + CUR * X3_BLK + 16);
            const uint4 sfa = *(const uint4 *) (bmn + CUR * X3_BLK), sfb = *(const uint4 *) (bmn + CUR * X3_BLK + 16);
            const uint2 al[4] = { { ma.x, ma.y }, { ma.z, ma.w }, { mb.x, mb.y }, { mb.z, mb.w } };
            const uint2 bl[4] = { { sfa.x, sfa.y }, { sfa.z, sfa.w }, { sfb.x, sfb.y }, { sfb.z, sfb.w } };
            bamd_f4 pm[4];
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                union { uint2 u; bamd_h4 h; } av4, bv4; av4.u = al[l]; bv4.u = bl[l];
                const bamd_f4 z = { 0.f, 0.f, 0.f, 0.f };
                pm[l] = __builtin_amdgcn_mfma_f32_16x16x16f16(av4.h, bv4.h, z, 0, 0, 0);
            }
#pragma unroll
            for (int l = 0; l < 4; ++l) {
#pragma unroll
                for (int i = 0; i < 4; ++i) accm[l][i] = fmaf(Dm[i], pm[l][i], accm[l][i]);
            }
        }
        lds_dma_wait();
        __syncthreads();
    };
    for (int ci = 0; ci < nb; ci += 2) {
        step(ci, std::integral_constant<int, 0>());
        if (ci + 1 < nb) step(ci + 1, std::integral_constant<int, 1>());
    }
    // hsum_float_8 over e and the acc_m folds, in the reference's order (finish_row), then the pair's row of four
    const int u = tt * 16 + m;
    if (u >= nt) return;
    float val[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float v = x_hsum8(acc, i);
        const float mm = Q5 ? accm[0][i] : (accm[0][i] + accm[2][i]) + (accm[1][i] + accm[3][i]);
        val[i] = v + mm;
    }
    moe_store<MODE>(a, moe_pair(a, first, nt, u), rtg * 16 + 4 * g, val);
}

// ==== eight waves, Q6_K: the policy X2Q6K and the half step of matmul_mfma2_kernel ===========================================================================
// scale x (q - 32) reaches 4096: the scale is split sc = sa + sl (prefill_aux_q6k_kernel), both fragments come from one f16 image (1024 + q) - 1056 of the quants
// as v x sa and v x sl (exact), and the two MFMAs of an (e, slot tile) are chained through the accumulator: the exact integer isum
struct MoeQ6K {
    static constexpr uint32_t RECB = BAMD_RECB_Q6K;
    static constexpr int CHRT = X_CH6_RT, PH_SB = 8192, PH_RT = 1024;
    uint2 ql[2]; uint32_t qh[2]; uint4 sc[2][2];
    bamd_h2u v0, v1, v2, v3;
    template <int S> __device__ __forceinline__ void load_set(int hs, const uint8_t * wql, const uint8_t * wqh, const uint8_t * phb) {     // operands of half step hs = 2 ci + h
        const int ci = hs >> 1, h = hs & 1;
        ql[S] = *(const uint2 *) (wql + (size_t) ci * RECB + h * 64);
        qh[S] = *(const uint32_t *) (wqh + (size_t) ci * RECB + h * 32);
        sc[S][0] = *(const uint4 *) (phb + (size_t) hs * (PH_SB / 2)); sc[S][1] = *(const uint4 *) (phb + (size_t) hs * (PH_SB / 2) + 256);
    }
    __device__ __forceinline__ void build_a(int S, int j) {
        // the two high bits of a quant sit at bits sh, sh + 1 (sub-block 2g) / sh + 2, sh + 3 (2g + 1) of their byte of hq (sh = 4 j) and belong at bits 4, 5
        const bamd_h2 k1056 = { (_Float16) -1056.f, (_Float16) -1056.f };
        const uint2 q = ql[S]; const uint32_t hq = qh[S], sh = 4u * (uint32_t) j;
        const uint32_t uA = (__builtin_amdgcn_alignbit(hq, hq, (28u + sh) & 31u) & 0x30303030u) | ((q.x >> sh) & 0x0f0f0f0fu);
        const uint32_t uB = (__builtin_amdgcn_alignbit(hq, hq, (30u + sh) & 31u) & 0x30303030u) | ((q.y >> sh) & 0x0f0f0f0fu);
        bamd_h2u c;
        c.u = __builtin_amdgcn_perm(0x64646464u, uA, 0x04010400u); v0.h = c.h + k1056;      // (1024 + q) - 1056 = q - 32, exact
        c.u = __builtin_amdgcn_perm(0x64646464u, uA, 0x04030402u); v1.h = c.h + k1056;
        c.u = __builtin_amdgcn_perm(0x64646464u, uB, 0x04010400u); v2.h = c.h + k1056;
        c.u = __builtin_amdgcn_perm(0x64646464u, uB, 0x04030402u); v3.h = c.h + k1056;
    }
    __device__ __forceinline__ void build_b(int S, int j, unsigned char * dst) const {  // dst: the A_a fragment; A_l X_FR bytes behind it
        const uint4 s = sc[S][j];
        bamd_h2u sa0, sl0, sa1, sl1, x0, x1, x2, x3; sa0.u = s.x; sl0.u = s.y; sa1.u = s.z; sl1.u = s.w;
        x0.h = v0.h * sa0.h; x1.h = v1.h * sa0.h; x2.h = v2.h * sa1.h; x3.h = v3.h * sa1.h;
        *(uint4 *) dst = (uint4) { x0.u, x1.u, x2.u, x3.u };
        x0.h = v0.h * sl0.h; x1.h = v1.h * sl0.h; x2.h = v2.h * sl1.h; x3.h = v3.h * sl1.h;
        *(uint4 *) (dst + X_FR) = (uint4) { x0.u, x1.u, x2.u, x3.u };
    }
};
// wave (rt, tp) = row tile rt x slot tiles 2 tp, 2 tp + 1.  A step is HALF a super-block (four e); the fragment ring holds two half steps x 4 row tiles x 4 e x 2
// fragments, the activation stage (whole super-blocks) is refilled every second half step
template <int MODE>
__global__ void __launch_bounds__(512) moe_mfma2_q6k_kernel(bamd_moe_mma_args a) {
    typedef MoeQ6K F;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int ex, first, nt;
    if (!moe_tile(a, blockIdx.x, ex, first, nt)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id(), m = lane & 15, g = lane >> 4;
    const int rt = wave >> 1, tp = wave & 1;
    const int nb = a.K >> 8;
    const int rb = blockIdx.y, rtg = rb * 4 + rt;
    const size_t b16 = BAMD_BLOB16_BYTES(nb);
    const uint8_t * wex = a.w + (size_t) ex * a.wstride, * ph = a.aux + (size_t) ex * a.astride, * ch = ph + a.ch_off;
    const uint32_t lds0 = (uint32_t) (size_t) (bamd_lds_vp) smem;
    // XStage's plan with the record sources gathered: rounds 0..3 (and round 4 of waves 0..5) are records, round 4 of wave 6 the 16 header chunks, the 64 block
    // scales d_y (behind a row's records) one 4-byte instruction on wave 1
    XStage<4 * F::CHRT / 16> stg;
#pragma unroll
    for (int r = 0; r < 4; ++r) stg.off[r] = moe_rec_off<MODE>(a, first, nt, r * 512 + tid, b16);
    stg.off[4] = wave < 6 ? moe_rec_off<MODE>(a, first, nt, 2048 + tid, b16) : (uint32_t) (tid - 384) * 16u;
    stg.offx = 0u; stg.x_on = false;
    if (wave == 1) stg.offx = moe_rec_off<MODE>(a, first, nt, lane * BAMD_B16_Q, b16) + (uint32_t) nb * BAMD_B16_REC;
    const uint8_t * chb = ch + (size_t) rb * nb * (4 * F::CHRT);
    auto stage = [&](int ci, int b) { stg.issue(a.blob16 + (size_t) ci * BAMD_B16_REC, chb + (size_t) ci * (4 * F::CHRT), a.blob16 + (size_t) ci * 4, lds0 + X_BLK0 + (uint32_t) b * X_BLK, wave, lane); };
    // builder (the stream's own rows, one record group per wave): wave (rt, q = tp), lane (p = lane >> 5, r = (lane >> 2) & 7, el = lane & 3) takes, per half step, chunk
    // e = 4 H + el of row 8q + r and builds the pieces of MFMA lanes (8q + r, g = 2p + j), j = 0, 1, of fragment e: per half step the ql dwords 2p, 2p + 1 and the qh
    // dword p of stream lane (r, e)
    const int bp = lane >> 5, br = (lane >> 2) & 7, bel = lane & 3;
    const uint8_t * rec0 = wex + (size_t) (2 * rtg + tp) * nb * F::RECB;
    const uint8_t * w0 = rec0 + (size_t) ((br * 8 + bel) * 16 + bp * 8), * w1 = rec0 + 1024 + (size_t) ((br * 8 + bel) * 8 + bp * 4);
    const uint8_t * phb = ph + (size_t) rb * nb * F::PH_SB + (size_t) rt * F::PH_RT + (size_t) (((2 * bp) * 16 + 8 * tp + br) * (F::PH_RT / 64));
    F f;
    unsigned char * afw = smem + X_AF0 + (rt * 4 + bel) * (2 * X_FR) + ((2 * bp) * 16 + 8 * tp + br) * 16;     // [row tile][e' = 0..3][2 x X_FR]: MFMA lane (8 tp + br, 2 bp + j) at + j * 256
    const unsigned char * afr = smem + X_AF0 + rt * 8 * X_FR + lane * 16;
    const unsigned char * tok = smem + X_BLK0 + (size_t) ((2 * tp) * 16 + m) * BAMD_B16_REC;       // this lane's slot record of tile n = 0; n = 1: 16 records on
    const unsigned char * bop = tok + g * 16;
    X2Hdr<false> hdr; hdr.init(tok, smem + X_BLK0, rt * F::CHRT, (2 * tp) * 16 + m, g);
    bamd_f4 acc[2][8];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[n][e] = (bamd_f4) { 0.f, 0.f, 0.f, 0.f };
    }
    stage(0, 0);
    f.template load_set<0>(0, w0, w1, phb);
    f.template load_set<1>(1, w0, w1, phb);
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
        f.template load_set<H>(hs + 2 < nhs ? hs + 2 : nhs - 2 + H, w0, w1, phb);
        __builtin_amdgcn_sched_barrier(0);
        float D[2][4];
        hdr.read(BLK, H, D);
        bamd_h8 Aq[2][2], Bq[2][2];
        auto load_ops = [&](int e) {                           // A fragments and B operands of e, double-buffered
#pragma unroll
            for (int p = 0; p < 2; ++p) Aq[e & 1][p] = *(const bamd_h8 *) (afr + H * X_AF_BYTES + e * (2 * X_FR) + p * X_FR);
#pragma unroll
            for (int n = 0; n < 2; ++n) Bq[e & 1][n] = *(const bamd_h8 *) (bop + BLK * X_BLK + n * (16 * BAMD_B16_REC) + (4 * H + e) * 64);
        };
        load_ops(0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e + 1 < 4) load_ops(e + 1);
            if ((e & 1) == 0) f.build_a(NXT, e >> 1);
#pragma unroll
            for (int n = 0; n < 2; ++n) {                      // two MFMAs chained through the accumulator: the exact integer isum_e of the tile
                bamd_f4 s = { 0.f, 0.f, 0.f, 0.f };
#pragma unroll
                for (int p = 0; p < 2; ++p) s = __builtin_amdgcn_mfma_f32_16x16x32_f16(Aq[e & 1][p], Bq[e & 1][n], s, 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[n][4 * H + e][i] = fmaf(D[n][i], s[i], acc[n][4 * H + e][i]);
            }
            if (e & 1) f.build_b(NXT, e >> 1, afw + NXT * X_AF_BYTES + (e >> 1) * 256);
            __builtin_amdgcn_sched_barrier(0);
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
    // hsum_float_8 over e, then rows 4g .. 4g+3 of the slot's pair
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int u = (2 * tp + n) * 16 + m;
        if (u >= nt) continue;
        float val[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) val[i] = x_hsum8(acc[n], i);
        moe_store<MODE>(a, moe_pair(a, first, nt, u), rtg * 16 + 4 * g, val);
    }
}

// ==== host side ===========================================================================================================================================
static long long g_moe_batch_mfma_runs = 0;
extern "C" __attribute__((visibility("default"))) long long bamd_moe_batch_mfma_runs(void) { return g_moe_batch_mfma_runs; }
// per tensor: a K-quant with a grouped kernel here, or a type whose own family switch is on: Q3_K / Q2_K / IQ4_XS (bamd_moe_batch_kq_mfma.hip) and the 32-weight
// block types (bamd_moe_batch_b32_mfma.hip)
static inline bool moe_kq_type(int type) { return type == BAMD_Q3_K || type == BAMD_Q2_K || type == BAMD_IQ4_XS; }
static inline bool moe_mfma_type(int type) { return type == BAMD_Q4_K || type == BAMD_Q5_K || type == BAMD_Q6_K || ((bamd_is_b32(type) || moe_kq_type(type)) && bamd_prefill_mfma_type(type)); }

template <int MODE>
static void launch_moe_mma(const bamd_moe_batch_args & b, const void * w, const void * aux, size_t astride, hipStream_t s) {
    const bamd_moe_args & m = b.m;
    constexpr bool GU = MODE != MOE_DOWN;
    const int type = GU ? m.type_gu : m.type_d;
    bamd_moe_mma_args a;
    a.w = (const uint8_t *) w; a.wstride = GU ? m.stride_gu : m.stride_d; a.aux = (const uint8_t *) aux; a.astride = astride;
    a.K = GU ? m.E : m.F; a.nrows = GU ? m.F : m.E; a.npairs = b.T * m.n_used; a.n_used = m.n_used; a.n_expert = m.n_expert;
    a.ch_off = bamd_is_b32(type) ? 0 : bamd_prefill_aux_ph_bytes(type, a.nrows, a.K);      // the builder part, as bamd_launch_prefill_aux lays it out in front of the consumer part
    a.blob16 = (const uint8_t *) b.blob16; a.lists = b.lists; a.tiles = b.tiles; a.out = GU ? m.h : b.prod; a.wgt = m.w;
    if (bamd_is_b32(type)) { bamd_launch_moe_mma_b32(a, type, MODE, a.npairs / 64 + m.n_expert, s); bamd_prefill_mfma_count(type); return; }
    if (moe_kq_type(type)) { bamd_launch_moe_mma_kq(a, type, MODE, a.npairs / 64 + m.n_expert, s); bamd_prefill_mfma_count(type); return; }
    const dim3 grid(a.npairs / 64 + m.n_expert, a.nrows / 64);
    auto launch = [&](auto kernel, int threads, size_t lds) { bamd_allow_lds(kernel, lds); hipLaunchKernelGGL(kernel, grid, dim3(threads), lds, s, a); };
    if (type == BAMD_Q6_K)      launch(moe_mfma2_q6k_kernel<MODE>, 512, X_LDS_BYTES);
    else if (type == BAMD_Q5_K) launch(moe_mfma3_q4k_kernel<MODE, true>, 1024, X3_LDS_BYTES);
    else                        launch(moe_mfma3_q4k_kernel<MODE, false>, 1024, X3_LDS_BYTES);
    bamd_prefill_mfma_count(type);
}
int bamd_moe_batch_mfma_ready(const bamd_moe_batch_args & a) {
    const bamd_moe_args & m = a.m;
    if ((bamd_is_b32(m.type_gu) || bamd_is_b32(m.type_d)) && !a.blob) return 0;      // the Q8_0 / Q8_1 quantiser writes its int8 image beside the f16 records
    return bamd_prefill_moe_on() && a.blob16 && a.aux_g && a.aux_u && a.aux_d && moe_mfma_type(m.type_gu) && moe_mfma_type(m.type_d) && !(m.E & 255) && !(m.F & 255) &&
           a.T * m.n_used <= 4096 && (size_t) a.T * m.n_used * BAMD_BLOB16_BYTES((m.E > m.F ? m.E : m.F) >> 8) < ((size_t) 1 << 32);
}
// launches 4 (gate, then up) and 6 (down) of the batched feed-forward; the caller (bamd_launch_moe_ffn_batch) has run the grouping with tt = 64 and written blob16,
// and whoever built the side tables has asked bamd_prefill_mfma_supported
void bamd_launch_moe_gate_up_mfma(const bamd_moe_batch_args & a, hipStream_t s) {
    launch_moe_mma<MOE_GATE>(a, a.m.wg, a.aux_g, a.aux_stride_gu, s);
    launch_moe_mma<MOE_UP>(a, a.m.wu, a.aux_u, a.aux_stride_gu, s);
    g_moe_batch_mfma_runs += 1;
}
void bamd_launch_moe_down_mfma(const bamd_moe_batch_args & a, hipStream_t s) { launch_moe_mma<MOE_DOWN>(a, a.m.wd, a.aux_d, a.aux_stride_d, s); }
