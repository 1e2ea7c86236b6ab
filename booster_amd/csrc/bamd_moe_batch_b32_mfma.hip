// bamd_moe_batch_b32_mfma.hip — the grouped, gathered expert mat-muls of a mixture-of-experts prompt micro-batch on the matrix cores for experts of the 32-weight
// block formats: launches 4 (gate, then up) and 6 (down) of bamd_moe_batch.hip for Q8_0 / Q4_0 / Q5_0 (Q8_0 activations), Q4_1 / Q5_1 (Q8_1 activations, the summs
// chain) and IQ4_NL (two accumulator sets by block parity).  Taken while BAMD_PREFILL_MOE is on AND the type's own family switch (BAMD_PREFILL_Q0 / _Q1 / _NL) is on;
// both default off (bamd_prefill_family.h).  It is the counterpart of matmul_mfma_b32_kernel (bamd_prefill2_b32.hip) on the tile table, pair lists, per-expert
// strides and scattered epilogues of bamd_moe_batch_mfma.hip; gate/up and down choose their kernel independently, so a K-quant sibling may read the same table.
//
// Arithmetic: the contract at the top of bamd_prefill2_b32.hip and in bamd_b32_device.h, instruction for instruction — v_mfma_f32_16x16x4_4b_f16 for the four-term
// dots over exact f16 operands ((0x6400 | u) plus the type's constant, y_kzero), one f32 scale product per (row, pair, block), the chain links as v_pk_fma_f32 in
// block order behind the NEXT MFMA's issue, b32_finish_row's tree, + summs (with a minimum), accum1 + accum2 per lane e (IQ4_NL).  Per (row, pair) the bits are
// those of the grouped integer-dot kernel (bamd_moe_batch_b32.hip), of the routed decode launches and of llm_build_moe_ffn.
//
// Work split.  The grouping launch writes ONE table of tiles of up to 64 pairs of one expert (tt = 64: a K-quant sibling reads it too).  The wave tile stays the
// one recorded as not spilling: 16 rows x 32 pairs with 64 accumulator registers, or 16 x 16 with two sets (IQ4_NL), four waves = 64 rows to a workgroup.  A tile
// is covered by 64 / YTile::TOK SUB-TILES of 32 (IQ4_NL: 16) pairs, one workgroup each: blockIdx.x = tile * NSUB + sub, blockIdx.y = row block of 64.  A workgroup
// whose tile is past the table, or whose sub-tile starts at or past the tile's count, exits before its first barrier (both conditions are workgroup-uniform).
//   * Why workgroups and not eight waves holding both halves of a tile: every weight line is then requested by exactly one wave of a workgroup and the stage, the
//     staging plan and the half step are the dense kernel's unchanged (17 920 / 18 944 / 8 960 B, two workgroups' worth resident next to each other), and a tile of
//     at most 32 pairs — the common case in a short micro-batch, where an expert meets few tokens — starts no idle waves at all.  The price is that a tile of more
//     than 32 pairs reads its expert's rows once per sub-tile; the sub-tiles of a tile are neighbours in blockIdx.x (not a blockIdx.z apart), as the tiles of an
//     expert already are, so these workgroups are dispatched together and the second read of a line meets the first in L2.
//   * Gate and up are two launches (up reads gate's h in place), as on the K-quant matrix-core path; one launch computing both would hold the gate values next to
//     64 accumulators.
//   Neither the eight-wave placement nor a fused gate/up launch was built; no measurement compares them.
// Gather: each staging thread computes its source offsets once, from the pair list — gate / up read the record row of the pair's TOKEN (pair / n_used), down the
// pair's own row of h; slots past the tile's count re-read the tile's last pair and are never stored.  What tiles / lists hold is bounded again where it becomes
// an address (moe_tile, moe_pair).  Staging is global -> registers -> LDS at the 528-byte pitch, double-buffered, one barrier per record; the weights go straight
// to registers from w + expert x stride; the side-table rows (bamd_launch_prefill_aux per expert: 32 B, with a minimum 64 B per row and 256 weights, IQ4_NL on the
// Q4_0 table) come from aux + expert x aux stride.  Rows (F, E) are multiples of 256: no ragged row block, and no slack is read behind an expert's stream (the
// record index is clamped at the end of K, as in the dense kernel).
// Epilogues, scattered by pair id: gate stores h[pair]; up stores silu(h[pair]) x value in place (every lane reads and writes its own elements: one row, its
// four pairs per token tile — sixteen lanes = 64 consecutive bytes of a pair's row); down stores value x w[pair], rounded before any add, to prod[pair].
#include "bamd_prefill2_b32.h"
#include "bamd_moe_batch_mfma.h"
#include "bamd_mv_select.h"
#include "bamd_kernels.h"

template <int TYPE, int MODE>
__global__ void __launch_bounds__(256) moe_mfma_b32_kernel(bamd_moe_mma_args a) {
    constexpr int RECB = BAMD_RECB_OF(TYPE);
    constexpr bool MIN = b32_has_min(TYPE);
    typedef YTile<TYPE> Y;
    constexpr int NT = Y::NT, NP = Y::NP, Y_TOK = Y::TOK, Y_XD_OFF = Y::XD_OFF, Y_XS_OFF = Y::XS_OFF, Y_STAGE = Y::STAGE, NSC = MIN ? 16 : 8;      // NSC: side-table floats of a row and record
    constexpr int NSUB = 64 / Y_TOK;                           // sub-tiles of a tile
    static_assert(!(MIN && NP == 2), "no type has a minimum and two accumulator sets");
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * Y_STAGE];
    int ex, first, nt;
    if (!moe_tile(a, blockIdx.x / NSUB, ex, first, nt)) return;
    const int u0 = (int) (blockIdx.x % NSUB) * Y_TOK;          // first slot of this sub-tile
    if (u0 >= nt) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4, r = j & 7;
    const int nb = a.K >> 8;
    const int row0 = blockIdx.y * Y_ROWS + wave * 16;
    const int rg = (row0 >> 3) + (j >> 3);                     // (nrows is a multiple of 64: every record group exists)
    const uint8_t * wrec = a.w + (size_t) ex * a.wstride + (size_t) rg * nb * RECB;
    const float * wsc = (const float *) (a.aux + (size_t) ex * a.astride) + ((size_t) rg * nb * 8 + r) * NSC;
    const size_t b16 = BAMD_BLOB16_BYTES(nb);
    // record row of slot tok of the sub-tile: the pair's token (gate / up) or the pair itself (down); slots past the count: the tile's last pair
    auto src_row = [&](int tok) { const int p = moe_pair(a, first, nt, u0 + tok); return (size_t) (MODE == MOE_DOWN ? p : p / a.n_used); };
    // staging plan of the dense kernel: 2 NT 16-byte pieces of quants and one block scale (MIN: one {d_x, s_x} pair) per thread and record.
    // NT == 1: the 128 block scales of a stage are taken twice, by threads t and t + 128: the same value to the same address, and no branch in the loop
    const uint8_t * sq[2 * NT]; uint32_t dq[2 * NT];
#pragma unroll
    for (int k = 0; k < 2 * NT; ++k) {
        const int idx = k * 256 + tid, tok = idx >> 5, q = idx & 31;
        sq[k] = a.blob16 + src_row(tok) * b16 + q * 16; dq[k] = (uint32_t) (tok * Y_QSTR + q * 16);
    }
    const uint8_t * sx; uint32_t dx;
    {
        const int tok = NT == 2 ? tid >> 3 : (tid >> 3) & 15, c = tid & 7;
        sx = a.blob16 + src_row(tok) * b16 + 512 + c * 4; dx = (uint32_t) (Y_XD_OFF + (c * Y_TOK + tok) * 4);
    }
    uint4 stq0, stq1, stq2, stq3; float stxd, stxs;            // (named, not an array: bamd_prefill2_b32.hip)
    auto stage_load = [&](int ci) {
        const size_t o = (size_t) ci * BAMD_B16_REC;
        stq0 = *(const uint4 *) (sq[0] + o); stq1 = *(const uint4 *) (sq[1] + o);
        if constexpr (NT == 2) { stq2 = *(const uint4 *) (sq[2] + o); stq3 = *(const uint4 *) (sq[3] + o); }
        stxd = *(const float *) (sx + o);
        if (MIN) stxs = *(const float *) (sx + o + 32);
    };
    auto stage_store = [&](int buf) {
        unsigned char * d = smem + buf * Y_STAGE;
        *(uint4 *) (d + dq[0]) = stq0; *(uint4 *) (d + dq[1]) = stq1;
        if constexpr (NT == 2) { *(uint4 *) (d + dq[2]) = stq2; *(uint4 *) (d + dq[3]) = stq3; }
        *(float *) (d + dx) = stxd;
        if (MIN) *(float *) (d + dx + (Y_XS_OFF - Y_XD_OFF)) = stxs;
    };
    // [set][e][pair of slots], set = slot tile n (NP == 1) or block parity (NP == 2): slots 16 n + 4 g + 0..3 of row j, written as float2 operations (v_pk_fma_f32,
    // an IEEE fma per half) so that the links of an accumulator stay a chain in block order; summs (MIN): [slot tile n][pair of slots]
    bamd_f2 acc[2][8][2], summs[2][2];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { acc[n][e][0] = (bamd_f2) { 0.f, 0.f }; acc[n][e][1] = (bamd_f2) { 0.f, 0.f }; }
        summs[n][0] = (bamd_f2) { 0.f, 0.f }; summs[n][1] = (bamd_f2) { 0.f, 0.f };
    }
    const _Float16 kz = y_kzero<TYPE>();
    const bamd_h2q kzero = { kz, kz };
    auto chain = [&](int n, int eh, const bamd_f16v & s, const bamd_f4 & S) {           // the links (l, 4 eh + 0..3) of the lane's four slots of tile n
        const bamd_f2 Slo = { S[0], S[1] }, Shi = { S[2], S[3] };
#define Y_LINK(blk_) do { \
            acc[n][4 * eh + blk_][0] = __builtin_elementwise_fma(Slo, __builtin_shufflevector(s, s, 4 * blk_, 4 * blk_ + 1), acc[n][4 * eh + blk_][0]); \
            acc[n][4 * eh + blk_][1] = __builtin_elementwise_fma(Shi, __builtin_shufflevector(s, s, 4 * blk_ + 2, 4 * blk_ + 3), acc[n][4 * eh + blk_][1]); } while (0)
        Y_LINK(0); Y_LINK(1); Y_LINK(2); Y_LINK(3);
#undef Y_LINK
    };
    // half step: blocks c = 4h .. 4h+3 of a record whose activations are in `stage`; dm: the row's d (0..7) and, MIN, m (8..15) of the record
    auto half_step = [&](const HalfB32<TYPE> & H, int h, const float (&dm)[NSC], const unsigned char * stage) {
        const unsigned char * aq = stage + j * Y_QSTR + g * 16;
        const unsigned char * xd = stage + Y_XD_OFF + g * 16;
        bamd_f16v prev; bamd_f4 Sprev;
#pragma unroll
        for (int cl = 0; cl < 4; ++cl) {
            const int c = 4 * h + cl;
            bamd_f4 S[NT], sxv[NT];
            union { uint2 u; bamd_h4 h; } A[NT][2], B[2];
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const bamd_f4 x = *(const bamd_f4 *) (xd + (c * Y_TOK + 16 * n) * 4);
                if (MIN) sxv[n] = *(const bamd_f4 *) (xd + (Y_XS_OFF - Y_XD_OFF) + (c * Y_TOK + 16 * n) * 4);
#pragma unroll
                for (int i = 0; i < 4; ++i) S[n][i] = dm[c] * x[i];
                const uint4 av = *(const uint4 *) (aq + n * (16 * Y_QSTR) + c * 64);
                A[n][0].u = (uint2) { av.x, av.y }; A[n][1].u = (uint2) { av.z, av.w };
            }
#pragma unroll
            for (int eh = 0; eh < 2; ++eh) {
                const uint32_t u = half_bytes(H, h, cl, eh);
                bamd_h2qu lo, hi;
                lo.u = __builtin_amdgcn_perm(0x64646464u, u, 0x04010400u); lo.h = lo.h + kzero;
                hi.u = __builtin_amdgcn_perm(0x64646464u, u, 0x04030402u); hi.h = hi.h + kzero;
                B[eh].u = (uint2) { lo.u, hi.u };
            }
            const bamd_f2 mw = { dm[MIN ? 8 + c : c], dm[MIN ? 8 + c : c] };            // MIN: m_w of block c
#pragma unroll
            for (int k = 0; k < 2 * NT; ++k) {                 // (eh, n) = (k / NT, k % NT); a link's set: the slot tile, or (NP == 2) the parity of its block
                const int eh = k / NT, n = k % NT;
                bamd_f16v z;
#pragma unroll
                for (int v = 0; v < 16; ++v) z[v] = 0.f;
                const bamd_f16v s = __builtin_amdgcn_mfma_f32_16x16x4f16(A[n][eh].h, B[eh].h, z, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);             // the MFMA first, the previous one's chain behind it
                if (k > 0) chain(NP == 2 ? cl & 1 : (k - 1) % NT, (k - 1) / NT, prev, S[(k - 1) % NT]);
                else if (cl > 0) chain(NP == 2 ? (cl - 1) & 1 : NT - 1, 1, prev, Sprev);
                if (MIN && k < NT) {                            // step c of the four summs pairs of slot tile k: summs += m_w[c] * s_x[c][slot]
                    summs[k][0] = __builtin_elementwise_fma(mw, (bamd_f2) { sxv[k][0], sxv[k][1] }, summs[k][0]);
                    summs[k][1] = __builtin_elementwise_fma(mw, (bamd_f2) { sxv[k][2], sxv[k][3] }, summs[k][1]);
                }
                prev = s;
                __builtin_amdgcn_sched_barrier(0);
            }
            Sprev = S[NT - 1];
        }
        chain(1, 1, prev, Sprev);                              // set 1: the last slot tile, and the parity of block 4h + 3
    };
    HalfB32<TYPE> H0, H1;
    float dm[NSC], dmn[NSC];
    auto load_dm = [&](float (&d)[NSC], int ci) {
#pragma unroll
        for (int q = 0; q < NSC / 4; ++q) {
            const bamd_f4 v = *(const bamd_f4 *) (wsc + (size_t) ci * (8 * NSC) + 4 * q);
#pragma unroll
            for (int i = 0; i < 4; ++i) d[4 * q + i] = v[i];
        }
    };
    stage_load(0);
    load_half(H0, wrec, 0, r, g);
    load_dm(dm, 0);
    stage_store(0);
    __syncthreads();
    for (int ci = 0; ci < nb; ++ci) {
        const int cn = ci + 1 < nb ? ci + 1 : ci;             // (clamped, no branch inside the loop: the last record is staged once more into the buffer nobody reads again)
        const unsigned char * stage = smem + (ci & 1) * Y_STAGE;
        stage_load(cn);
        load_half(H1, wrec + (size_t) ci * RECB, 1, r, g);
        load_dm(dmn, cn);
        __builtin_amdgcn_sched_barrier(0);
        half_step(H0, 0, dm, stage);
        load_half(H0, wrec + (size_t) cn * RECB, 0, r, g);
        __builtin_amdgcn_sched_barrier(0);
        half_step(H1, 1, dm, stage);
#pragma unroll
        for (int i = 0; i < NSC; ++i) dm[i] = dmn[i];
        stage_store((ci + 1) & 1);                             // the buffer read in step ci - 1: every wave is past that step's barrier
        __syncthreads();
    }
    const int row = row0 + j;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int u = u0 + 16 * n + 4 * g + i;
#define Y_ACC(e_) (NP == 2 ? acc[0][e_][i >> 1][i & 1] + acc[1][e_][i >> 1][i & 1] : acc[n][e_][i >> 1][i & 1])                          /* NP == 2: accum1 + accum2, lane e */
            const float tree = ((Y_ACC(0) + Y_ACC(4)) + (Y_ACC(2) + Y_ACC(6))) + ((Y_ACC(1) + Y_ACC(5)) + (Y_ACC(3) + Y_ACC(7)));      // b32_finish_row's tree
#undef Y_ACC
            const float val = MIN ? tree + summs[n][i >> 1][i & 1] : tree;                                                             // b32_finish_row<MIN>
            if (u < nt) {
                const int p = moe_pair(a, first, nt, u);
                float * o = a.out + (size_t) p * a.nrows + row;
                *o = MODE == MOE_UP ? v_silu(*o) * val : MODE == MOE_DOWN ? val * a.wgt[p] : val;      // down: ggml_mul(experts, weights), rounded before any add
            }
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------
// the launch behind launch_moe_mma (bamd_moe_batch_mfma.hip), which fills the arguments for every family alike; tile_bound: the host-known bound of the tile table
void bamd_launch_moe_mma_b32(const bamd_moe_mma_args & a, int type, int mode, int tile_bound, hipStream_t s) {
    with_const(consts<BAMD_Q8_0, BAMD_Q4_0, BAMD_Q5_0, BAMD_Q4_1, BAMD_Q5_1, BAMD_IQ4_NL>(), type, [&](auto TY) -> bool {
        constexpr int TYPE_ = decltype(TY)::value;
        const dim3 grid(tile_bound * (64 / YTile<TYPE_>::TOK), a.nrows / Y_ROWS);
        return with_const(consts<MOE_GATE, MOE_UP, MOE_DOWN>(), mode, [&](auto M) -> bool {
            hipLaunchKernelGGL((moe_mfma_b32_kernel<TYPE_, decltype(M)::value>), grid, dim3(256), 0, s, a);
            return true; }); });
}
