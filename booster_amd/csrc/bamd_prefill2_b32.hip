// bamd_prefill2_b32.hip — the exact matrix-core prompt mat-mul for the 32-weight block formats: Q8_0 / Q4_0 / Q5_0 weights x Q8_0 activations behind the switch
// BAMD_PREFILL_Q0 / bamd_set_prefill_q0, Q4_1 / Q5_1 weights x Q8_1 activations behind BAMD_PREFILL_Q1 / bamd_set_prefill_q1, IQ4_NL weights x Q8_0 activations
// behind BAMD_PREFILL_NL / bamd_set_prefill_nl (all three default off; the list of types is bamd_prefill_mfma_type, bamd_prefill_family.h).  One kernel template for
// the six types; MIN = b32_has_min(TYPE) marks what the types with a minimum add, YTile<TYPE>::NP == 2 what the type with two accumulator sets (b32_two_acc) changes.
//
// Arithmetic: the contract of bamd_b32_device.h.  One output = eight f32 chains e = 0..7 over the 32-weight blocks l in order,
//     acc_e = fma(f32(d_w) * f32(d_x), (float) dot4_e, acc_e),         dot4_e = the signed dot of bytes 4e .. 4e+3 of weight block and activation block,
// closed by b32_finish_row's tree.  A chain link sums FOUR products, so the K = 32 instructions of bamd_prefill2.hip would add across links; what fits are the
// K = 4 multi-block forms.  This kernel uses v_mfma_f32_16x16x4_4b_f16: one instruction = the links (l, e = 4 eh + 0..3) of a 16 x 16 tile.  With f16 operands
// (|w| <= 128, |x| <= 127) every product and every four-term sum is an integer below 2^24, exact in f32 in any order; the scale product of two widened f16 is
// exact as well.  The links themselves stay on the VALU: one f32 multiply per (row, token, block) and one fma per (row, token, block, e), in block order.
// (The two-block 32 x 32 form has the same rate — tools/mfma_k4_probe.hip — but a wave must then hold 128 accumulators and two 32-register results next to
// them: the first version of this kernel did, and spilled.  Four blocks of 16 x 16 put all eight e of a 16-row x 32-token wave tile in 64 registers.)
// MIN: a second accumulator per output,
//     summs = summs + f32(m_w) * f32(s_x)                               one scalar chain per (row, token).  The product of two widened f16 is exact in f32,
//                                                                       so a multiply and an add give the bits of one fma; the K/32 steps stay in block order
// and the result is the tree over acc_e, plus summs.  The weights of the 8-lane chain are UNSIGNED and without an offset there (Q4_1: the nibble 0..15, Q5_1:
// nibble | bit << 4, 0..31): the B operand is (0x6400 | u) - 1024 = u, exact in f16; |w| <= 31, |x| <= 127: every four-term sum is an integer far below 2^24.
//
// Layout.  The activations are the A operand, the weights the B operand: D[i = token][j = row], so a lane owns ONE weight row (j = lane & 15) and four tokens
// per token tile (register v: block v >> 2, token 4 (lane >> 4) + (v & 3)); its row's eight d_w of a record are two 16-byte loads of the side table, the tokens'
// d_x come from LDS.  Lane maps of the instruction (tools/mfma_k4_probe.hip checks them with exact integers): A / B lane = 16 block + i / j, the four k in
// the lane's four halves.
//   * a workgroup is four waves = 64 rows x 32 tokens; a wave owns 16 rows x two token tiles of 16 with all eight e: 64 accumulator registers (two sets: below);
//   * per record (256 of K) the 32 tokens' f16 quants and f32 block scales are staged global -> registers -> LDS, double-buffered, one barrier per record;
//     a token's 512 bytes sit 528 bytes apart (132 dwords = 4 mod 64: the 16-byte reads of sixteen lanes fall on sixteen bank quads);
//   * the weights never go through LDS: MFMA lane (row j, block g) needs, for chunk e = 4 eh + g, exactly the dwords that wave-stream lane (r = j & 7, e) of
//     its record group holds, so each lane loads its own 16-byte pieces half a record ahead and unpacks them with the 0x6400 | byte v_perm idiom of
//     build_a (bamd_prefill2.hip): (1024 + u) - (1024 + offset), exact in f16, u = byte ^ 0x80 (Q8_0), nibble (Q4_0, Q4_1), nibble | bit 4 (Q5_0, Q5_1),
//     table value ^ 0x80 (IQ4_NL);
//   * the chain of one MFMA's 16 results follows the NEXT MFMA's issue (no MFMA -> VALU wait states in front of it).
// Side table ("prefill aux"): the eight f16 d of every row and record widened to f32, [record group][record][row][block] — 32 B per row and 256 weights.
// What MIN adds:
//   * the lane (row j, tokens 16 n + 4 g + 0..3) carries eight summs accumulators next to its 64 chain accumulators.  Per block it takes ONE step of each, written
//     as two-wide vector fmas (v_pk_fma_f32, an IEEE fma per half) whose only operand that changes is the accumulator itself: the order of a summs chain is its
//     data dependence, block c + 1 after block c, and there is no scalar f32 add for the SLP vectoriser to gather into a tree;
//   * side table: the row's eight f16 d AND eight f16 m of every record widened to f32, [record group][record][row r][d 0..7 | m 0..7] — 64 B per row and 256
//     weights, four 16-byte loads per lane and record;
//   * f16 activation records (quantize_batch_b32_kernel, bamd_prefill_b32.hip): the Q8_0 form's 512 B of quants and eight f32 d_x at byte 512, then the eight s_x
//     widened to f32 at byte 544 (576 of the BAMD_B16_REC bytes used); d_x and s_x of a stage sit side by side in LDS, [block c][token].
// What two accumulator sets change (IQ4_NL, the contract of bamd_b32_device.h: the even blocks into accum1, the odd ones into accum2):
//   * one output = TWO sets of eight chains, acc[l & 1]_e = fma(f32(d_w) * f32(d_x), (float) dot4_e, acc[l & 1]_e), dot4_e = the dot of kvalues_iq4nl[nibble] with
//     bytes 4e .. 4e+3 of the activation block, closed by a_e = acc[0]_e + acc[1]_e and b32_finish_row's tree over a_e.  A record is eight consecutive blocks, so
//     l & 1 = c & 1 with c the block's index in the record: a compile-time index of the unrolled half step, the choice of the set costs no instruction;
//   * weight operand: the nibble dword through b32_iq4nl_values (bamd_device.h, where the table stands), ^ 0x80808080 gives u = value + 128 (1 .. 241),
//     and (0x6400 | u) - 1152 is the table value, exact in f16 — the Q8_0 constant.  |w| <= 127, |x| <= 127: every four-term sum is an integer <= 64 516 < 2^24;
//   * tile: two sets at the 16-row x 32-token wave tile would be 128 accumulator registers, the shape recorded above as spilling.  A wave owns 16 rows x ONE token
//     tile of 16 with all eight e and both parities, 64 registers again, and a workgroup is four waves = 64 rows x 16 tokens: half the stage (8 960 B) and two
//     16-byte staging pieces per thread and record, not four.  The other way to place four such waves, 32 rows x 32 tokens, gives each wave the same instruction
//     stream (its own 16 x 16 tile: one weight unpack, one LDS read and two MFMAs per block either way); the two differ only on the memory side: 64 x 16 walks the
//     matrix once per 16-token tile (T / 16 passes out of L2), 32 x 32 once per 32 tokens but with two waves of a workgroup requesting the same lines and a
//     17 920 B stage.  64 x 16 was chosen: every weight line is requested by exactly one wave of a workgroup, the stage is half the size, and the row /
//     record-group arithmetic (ragged rows included) is unchanged.  The 32 x 32 placement was not built; no measurement compares them;
//   * side table and activations: the record IS the Q4_0 record, so the table is the Q4_0 one, written by prefill_aux_b32_kernel<BAMD_Q4_0>, and the activations are
//     the f16 Q8_0 records unchanged.
#include "bamd_b32_device.h"
#include "bamd_mfma_common.h"
#include "bamd_mv_select.h"

typedef float bamd_f16v __attribute__((ext_vector_type(16)));
typedef float bamd_f2 __attribute__((ext_vector_type(2)));
typedef _Float16 bamd_h2q __attribute__((ext_vector_type(2)));
union bamd_h2qu { uint32_t u; bamd_h2q h; };

#define Y_ROWS 64                                          /* rows of a workgroup: four waves x 16 */
#define Y_QSTR 528                                         /* LDS bytes between the quants of consecutive tokens */
// the tile of a type: a wave owns NT token tiles of 16 and NP accumulator sets per output, NT * NP = 2 either way (64 accumulator registers)
template <int TYPE> struct YTile {
    static constexpr int NP = b32_two_acc(TYPE) ? 2 : 1;      // accumulator sets per output: by block parity
    static constexpr int NT = b32_two_acc(TYPE) ? 1 : 2;      // token tiles of a wave
    static constexpr int TOK = 16 * NT;                       // tokens of a workgroup
    static constexpr int XD_OFF = TOK * Y_QSTR;               // d_x of the stage: [block c][token] f32
    static constexpr int XS_OFF = XD_OFF + 8 * TOK * 4;       // MIN: s_x of the stage, the same shape
    static constexpr int STAGE = b32_has_min(TYPE) ? XS_OFF + 8 * TOK * 4 : XS_OFF;     // 17 920 B, MIN 18 944 B, two sets 8 960 B
};
// a BAMD_B16_REC record in this form uses 544 bytes: element 4e + k of block c as f16 at half c * 32 + (e & 3) * 8 + (e >> 2) * 4 + k (the A operands of both
// e-halves of an MFMA lane are 16 consecutive bytes), then the eight d_x as f32 at byte 512; MIN: 576 bytes, the eight s_x as f32 at byte 544
static_assert(BAMD_B16_REC >= 512 + 32 + 32, "the f16 activation record holds the quants, eight d_x and eight s_x");

struct bamd_mma_b32_args {
    const uint8_t * w;               // wave-stream records (bamd_formats.h)
    const float * sc;                // side table: [record group][record][row r][block c] f32; MIN: [..][row r][d of block 0..7 | m of block 0..7]
    float * out; const float * res;  // [T][ldo]
    const uint8_t * blob16;          // f16 activation records (quantize_batch_b32_kernel)
    int K, T, nrows, nrows_pad, ldo;
};

// grid (records, record groups), 64 threads = (row r, block c); MIN: 128 threads = (row r, d of block 0..7 | m of block 0..7): the record's d / dm table is in
// this order already
template <int TYPE>
__global__ void __launch_bounds__(b32_has_min(TYPE) ? 128 : 64) prefill_aux_b32_kernel(const uint8_t * __restrict__ w, int nb, float * __restrict__ sc) {
    constexpr int RECB = BAMD_RECB_OF(TYPE), SDO = TYPE == BAMD_Q8_0 ? 2048 : b32_has_qh(TYPE) ? 1280 : 1024, NT = b32_has_min(TYPE) ? 128 : 64;
    const size_t rec = (size_t) blockIdx.y * nb + blockIdx.x;
    sc[rec * NT + threadIdx.x] = h2f(*(const unsigned short *) (w + rec * RECB + SDO + threadIdx.x * 2));
}

// the lane's pieces of HALF a record (blocks c = 4h .. 4h+3) for its two chunks e = g and g + 4
template <int TYPE> struct HalfB32 { uint4 q[TYPE == BAMD_Q8_0 ? 2 : 1]; uint32_t qh[2]; };
// (r by reference for the two-set type, by value for the others: either form for all six moves the address arithmetic of the other group's prologue — with r by
//  value the IQ4_NL side-table pointer becomes a float index, its prologue is scheduled in another order and loses one v_mov_b32; profiles/b32_mfma_unify.txt)
template <int TYPE> using y_row_arg = std::conditional_t<b32_two_acc(TYPE), const int &, int>;
template <int TYPE> __device__ __forceinline__ void load_half(HalfB32<TYPE> & H, const uint8_t * rec, int h, y_row_arg<TYPE> r, int g) {
    if (TYPE == BAMD_Q8_0) {
        H.q[0] = *(const uint4 *) (rec + h * 1024 + (r * 8 + g) * 16); H.q[1] = *(const uint4 *) (rec + h * 1024 + (r * 8 + g + 4) * 16);
    } else {
        H.q[0] = *(const uint4 *) (rec + (r * 4 + g) * 32 + h * 16);             // chunks g and g + 4 share the bytes: low / high nibbles
        if (b32_has_qh(TYPE)) { H.qh[0] = *(const uint32_t *) (rec + 1024 + (r * 8 + g) * 4); H.qh[1] = *(const uint32_t *) (rec + 1024 + (r * 8 + g + 4) * 4); }
    }
}
// the four weights of block 4h + cl, chunk 4 eh + g, as unsigned bytes u = weight + offset (128 / 8 / 16; MIN: b32_weights' bytes, no offset)
template <int TYPE> __device__ __forceinline__ uint32_t half_bytes(const HalfB32<TYPE> & H, int h, int cl, int eh) {
    if (TYPE == BAMD_Q8_0) return BAMD_B32_COMP(H.q[eh], cl) ^ 0x80808080u;
    const uint32_t nib = (BAMD_B32_COMP(H.q[0], cl) >> (eh * 4)) & 0x0f0f0f0fu;
    if (TYPE == BAMD_IQ4_NL) return b32_iq4nl_values(nib) ^ 0x80808080u;     // value + 128 (1 .. 241): the table stands in bamd_b32_device.h only
    if (!b32_has_qh(TYPE)) return nib;
    return nib | (((H.qh[eh] >> (4 * h + cl)) & 0x01010101u) << 4);
}

template <int TYPE, int EPI>
__global__ void __launch_bounds__(256) matmul_mfma_b32_kernel(bamd_mma_b32_args a) {
    constexpr int RECB = BAMD_RECB_OF(TYPE);
    constexpr bool MIN = b32_has_min(TYPE);
    typedef YTile<TYPE> Y;
    constexpr int NT = Y::NT, NP = Y::NP, Y_TOK = Y::TOK, Y_XD_OFF = Y::XD_OFF, Y_XS_OFF = Y::XS_OFF, Y_STAGE = Y::STAGE, NSC = MIN ? 16 : 8;      // NSC: side-table floats of a row and record
    static_assert(!(MIN && NP == 2), "no type has a minimum and two accumulator sets");
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * Y_STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4, r = j & 7;
    const int nb = a.K >> 8;
    const int t0 = blockIdx.x * Y_TOK, row0 = blockIdx.y * Y_ROWS + wave * 16;
    const int nrg = a.nrows_pad >> 3;
    const int rg = (row0 >> 3) + (j >> 3) < nrg ? (row0 >> 3) + (j >> 3) : nrg - 1;      // rows behind the matrix: the last record group again, never stored
    const uint8_t * wrec = a.w + (size_t) rg * nb * RECB;
    const float * wsc = a.sc + ((size_t) rg * nb * 8 + r) * NSC;
    const size_t b16 = BAMD_BLOB16_BYTES(nb);
    // staging plan: 2 NT 16-byte pieces of quants and one block scale (MIN: one {d_x, s_x} pair) per thread and record (tokens behind T: the last token again).
    // NT == 1: the 128 block scales of a stage are taken twice, by threads t and t + 128: the same value to the same address, and no branch in the loop
    const uint8_t * sq[2 * NT]; uint32_t dq[2 * NT];
#pragma unroll
    for (int k = 0; k < 2 * NT; ++k) {
        const int idx = k * 256 + tid, tok = idx >> 5, q = idx & 31;
        const int tg = t0 + tok < a.T ? t0 + tok : a.T - 1;
        sq[k] = a.blob16 + (size_t) tg * b16 + q * 16; dq[k] = (uint32_t) (tok * Y_QSTR + q * 16);
    }
    const uint8_t * sx; uint32_t dx;
    {
        const int tok = NT == 2 ? tid >> 3 : (tid >> 3) & 15, c = tid & 7;
        const int tg = t0 + tok < a.T ? t0 + tok : a.T - 1;
        sx = a.blob16 + (size_t) tg * b16 + 512 + c * 4; dx = (uint32_t) (Y_XD_OFF + (c * Y_TOK + tok) * 4);
    }
    uint4 stq0, stq1, stq2, stq3; float stxd, stxs;            // (named: as an array behind the lambdas' references the four stayed in scratch memory)
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
    // [set][e][pair], set = token tile n (NP == 1) or block parity (NP == 2): tokens 16 n + 4 g + 0..3 of row j.  The chains are WRITTEN as float2 operations (v_pk_fma_f32, an IEEE fma per half): left as scalar
    // fmaf, the eight links an accumulator takes per record become one tree for the SLP vectoriser, which emits it behind the last MFMA of the loop body.
    // summs (MIN): [token tile n][pair]
    bamd_f2 acc[2][8][2], summs[2][2];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { acc[n][e][0] = (bamd_f2) { 0.f, 0.f }; acc[n][e][1] = (bamd_f2) { 0.f, 0.f }; }
        summs[n][0] = (bamd_f2) { 0.f, 0.f }; summs[n][1] = (bamd_f2) { 0.f, 0.f };
    }
    const _Float16 kz = MIN ? (_Float16) -1024.f : TYPE == BAMD_Q8_0 || TYPE == BAMD_IQ4_NL ? (_Float16) -1152.f : TYPE == BAMD_Q4_0 ? (_Float16) -1032.f : (_Float16) -1040.f;
    const bamd_h2q kzero = { kz, kz };
    auto chain = [&](int n, int eh, const bamd_f16v & s, const bamd_f4 & S) {           // the links (l, 4 eh + 0..3) of the lane's four tokens of tile n
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
            for (int k = 0; k < 2 * NT; ++k) {                 // (eh, n) = (k / NT, k % NT); a link's set: the token tile, or (NP == 2) the parity of its block
                const int eh = k / NT, n = k % NT;
                bamd_f16v z;
#pragma unroll
                for (int v = 0; v < 16; ++v) z[v] = 0.f;
                const bamd_f16v s = __builtin_amdgcn_mfma_f32_16x16x4f16(A[n][eh].h, B[eh].h, z, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);             // the MFMA first, the previous one's chain behind it
                if (k > 0) chain(NP == 2 ? cl & 1 : (k - 1) % NT, (k - 1) / NT, prev, S[(k - 1) % NT]);
                else if (cl > 0) chain(NP == 2 ? (cl - 1) & 1 : NT - 1, 1, prev, Sprev);
                if (MIN && k < NT) {                            // step c of the four summs pairs of token tile k: summs += m_w[c] * s_x[c][token]
                    summs[k][0] = __builtin_elementwise_fma(mw, (bamd_f2) { sxv[k][0], sxv[k][1] }, summs[k][0]);
                    summs[k][1] = __builtin_elementwise_fma(mw, (bamd_f2) { sxv[k][2], sxv[k][3] }, summs[k][1]);
                }
                prev = s;
                __builtin_amdgcn_sched_barrier(0);
            }
            Sprev = S[NT - 1];
        }
        chain(1, 1, prev, Sprev);                              // set 1: the last token tile, and the parity of block 4h + 3
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
        const int cn = ci + 1 < nb ? ci + 1 : ci;
        const unsigned char * stage = smem + (ci & 1) * Y_STAGE;
        stage_load(cn);                                        // (no branch inside the loop: the compiler would sink the chains behind it, away from their MFMAs; the last
                                                               //  record is staged once more into the buffer nobody reads again)
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
    if (row >= a.nrows) return;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int t = t0 + 16 * n + 4 * g + i;
#define Y_ACC(e_) (NP == 2 ? acc[0][e_][i >> 1][i & 1] + acc[1][e_][i >> 1][i & 1] : acc[n][e_][i >> 1][i & 1])                          /* NP == 2: accum1 + accum2, lane e */
            const float tree = ((Y_ACC(0) + Y_ACC(4)) + (Y_ACC(2) + Y_ACC(6))) + ((Y_ACC(1) + Y_ACC(5)) + (Y_ACC(3) + Y_ACC(7)));      // b32_finish_row's tree
#undef Y_ACC
            const float val = MIN ? tree + summs[n][i >> 1][i & 1] : tree;                                                             // b32_finish_row<MIN>
            if (t < a.T) {
                const size_t o = (size_t) t * a.ldo + row;
                a.out[o] = EPI == BAMD_EPI_ADD ? val + a.res[o] : EPI == BAMD_EPI_SILU_MUL ? v_silu(a.res[o]) * val : val;
            }
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------
size_t bamd_prefill_aux_bytes_b32(int type, int nrows_pad, int K) { return (size_t) (nrows_pad >> 3) * (size_t) (K >> 8) * (bamd_is_q1(type) ? 512 : 256); }
void bamd_launch_prefill_aux_b32(const void * w_stream, int type, int nrows_pad, int K, void * aux, hipStream_t s) {
    const dim3 grid(K >> 8, nrows_pad >> 3);
    if (type == BAMD_IQ4_NL) type = BAMD_Q4_0;                 // the record is the Q4_0 record: the same table at the same offsets
    with_const(consts<BAMD_Q8_0, BAMD_Q4_0, BAMD_Q5_0, BAMD_Q4_1, BAMD_Q5_1>(), type, [&](auto T) -> bool {
        hipLaunchKernelGGL((prefill_aux_b32_kernel<decltype(T)::value>), grid, dim3(b32_has_min(decltype(T)::value) ? 128 : 64), 0, s, (const uint8_t *) w_stream, K >> 8, (float *) aux);
        return true; });
}
// the launch interface of bamd_launch_matmul_mfma2, which checks the arguments and routes the six types here; the grid follows the type's tile
int bamd_launch_matmul_mfma_b32(const void * w_stream, const void * aux, int type, int nrows, int nrows_pad, int K, const void * blob16, int T, float * out, const float * res,
                                int epi, int ldo, hipStream_t s) {
    if (!bamd_is_b32(type) || T < 1 || nrows_pad < 8 || K < 256) return 1;
    bamd_mma_b32_args a; a.w = (const uint8_t *) w_stream; a.sc = (const float *) aux; a.out = out; a.res = res; a.blob16 = (const uint8_t *) blob16;
    a.K = K; a.T = T; a.nrows = nrows; a.nrows_pad = nrows_pad; a.ldo = ldo;
    with_const(consts<BAMD_Q8_0, BAMD_Q4_0, BAMD_Q5_0, BAMD_Q4_1, BAMD_Q5_1, BAMD_IQ4_NL>(), type, [&](auto TY) -> bool {
        constexpr int TYPE_ = decltype(TY)::value;
        const dim3 grid((T + YTile<TYPE_>::TOK - 1) / YTile<TYPE_>::TOK, (nrows_pad + Y_ROWS - 1) / Y_ROWS);
        return with_const(consts<BAMD_EPI_ADD, BAMD_EPI_SILU_MUL, BAMD_EPI_STORE>(), epi, [&](auto E) -> bool {
            hipLaunchKernelGGL((matmul_mfma_b32_kernel<TYPE_, decltype(E)::value>), grid, dim3(256), 0, s, a);
            return true; }); });
    return 0;
}
