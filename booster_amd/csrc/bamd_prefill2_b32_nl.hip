// bamd_prefill2_b32_nl.hip — the exact matrix-core prompt mat-mul for IQ4_NL weights x Q8_0 activations, behind the switch BAMD_PREFILL_NL / bamd_set_prefill_nl
// (default off; the list of types is bamd_prefill_mfma_type, bamd_prefill_family.h).  A sibling of matmul_mfma_b32_kernel (bamd_prefill2_b32.hip) in a translation unit of
// its own, so that kernel's five instances stay instruction for instruction what they are; read that file's header first: the instruction
// (v_mfma_f32_16x16x4_4b_f16), the lane maps, the f16 operand images, the weights from the wave stream straight into registers, the activations through the
// double-buffered LDS stage, the links on the VALU as v_pk_fma_f32 and one MFMA's chain behind the next MFMA's issue are the same here.
//
// Arithmetic: the IQ4_NL contract of bamd_b32_device.h.  One output = TWO sets of eight f32 chains over the 32-weight blocks l in order,
//     acc[l & 1]_e = fma(f32(d_w) * f32(d_x), (float) dot4_e, acc[l & 1]_e),     dot4_e = the dot of kvalues_iq4nl[nibble] with bytes 4e .. 4e+3 of the activation block,
// closed by a_e = acc[0]_e + acc[1]_e and b32_finish_row's tree over a_e.  A record is eight consecutive blocks, so l & 1 = c & 1 with c the block's index in the
// record: a compile-time index of the unrolled half step, the choice of the set costs no instruction.
// Weight operand: the nibble dword through b32_iq4nl_values (bamd_b32_device.h, the one place the table stands), ^ 0x80808080 gives u = value + 128 (1 .. 241),
// and (0x6400 | u) - 1152 is the table value, exact in f16 — the Q8_0 instance's constant.  |w| <= 127, |x| <= 127: every product and every four-term sum is an
// integer <= 64 516 < 2^24, exact in f32 in any order.
//
// Tile.  Two accumulators per output at the sibling's 16-row x 32-token wave tile would be 128 registers, the shape that kernel's header records as spilling.  Here a
// wave owns 16 rows x ONE token tile of 16 with all eight e and both parities: 64 accumulator registers, as there.  A workgroup is four waves = 64 rows x 16 tokens.
// The other way to place four such waves, 32 rows x 32 tokens, gives each wave the same instruction stream (its own 16 x 16 tile: one weight unpack, one LDS read
// and two MFMAs per block either way); the two differ only on the memory side:
//   * weight re-reads: 64 x 16 walks the matrix once per 16-token tile (T / 16 passes out of L2), 32 x 32 once per 32 tokens but with two waves of a workgroup
//     requesting the same lines;
//   * LDS per stage: 16 tokens = 8 960 B against 32 tokens = 17 920 B, and half the staging requests per thread and record (two 16-byte pieces, not four).
// 64 x 16 was chosen: every weight line is requested by exactly one wave of a workgroup, the stage is half the size, and the row / record-group arithmetic (ragged
// rows included) is the sibling's unchanged.  The 32 x 32 placement was not built; no measurement compares them.
// Side table: the Q4_0 one (the record IS the Q4_0 record): the row's eight f16 d of a record widened to f32, [record group][record][row][block], 32 B per row and
// 256 weights, written by prefill_aux_b32_kernel<BAMD_Q4_0>.  Activations: the f16 Q8_0 records of quantize_batch_b32_kernel, unchanged.
#include "bamd_b32_device.h"
#include "bamd_mfma_common.h"
#include "bamd_mv_select.h"

typedef float bamd_f16v __attribute__((ext_vector_type(16)));
typedef float bamd_f2 __attribute__((ext_vector_type(2)));
typedef _Float16 bamd_h2q __attribute__((ext_vector_type(2)));
union bamd_h2qu { uint32_t u; bamd_h2q h; };

#define N_TOK 16                                           /* tokens of a workgroup: one token tile */
#define N_ROWS 64                                          /* rows of a workgroup: four waves x 16 */
#define N_QSTR 528                                         /* LDS bytes between the quants of consecutive tokens (132 dwords = 4 mod 64, as in the sibling) */
#define N_XD_OFF (N_TOK * N_QSTR)                          /* d_x of the stage: [block c][token] f32 */
#define N_STAGE (N_XD_OFF + 8 * N_TOK * 4)                 /* 8 960 B */
static_assert(BAMD_B16_REC >= 512 + 32, "the f16 activation record holds the quants and eight d_x");

struct bamd_mma_nl_args {
    const uint8_t * w;               // wave-stream records (bamd_formats.h: the Q4_0 record)
    const float * sc;                // side table: [record group][record][row r][block c] f32
    float * out; const float * res;  // [T][ldo]
    const uint8_t * blob16;          // f16 activation records (quantize_batch_b32_kernel)
    int K, T, nrows, nrows_pad, ldo;
};

template <int EPI>
__global__ void __launch_bounds__(256) matmul_mfma_b32_nl_kernel(bamd_mma_nl_args a) {
    constexpr int RECB = BAMD_RECB_OF(BAMD_IQ4_NL);
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * N_STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4, r = j & 7;
    const int nb = a.K >> 8;
    const int t0 = blockIdx.x * N_TOK, row0 = blockIdx.y * N_ROWS + wave * 16;
    const int nrg = a.nrows_pad >> 3;
    const int rg = (row0 >> 3) + (j >> 3) < nrg ? (row0 >> 3) + (j >> 3) : nrg - 1;      // rows behind the matrix: the last record group again, never stored
    const uint8_t * wrec = a.w + (size_t) rg * nb * RECB;
    const float * wsc = a.sc + ((size_t) rg * nb * 8 + r) * 8;
    const size_t b16 = BAMD_BLOB16_BYTES(nb);
    // staging plan: two 16-byte pieces of quants and one block scale per thread and record (tokens behind T: the last token again).  The 128 block scales of a stage
    // are taken twice, by threads t and t + 128: the same value to the same address, and no branch in the loop
    const uint8_t * sq[2]; uint32_t dq[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int idx = k * 256 + tid, tok = idx >> 5, q = idx & 31;
        const int tg = t0 + tok < a.T ? t0 + tok : a.T - 1;
        sq[k] = a.blob16 + (size_t) tg * b16 + q * 16; dq[k] = (uint32_t) (tok * N_QSTR + q * 16);
    }
    const uint8_t * sx; uint32_t dx;
    {
        const int tok = (tid >> 3) & 15, c = tid & 7;
        const int tg = t0 + tok < a.T ? t0 + tok : a.T - 1;
        sx = a.blob16 + (size_t) tg * b16 + 512 + c * 4; dx = (uint32_t) (N_XD_OFF + (c * N_TOK + tok) * 4);
    }
    uint4 stq0, stq1; float stxd;
    auto stage_load = [&](int ci) {
        const size_t o = (size_t) ci * BAMD_B16_REC;
        stq0 = *(const uint4 *) (sq[0] + o); stq1 = *(const uint4 *) (sq[1] + o);
        stxd = *(const float *) (sx + o);
    };
    auto stage_store = [&](int buf) {
        unsigned char * d = smem + buf * N_STAGE;
        *(uint4 *) (d + dq[0]) = stq0; *(uint4 *) (d + dq[1]) = stq1;
        *(float *) (d + dx) = stxd;
    };
    // [block parity p][e][pair]: tokens 4 g + 0..3 of row j.  Written as float2 operations (v_pk_fma_f32, an IEEE fma per half), as in the sibling: left as scalar fmaf,
    // the links an accumulator takes per record become one tree for the SLP vectoriser
    bamd_f2 acc[2][8][2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { acc[p][e][0] = (bamd_f2) { 0.f, 0.f }; acc[p][e][1] = (bamd_f2) { 0.f, 0.f }; }
    }
    const bamd_h2q kzero = { (_Float16) -1152.f, (_Float16) -1152.f };
    auto chain = [&](int p, int eh, const bamd_f16v & s, const bamd_f4 & S) {           // the links (l, 4 eh + 0..3) of the lane's four tokens, l of parity p
        const bamd_f2 Slo = { S[0], S[1] }, Shi = { S[2], S[3] };
#define N_LINK(blk_) do { \
            acc[p][4 * eh + blk_][0] = __builtin_elementwise_fma(Slo, __builtin_shufflevector(s, s, 4 * blk_, 4 * blk_ + 1), acc[p][4 * eh + blk_][0]); \
            acc[p][4 * eh + blk_][1] = __builtin_elementwise_fma(Shi, __builtin_shufflevector(s, s, 4 * blk_ + 2, 4 * blk_ + 3), acc[p][4 * eh + blk_][1]); } while (0)
        N_LINK(0); N_LINK(1); N_LINK(2); N_LINK(3);
#undef N_LINK
    };
    // half step: blocks c = 4h .. 4h+3 of a record whose activations are in `stage`; H: the lane's 16 bytes of nibbles of those blocks (chunks g and g + 4 share
    // them: low / high nibbles); d: the row's eight d of the record.  Block c = 4h + cl has parity cl & 1
    auto half_step = [&](const uint4 & H, int h, const float (&d)[8], const unsigned char * stage) {
        const unsigned char * aq = stage + j * N_QSTR + g * 16;
        const unsigned char * xd = stage + N_XD_OFF + g * 16;
        bamd_f16v prev; bamd_f4 Sprev;
#pragma unroll
        for (int cl = 0; cl < 4; ++cl) {
            const int c = 4 * h + cl;
            bamd_f4 S;
            union { uint2 u; bamd_h4 h; } A[2], B[2];
            const bamd_f4 x = *(const bamd_f4 *) (xd + c * N_TOK * 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) S[i] = d[c] * x[i];
            const uint4 av = *(const uint4 *) (aq + c * 64);
            A[0].u = (uint2) { av.x, av.y }; A[1].u = (uint2) { av.z, av.w };
#pragma unroll
            for (int eh = 0; eh < 2; ++eh) {
                const uint32_t u = b32_iq4nl_values((BAMD_B32_COMP(H, cl) >> (eh * 4)) & 0x0f0f0f0fu) ^ 0x80808080u;
                bamd_h2qu lo, hi;
                lo.u = __builtin_amdgcn_perm(0x64646464u, u, 0x04010400u); lo.h = lo.h + kzero;
                hi.u = __builtin_amdgcn_perm(0x64646464u, u, 0x04030402u); hi.h = hi.h + kzero;
                B[eh].u = (uint2) { lo.u, hi.u };
            }
#pragma unroll
            for (int eh = 0; eh < 2; ++eh) {
                bamd_f16v z;
#pragma unroll
                for (int v = 0; v < 16; ++v) z[v] = 0.f;
                const bamd_f16v s = __builtin_amdgcn_mfma_f32_16x16x4f16(A[eh].h, B[eh].h, z, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);             // the MFMA first, the previous one's chain behind it
                if (eh > 0) chain(cl & 1, 0, prev, S);
                else if (cl > 0) chain((cl - 1) & 1, 1, prev, Sprev);
                prev = s;
                __builtin_amdgcn_sched_barrier(0);
            }
            Sprev = S;
        }
        chain(1, 1, prev, Sprev);
    };
    uint4 H0, H1;
    float dw[8], dwn[8];
    auto load_half = [&](uint4 & H, const uint8_t * rec, int h) { H = *(const uint4 *) (rec + (r * 4 + g) * 32 + h * 16); };
    auto load_dw = [&](float (&d)[8], int ci) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const bamd_f4 v = *(const bamd_f4 *) (wsc + (size_t) ci * 64 + 4 * q);
#pragma unroll
            for (int i = 0; i < 4; ++i) d[4 * q + i] = v[i];
        }
    };
    stage_load(0);
    load_half(H0, wrec, 0);
    load_dw(dw, 0);
    stage_store(0);
    __syncthreads();
    for (int ci = 0; ci < nb; ++ci) {
        const int cn = ci + 1 < nb ? ci + 1 : ci;
        const unsigned char * stage = smem + (ci & 1) * N_STAGE;
        stage_load(cn);                                        // (no branch inside the loop; the last record is staged once more into the buffer nobody reads again)
        load_half(H1, wrec + (size_t) ci * RECB, 1);
        load_dw(dwn, cn);
        __builtin_amdgcn_sched_barrier(0);
        half_step(H0, 0, dw, stage);
        load_half(H0, wrec + (size_t) cn * RECB, 0);
        __builtin_amdgcn_sched_barrier(0);
        half_step(H1, 1, dw, stage);
#pragma unroll
        for (int i = 0; i < 8; ++i) dw[i] = dwn[i];
        stage_store((ci + 1) & 1);                             // the buffer read in step ci - 1: every wave is past that step's barrier
        __syncthreads();
    }
    const int row = row0 + j;
    if (row >= a.nrows) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = t0 + 4 * g + i;
#define N_ACC(e_) (acc[0][e_][i >> 1][i & 1] + acc[1][e_][i >> 1][i & 1])                                                                  /* accum1 + accum2, lane e */
        const float val = ((N_ACC(0) + N_ACC(4)) + (N_ACC(2) + N_ACC(6))) + ((N_ACC(1) + N_ACC(5)) + (N_ACC(3) + N_ACC(7)));               // b32_finish_row's tree
#undef N_ACC
        if (t < a.T) {
            const size_t o = (size_t) t * a.ldo + row;
            a.out[o] = EPI == BAMD_EPI_ADD ? val + a.res[o] : EPI == BAMD_EPI_SILU_MUL ? v_silu(a.res[o]) * val : val;
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------
// behind bamd_launch_matmul_mfma_b32 (bamd_prefill2_b32.hip), which bamd_launch_matmul_mfma2 calls after it checked the arguments
int bamd_launch_matmul_mfma_b32_nl(const void * w_stream, const void * aux, int nrows, int nrows_pad, int K, const void * blob16, int T, float * out, const float * res, int epi,
                                   int ldo, hipStream_t s) {
    if (T < 1 || nrows_pad < 8 || K < 256) return 1;
    bamd_mma_nl_args a; a.w = (const uint8_t *) w_stream; a.sc = (const float *) aux; a.out = out; a.res = res; a.blob16 = (const uint8_t *) blob16;
    a.K = K; a.T = T; a.nrows = nrows; a.nrows_pad = nrows_pad; a.ldo = ldo;
    const dim3 grid((T + N_TOK - 1) / N_TOK, (nrows_pad + N_ROWS - 1) / N_ROWS);
    if (epi == BAMD_EPI_ADD)           hipLaunchKernelGGL((matmul_mfma_b32_nl_kernel<BAMD_EPI_ADD>),      grid, dim3(256), 0, s, a);
    else if (epi == BAMD_EPI_SILU_MUL) hipLaunchKernelGGL((matmul_mfma_b32_nl_kernel<BAMD_EPI_SILU_MUL>), grid, dim3(256), 0, s, a);
    else                               hipLaunchKernelGGL((matmul_mfma_b32_nl_kernel<BAMD_EPI_STORE>),    grid, dim3(256), 0, s, a);
    return 0;
}
