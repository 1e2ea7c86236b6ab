// bamd_prefill2_q1.hip — the exact matrix-core prompt mat-mul for Q4_1 / Q5_1 weights x Q8_1 activations, behind the switch BAMD_PREFILL_Q1 /
// bamd_set_prefill_q1 (default off; the list of types is bamd_prefill_mfma_type, bamd_kernels.h).  A sibling of matmul_mfma_q0_kernel (bamd_prefill2_q0.hip):
// the same instruction, tiling, LDS staging and MFMA / chain interleave; read that file's header for the lane maps and why the K = 4 form fits.
//
// Arithmetic: the contract of bamd_q1_device.h.  One output = TWO accumulators over the 32-weight blocks l in order:
//     acc_e = fma(f32(d_w) * f32(d_x), (float) dot4_e, acc_e),  e = 0..7     the 8-lane chain of the Q8_0 family, here with UNSIGNED weights without an offset
//                                                                            (Q4_1: the nibble 0..15, Q5_1: nibble | bit << 4, 0..31): the B operand is
//                                                                            (0x6400 | u) - 1024 = u, exact in f16; |w| <= 31, |x| <= 127: every four-term sum is
//                                                                            an integer far below 2^24, exact in f32 in any order
//     summs = summs + f32(m_w) * f32(s_x)                                    one scalar chain per (row, token).  The product of two widened f16 is exact in f32,
//                                                                            so a multiply and an add give the bits of one fma; the K/32 steps stay in block order
// and the result is q0_finish_row's tree over acc_e, plus summs.
// What differs from the Q0 kernel:
//   * the lane (row j, tokens 16 n + 4 g + 0..3) carries eight summs accumulators next to its 64 chain accumulators.  Per block it takes ONE step of each, written
//     as two-wide vector fmas (v_pk_fma_f32, an IEEE fma per half) whose only operand that changes is the accumulator itself: the order of a summs chain is its
//     data dependence, block c + 1 after block c, and there is no scalar f32 add for the SLP vectoriser to gather into a tree;
//   * side table: the row's eight f16 d AND eight f16 m of every record widened to f32, [record group][record][row r][d 0..7 | m 0..7] — 64 B per row and 256
//     weights, four 16-byte loads per lane and record;
//   * f16 activation records (quantize_batch_q1_kernel, bamd_prefill_q1.hip): the Q8_0 form's 512 B of quants and eight f32 d_x at byte 512, then the eight s_x
//     widened to f32 at byte 544 (576 of the BAMD_B16_REC bytes used); d_x and s_x of a stage sit side by side in LDS, [block c][token].
#include "bamd_q1_device.h"
#include "bamd_mfma_common.h"

typedef float bamd_f16v __attribute__((ext_vector_type(16)));
typedef float bamd_f2 __attribute__((ext_vector_type(2)));
typedef _Float16 bamd_h2q __attribute__((ext_vector_type(2)));
union bamd_h2qu { uint32_t u; bamd_h2q h; };

#define Z_TOK 32                                           /* tokens of a workgroup */
#define Z_ROWS 64                                          /* rows of a workgroup: four waves x 16 */
#define Z_QSTR 528                                         /* LDS bytes between the quants of consecutive tokens (bamd_prefill2_q0.hip) */
#define Z_XD_OFF (Z_TOK * Z_QSTR)                          /* d_x of the stage: [block c][token] f32 */
#define Z_XS_OFF (Z_XD_OFF + 8 * Z_TOK * 4)                /* s_x of the stage, the same shape */
#define Z_STAGE (Z_XS_OFF + 8 * Z_TOK * 4)                 /* 18 944 B */

static_assert(BAMD_B16_REC >= 512 + 32 + 32, "the f16 activation record holds the quants, eight d_x and eight s_x");

struct bamd_mmaq1_args {
    const uint8_t * w;               // wave-stream records (bamd_formats.h)
    const float * sc;                // side table: [record group][record][row r][d of block 0..7 | m of block 0..7] f32
    float * out; const float * res;  // [T][ldo]
    const uint8_t * blob16;          // f16 activation records (quantize_batch_q1_kernel)
    int K, T, nrows, nrows_pad, ldo;
};

// grid (records, record groups), 128 threads = (row r, d of block 0..7 | m of block 0..7): the record's dm table is in this order already
template <int TYPE>
__global__ void __launch_bounds__(128) prefill_aux_q1_kernel(const uint8_t * __restrict__ w, int nb, float * __restrict__ sc) {
    constexpr int RECB = BAMD_RECB_OF(TYPE), DMO = TYPE == BAMD_Q4_1 ? 1024 : 1280;
    const size_t rec = (size_t) blockIdx.y * nb + blockIdx.x;
    sc[rec * 128 + threadIdx.x] = h2f(*(const unsigned short *) (w + rec * RECB + DMO + threadIdx.x * 2));
}

// the lane's pieces of HALF a record (blocks c = 4h .. 4h+3) for its two chunks e = g and g + 4, which share the nibble bytes: low / high nibbles
template <int TYPE> struct HalfQ1 { uint4 q; uint32_t qh[2]; };
template <int TYPE> __device__ __forceinline__ void load_half(HalfQ1<TYPE> & H, const uint8_t * rec, int h, int r, int g) {
    H.q = *(const uint4 *) (rec + (r * 4 + g) * 32 + h * 16);
    if (TYPE == BAMD_Q5_1) { H.qh[0] = *(const uint32_t *) (rec + 1024 + (r * 8 + g) * 4); H.qh[1] = *(const uint32_t *) (rec + 1024 + (r * 8 + g + 4) * 4); }
}
// the four weights of block 4h + cl, chunk 4 eh + g: q1_weights' bytes, unsigned and without an offset
template <int TYPE> __device__ __forceinline__ uint32_t half_bytes(const HalfQ1<TYPE> & H, int h, int cl, int eh) {
    const uint32_t nib = (BAMD_Q0_COMP(H.q, cl) >> (eh * 4)) & 0x0f0f0f0fu;
    if (TYPE == BAMD_Q4_1) return nib;
    return nib | (((H.qh[eh] >> (4 * h + cl)) & 0x01010101u) << 4);
}

template <int TYPE, int EPI>
__global__ void __launch_bounds__(256) matmul_mfma_q1_kernel(bamd_mmaq1_args a) {
    constexpr int RECB = BAMD_RECB_OF(TYPE);
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * Z_STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4, r = j & 7;
    const int nb = a.K >> 8;
    const int t0 = blockIdx.x * Z_TOK, row0 = blockIdx.y * Z_ROWS + wave * 16;
    const int nrg = a.nrows_pad >> 3;
    const int rg = (row0 >> 3) + (j >> 3) < nrg ? (row0 >> 3) + (j >> 3) : nrg - 1;      // rows behind the matrix: the last record group again, never stored
    const uint8_t * wrec = a.w + (size_t) rg * nb * RECB;
    const float * wsc = a.sc + ((size_t) rg * nb * 8 + r) * 16;
    const size_t b16 = BAMD_BLOB16_BYTES(nb);
    // staging plan: four 16-byte pieces of quants and one {d_x, s_x} pair per thread and record (tokens behind T: the last token again)
    const uint8_t * sq[4]; uint32_t dq[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int idx = k * 256 + tid, tok = idx >> 5, q = idx & 31;
        const int tg = t0 + tok < a.T ? t0 + tok : a.T - 1;
        sq[k] = a.blob16 + (size_t) tg * b16 + q * 16; dq[k] = (uint32_t) (tok * Z_QSTR + q * 16);
    }
    const uint8_t * sx; uint32_t dx;
    {
        const int tok = tid >> 3, c = tid & 7;
        const int tg = t0 + tok < a.T ? t0 + tok : a.T - 1;
        sx = a.blob16 + (size_t) tg * b16 + 512 + c * 4; dx = (uint32_t) (Z_XD_OFF + (c * Z_TOK + tok) * 4);
    }
    uint4 stq0, stq1, stq2, stq3; float stxd, stxs;
    auto stage_load = [&](int ci) {
        const size_t o = (size_t) ci * BAMD_B16_REC;
        stq0 = *(const uint4 *) (sq[0] + o); stq1 = *(const uint4 *) (sq[1] + o); stq2 = *(const uint4 *) (sq[2] + o); stq3 = *(const uint4 *) (sq[3] + o);
        stxd = *(const float *) (sx + o); stxs = *(const float *) (sx + o + 32);
    };
    auto stage_store = [&](int buf) {
        unsigned char * d = smem + buf * Z_STAGE;
        *(uint4 *) (d + dq[0]) = stq0; *(uint4 *) (d + dq[1]) = stq1; *(uint4 *) (d + dq[2]) = stq2; *(uint4 *) (d + dq[3]) = stq3;
        *(float *) (d + dx) = stxd; *(float *) (d + dx + (Z_XS_OFF - Z_XD_OFF)) = stxs;
    };
    // [token tile n][e][pair]: tokens 16 n + 4 g + 0..3 of row j; float2 operations, as in the Q0 kernel.  summs: [token tile n][pair]
    bamd_f2 acc[2][8][2], summs[2][2];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { acc[n][e][0] = (bamd_f2) { 0.f, 0.f }; acc[n][e][1] = (bamd_f2) { 0.f, 0.f }; }
        summs[n][0] = (bamd_f2) { 0.f, 0.f }; summs[n][1] = (bamd_f2) { 0.f, 0.f };
    }
    const bamd_h2q kzero = { (_Float16) -1024.f, (_Float16) -1024.f };
    auto chain = [&](int n, int eh, const bamd_f16v & s, const bamd_f4 & S) {           // the links (l, 4 eh + 0..3) of the lane's four tokens of tile n
        const bamd_f2 Slo = { S[0], S[1] }, Shi = { S[2], S[3] };
#define Z_LINK(blk_) do { \
            acc[n][4 * eh + blk_][0] = __builtin_elementwise_fma(Slo, __builtin_shufflevector(s, s, 4 * blk_, 4 * blk_ + 1), acc[n][4 * eh + blk_][0]); \
            acc[n][4 * eh + blk_][1] = __builtin_elementwise_fma(Shi, __builtin_shufflevector(s, s, 4 * blk_ + 2, 4 * blk_ + 3), acc[n][4 * eh + blk_][1]); } while (0)
        Z_LINK(0); Z_LINK(1); Z_LINK(2); Z_LINK(3);
#undef Z_LINK
    };
    // half step: blocks c = 4h .. 4h+3 of a record whose activations are in `stage`; dm: the row's d (0..7) and m (8..15) of the record
    auto half_step = [&](const HalfQ1<TYPE> & H, int h, const float (&dm)[16], const unsigned char * stage) {
        const unsigned char * aq = stage + j * Z_QSTR + g * 16;
        const unsigned char * xd = stage + Z_XD_OFF + g * 16;
        bamd_f16v prev; bamd_f4 Sprev;
#pragma unroll
        for (int cl = 0; cl < 4; ++cl) {
            const int c = 4 * h + cl;
            bamd_f4 S[2], sxv[2];
            union { uint2 u; bamd_h4 h; } A[2][2], B[2];
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const bamd_f4 x = *(const bamd_f4 *) (xd + (c * Z_TOK + 16 * n) * 4);
                sxv[n] = *(const bamd_f4 *) (xd + (Z_XS_OFF - Z_XD_OFF) + (c * Z_TOK + 16 * n) * 4);
#pragma unroll
                for (int i = 0; i < 4; ++i) S[n][i] = dm[c] * x[i];
                const uint4 av = *(const uint4 *) (aq + n * (16 * Z_QSTR) + c * 64);
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
            const bamd_f2 mw = { dm[8 + c], dm[8 + c] };
#pragma unroll
            for (int k = 0; k < 4; ++k) {                      // (eh, n) = (k >> 1, k & 1)
                const int eh = k >> 1, n = k & 1;
                bamd_f16v z;
#pragma unroll
                for (int v = 0; v < 16; ++v) z[v] = 0.f;
                const bamd_f16v s = __builtin_amdgcn_mfma_f32_16x16x4f16(A[n][eh].h, B[eh].h, z, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);             // the MFMA first, the previous one's chain behind it
                if (k > 0) chain((k - 1) & 1, (k - 1) >> 1, prev, S[(k - 1) & 1]);
                else if (cl > 0) chain(1, 1, prev, Sprev);
                if (k < 2) {                                   // step c of the four summs pairs of token tile k: summs += m_w[c] * s_x[c][token]
                    summs[k][0] = __builtin_elementwise_fma(mw, (bamd_f2) { sxv[k][0], sxv[k][1] }, summs[k][0]);
                    summs[k][1] = __builtin_elementwise_fma(mw, (bamd_f2) { sxv[k][2], sxv[k][3] }, summs[k][1]);
                }
                prev = s;
                __builtin_amdgcn_sched_barrier(0);
            }
            Sprev = S[1];
        }
        chain(1, 1, prev, Sprev);
    };
    HalfQ1<TYPE> H0, H1;
    float dm[16], dmn[16];
    auto load_dm = [&](float (&d)[16], int ci) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bamd_f4 v = *(const bamd_f4 *) (wsc + (size_t) ci * 128 + 4 * q);
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
        const unsigned char * stage = smem + (ci & 1) * Z_STAGE;
        stage_load(cn);                                        // (no branch inside the loop; the last record is staged once more into the buffer nobody reads again)
        load_half(H1, wrec + (size_t) ci * RECB, 1, r, g);
        load_dm(dmn, cn);
        __builtin_amdgcn_sched_barrier(0);
        half_step(H0, 0, dm, stage);
        load_half(H0, wrec + (size_t) cn * RECB, 0, r, g);
        __builtin_amdgcn_sched_barrier(0);
        half_step(H1, 1, dm, stage);
#pragma unroll
        for (int i = 0; i < 16; ++i) dm[i] = dmn[i];
        stage_store((ci + 1) & 1);                             // the buffer read in step ci - 1: every wave is past that step's barrier
        __syncthreads();
    }
    const int row = row0 + j;
    if (row >= a.nrows) return;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int t = t0 + 16 * n + 4 * g + i;
#define Z_ACC(e_) acc[n][e_][i >> 1][i & 1]
            const float tree = ((Z_ACC(0) + Z_ACC(4)) + (Z_ACC(2) + Z_ACC(6))) + ((Z_ACC(1) + Z_ACC(5)) + (Z_ACC(3) + Z_ACC(7)));      // q0_finish_row's tree
#undef Z_ACC
            const float val = tree + summs[n][i >> 1][i & 1];                                                                          // q1_finish_row
            if (t < a.T) {
                const size_t o = (size_t) t * a.ldo + row;
                a.out[o] = EPI == BAMD_EPI_ADD ? val + a.res[o] : EPI == BAMD_EPI_SILU_MUL ? v_silu(a.res[o]) * val : val;
            }
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------
size_t bamd_prefill_aux_bytes_q1(int nrows_pad, int K) { return (size_t) (nrows_pad >> 3) * (size_t) (K >> 8) * 512; }
void bamd_launch_prefill_aux_q1(const void * w_stream, int type, int nrows_pad, int K, void * aux, hipStream_t s) {
    const dim3 grid(K >> 8, nrows_pad >> 3);
    if (type == BAMD_Q4_1) hipLaunchKernelGGL((prefill_aux_q1_kernel<BAMD_Q4_1>), grid, dim3(128), 0, s, (const uint8_t *) w_stream, K >> 8, (float *) aux);
    else                   hipLaunchKernelGGL((prefill_aux_q1_kernel<BAMD_Q5_1>), grid, dim3(128), 0, s, (const uint8_t *) w_stream, K >> 8, (float *) aux);
}
// the launch interface of bamd_launch_matmul_mfma2, which checks the arguments and routes the two types here
int bamd_launch_matmul_mfma_q1(const void * w_stream, const void * aux, int type, int nrows, int nrows_pad, int K, const void * blob16, int T, float * out, const float * res,
                               int epi, int ldo, hipStream_t s) {
    if (!bamd_is_q1(type) || T < 1 || nrows_pad < 8) return 1;
    bamd_mmaq1_args a; a.w = (const uint8_t *) w_stream; a.sc = (const float *) aux; a.out = out; a.res = res; a.blob16 = (const uint8_t *) blob16;
    a.K = K; a.T = T; a.nrows = nrows; a.nrows_pad = nrows_pad; a.ldo = ldo;
    const dim3 grid((T + Z_TOK - 1) / Z_TOK, (nrows_pad + Z_ROWS - 1) / Z_ROWS);
#define Z_LAUNCH(TYPE_) do { \
        if (epi == BAMD_EPI_ADD)           hipLaunchKernelGGL((matmul_mfma_q1_kernel<TYPE_, BAMD_EPI_ADD>),      grid, dim3(256), 0, s, a); \
        else if (epi == BAMD_EPI_SILU_MUL) hipLaunchKernelGGL((matmul_mfma_q1_kernel<TYPE_, BAMD_EPI_SILU_MUL>), grid, dim3(256), 0, s, a); \
        else                               hipLaunchKernelGGL((matmul_mfma_q1_kernel<TYPE_, BAMD_EPI_STORE>),    grid, dim3(256), 0, s, a); } while (0)
    if (type == BAMD_Q4_1) Z_LAUNCH(BAMD_Q4_1);
    else                   Z_LAUNCH(BAMD_Q5_1);
#undef Z_LAUNCH
    return 0;
}
