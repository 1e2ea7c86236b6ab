// bamd_prefill2_flt.hip — the exact matrix-core prompt mat-mul for F32 / F16 weights x f32 activations, behind the switch BAMD_PREFILL_FLT=1 /
// bamd_set_prefill_flt (default off; the families and their switches: bamd_prefill_family.h).  BF16 weights have a kernel and a switch of their own (bamd_prefill2_bf16.hip, BAMD_PREFILL_BF16): their chain
// is add(mul(w, x), c) with two roundings, which an fma chain restates only where every product is exact in f32 — that kernel proves it from exponent ranges.
//
// Arithmetic: the contract of bamd_flt_device.h.  One output = ONE 8-lane accumulator, lane j: acc_j = fmaf(w[8i + j], x[8i + j], acc_j) for i = 0 .. K/8 - 1,
// then hsum8_tinyblas' tree over the eight lanes.  v_mfma_f32_16x16x4_f32 is the sequential chain D = fma(a3, b3, fma(a2, b2, fma(a1, b1, fma(a0, b0, C))))
// (tools/mfma_f32_probe.hip; the P.V pass of bamd_attention_mfma.hip runs the same tinyBLAS chain on it), it never flushes C or D, and its f32 A / B inputs keep
// subnormals in the kernels' default mode.  So a 16 x 16 output tile is EIGHT accumulator tiles, one per j, and MFMA step s of tile j takes k = 32 s + 8 kk + j for
// kk = 0..3: the steps i = 4 s .. 4 s + 3 of lane j's chain, in order, chained through C.  No split over K; the eight tiles are summed element-wise in the tree
// ((c0 + c4) + (c2 + c6)) + ((c1 + c5) + (c3 + c7)) after the last step.  F16 weights are widened (exactly) on their way into LDS; activations are never rounded.
//
// Layout.  Lane maps of the instruction: A lane = (row m = lane & 15, kk = lane >> 4), B lane = (kk, token n = lane & 15), D register v of a lane = row 4 kk + v of
// token n.  Both operands are staged in LDS in the order [row or token][step s][j][kk], 132 dwords per row and 128 of K:
//   * that is the order the data lies in already.  Wave-stream lane (r, j) of a record (bamd_formats.h) holds, in request q, the four (F16: eight) chain steps
//     i = 4 q .. of its row: one 16-byte piece = the four kk of (row r, step s = q, tile j), stored with one ds_write_b128 (F16: two, widened).  The activation
//     rows of act_batch_flt_kernel are in the same [s][j][kk] order (bamd_flt_device.h): they are copied as they are.  No side table, no second activation pass;
//   * an MFMA lane reads its operand of (s, j) as one dword at row * 132 + s * 32 + j * 4 + kk: the 64 lanes of a read fall on the 64 banks (4 m + kk), and the
//     eight j of a step are eight reads 16 bytes apart (ds_read2_b32 pairs).
// A workgroup is four waves = 64 rows x 64 tokens, a wave owns 32 rows x 32 tokens = 2 x 2 tiles x 8 j = 32 accumulator tiles, 128 registers.  Per 128 of K the
// next chunk travels global -> registers while the MFMAs of this one run, then registers -> the other LDS buffer, one barrier per chunk.  Consecutive MFMAs always
// write different accumulators: an accumulator is revisited after 31 others (the dependent latency is 40 cycles against a 32-cycle issue).
#include "bamd_flt_device.h"
#include "bamd_kernels.h"
#include "bamd_mfma_common.h"
#include "bamd_mv_select.h"

#define F_ROWS 64                                          /* rows of a workgroup: two wave rows x 32 */
#define F_TOK 64                                           /* tokens of a workgroup: two wave columns x 32 */
#define F_KC 128                                           /* K of a stage: four MFMA steps */
#define F_LD 132                                           /* LDS dwords between consecutive rows / tokens of a stage (4 mod 64) */
#define F_B_OFF (F_ROWS * F_LD)                            /* dword offset of the activations in a stage */
#define F_STAGE ((F_ROWS + F_TOK) * F_LD)                  /* dwords of a stage: 16 896 = 67 584 B */
#define F_LDS_BYTES (2 * F_STAGE * 4)                      /* 135 168 B */

struct bamd_mma_flt_args {
    const uint8_t * w;               // wave-stream records (bamd_formats.h)
    const float * blob;              // [T][K] f32 activations in the mat-vec's lane order (act_batch_flt_kernel)
    float * out; const float * res;  // [T][ldo]
    int K, T, nrows, nrows_pad, ldo;
};

template <int WT, int EPI>
__global__ void __launch_bounds__(256) matmul_mfma_flt_kernel(bamd_mma_flt_args a) {
    constexpr bool W32 = WT == BAMD_F32;
    constexpr int NA = W32 ? 8 : 4;                        // 16-byte weight pieces of a thread and stage
    constexpr int CHB = W32 ? 4096 : 2048;                 // bytes of a stage in a row-group's stream
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = lane & 15, kk = lane >> 4;
    const int wm = wave & 1, wn = wave >> 1;
    const int nch = a.K / F_KC;
    const int row0 = blockIdx.x * F_ROWS, t0 = blockIdx.y * F_TOK;
    const int nrg = a.nrows_pad >> 3;
    const size_t rgb = (size_t) (a.K >> 8) * (W32 ? BAMD_RECB_F32 : BAMD_RECB_F16);
    // staging plan.  Weights: piece p = it * 256 + tid of the stage's 8 row-groups (rows behind the matrix: the last row-group again, never stored)
    const uint8_t * wsrc[NA]; uint32_t wdst[NA];
#pragma unroll
    for (int it = 0; it < NA; ++it) {
        const int rgl = W32 ? it : 2 * it + (tid >> 7), q = W32 ? wave : wave & 1;           // row-group of the workgroup, request of the stage
        const int rg = (row0 >> 3) + rgl < nrg ? (row0 >> 3) + rgl : nrg - 1;
        wsrc[it] = a.w + (size_t) rg * rgb + q * 1024 + lane * 16;
        wdst[it] = (uint32_t) ((rgl * 8 + (lane >> 3)) * F_LD + (W32 ? q : 2 * q) * 32 + (lane & 7) * 4);
    }
    // activations: token it * 8 + tid / 32, piece tid & 31 of its 512 bytes (tokens behind T: the last token again, never stored)
    const float * xsrc[8]; uint32_t xdst[8];
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int tok = it * 8 + (tid >> 5), tg = t0 + tok < a.T ? t0 + tok : a.T - 1;
        xsrc[it] = a.blob + (size_t) tg * a.K + (tid & 31) * 4;
        xdst[it] = (uint32_t) (F_B_OFF + tok * F_LD + (tid & 31) * 4);
    }
    uint4 stw[NA]; bamd_f4 stx[8];
    // (macros, not lambdas: behind a lambda's reference the eight staged pieces of the F32 instance stayed in scratch memory)
#define F_STAGE_LOAD(c_) do { \
        _Pragma("unroll") for (int it = 0; it < NA; ++it) stw[it] = *(const uint4 *) (wsrc[it] + (size_t) (c_) * CHB); \
        _Pragma("unroll") for (int it = 0; it < 8; ++it) stx[it] = *(const bamd_f4 *) (xsrc[it] + (size_t) (c_) * F_KC); } while (0)
    // F16: eight halves = steps s = 2 q (kk 0..3) and 2 q + 1 (kk 0..3), widened exactly
#define F_STAGE_STORE(buf_) do { \
        float * d = smem + (buf_) * F_STAGE; \
        _Pragma("unroll") for (int it = 0; it < NA; ++it) { \
            const uint4 v = stw[it]; \
            if constexpr (W32) *(uint4 *) (d + wdst[it]) = v; \
            else { \
                *(bamd_f4 *) (d + wdst[it])      = (bamd_f4) { h2f(v.x & 0xffffu), h2f(v.x >> 16), h2f(v.y & 0xffffu), h2f(v.y >> 16) }; \
                *(bamd_f4 *) (d + wdst[it] + 32) = (bamd_f4) { h2f(v.z & 0xffffu), h2f(v.z >> 16), h2f(v.w & 0xffffu), h2f(v.w >> 16) }; \
            } \
        } \
        _Pragma("unroll") for (int it = 0; it < 8; ++it) *(bamd_f4 *) (d + xdst[it]) = stx[it]; } while (0)
    bamd_f4 acc[2][2][8];                                  // [row tile][token tile][j]
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[mt][nt][j] = (bamd_f4) { 0.f, 0.f, 0.f, 0.f };
    const uint32_t ra = (uint32_t) ((wm * 32 + m) * F_LD + kk), rb = (uint32_t) (F_B_OFF + (wn * 32 + m) * F_LD + kk);
    F_STAGE_LOAD(0);
    F_STAGE_STORE(0);
    __syncthreads();
    for (int c = 0; c < nch; ++c) {
        const float * st = smem + (c & 1) * F_STAGE;
        F_STAGE_LOAD(c + 1 < nch ? c + 1 : c);              // (the last chunk is staged once more into the buffer nobody reads again)
        __builtin_amdgcn_sched_barrier(0);                 // the requests in front of the MFMAs they travel under (left alone, the compiler sinks them to their stores)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            float av[2][8], bv[2][8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                av[0][j] = st[ra + s * 32 + j * 4]; av[1][j] = st[ra + 16 * F_LD + s * 32 + j * 4];
                bv[0][j] = st[rb + s * 32 + j * 4]; bv[1][j] = st[rb + 16 * F_LD + s * 32 + j * 4];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                acc[0][0][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[0][j], bv[0][j], acc[0][0][j], 0, 0, 0);
                acc[0][1][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[0][j], bv[1][j], acc[0][1][j], 0, 0, 0);
                acc[1][0][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[1][j], bv[0][j], acc[1][0][j], 0, 0, 0);
                acc[1][1][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[1][j], bv[1][j], acc[1][1][j], 0, 0, 0);
            }
        }
        F_STAGE_STORE((c + 1) & 1);                        // the buffer read in chunk c - 1: every wave is past that chunk's barrier
        __syncthreads();
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const bamd_f4 * c = acc[mt][nt];
            const bamd_f4 val = ((c[0] + c[4]) + (c[2] + c[6])) + ((c[1] + c[5]) + (c[3] + c[7]));      // hsum8_tinyblas' tree, element-wise
            const int t = t0 + wn * 32 + nt * 16 + m;
            if (t >= a.T) continue;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int row = row0 + wm * 32 + mt * 16 + 4 * kk + v;
                if (row >= a.nrows) continue;
                const size_t o = (size_t) t * a.ldo + row;
                a.out[o] = EPI == BAMD_EPI_ADD ? val[v] + a.res[o] : EPI == BAMD_EPI_SILU_MUL ? v_silu(a.res[o]) * val[v] : val[v];
            }
        }
    }
}

#undef F_STAGE_LOAD
#undef F_STAGE_STORE

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------
// (the callers ask the family's switch at each launch: bamd_prefill_mfma_type_notable, bamd_prefill_family.h)
template <int WT, int EPI> static int launch_flt(const bamd_mma_flt_args & a, dim3 grid, hipStream_t s) {
    // (once per device and instance: the attribute belongs to the current device, and the stages of a layer-split model launch on several)
    static bool set[64] = { false };
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { (void) hipGetLastError(); return 1; }
    if (!set[dev]) {
        if (hipFuncSetAttribute((const void *) matmul_mfma_flt_kernel<WT, EPI>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) F_LDS_BYTES) != hipSuccess) { (void) hipGetLastError(); return 1; }
        set[dev] = true;
    }
    hipLaunchKernelGGL((matmul_mfma_flt_kernel<WT, EPI>), grid, dim3(256), F_LDS_BYTES, s, a);
    return 0;
}
// one F32 or F16 matrix; the epilogues of bamd_launch_matmul_mfma2.  blob: the f32 activation rows of bamd_launch_act_batch_flt.  1 = type / shape not supported
int bamd_launch_matmul_mfma_flt(const void * w_stream, int type, int nrows, int nrows_pad, int K, const void * blob, int T, float * out, const float * res, int epi, int ldo,
                                hipStream_t s) {
    if ((type != BAMD_F32 && type != BAMD_F16) || T < 1 || nrows < 1 || nrows > nrows_pad || nrows_pad < 8 || (nrows_pad & 7) || K <= 0 || (K & 255) || K > bamd_flt_max_k(type)) return 1;
    if (epi != BAMD_EPI_STORE && epi != BAMD_EPI_ADD && epi != BAMD_EPI_SILU_MUL) return 1;
    if ((epi != BAMD_EPI_STORE) != (res != nullptr)) return 1;
    bamd_mma_flt_args a; a.w = (const uint8_t *) w_stream; a.blob = (const float *) blob; a.out = out; a.res = res;
    a.K = K; a.T = T; a.nrows = nrows; a.nrows_pad = nrows_pad; a.ldo = ldo;
    const dim3 grid((nrows_pad + F_ROWS - 1) / F_ROWS, (T + F_TOK - 1) / F_TOK);
    int rc = 1;
    with_const(consts<BAMD_EPI_ADD, BAMD_EPI_SILU_MUL, BAMD_EPI_STORE>(), epi, [&](auto E) -> bool {
        constexpr int EPI = decltype(E)::value;
        rc = type == BAMD_F32 ? launch_flt<BAMD_F32, EPI>(a, grid, s) : launch_flt<BAMD_F16, EPI>(a, grid, s);
        return true; });
    if (!rc) bamd_prefill_mfma_count(type);
    return rc;
}
