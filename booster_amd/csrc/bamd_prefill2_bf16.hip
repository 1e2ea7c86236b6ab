// bamd_prefill2_bf16.hip — the exact matrix-core prompt mat-mul for BF16 weights x bf16 activations, behind the switch BAMD_PREFILL_BF16=1 /
// bamd_set_prefill_bf16 (default off; the families and their switches: bamd_prefill_family.h).
//
// Arithmetic: the contract of bamd_flt_device.h — ggml_vec_dot_bf16's AVX2 branch.  One output = 32 chain lanes c = 8a + j, chain c:
// acc_c = add(mul(w[32i + c], x[32i + c]), acc_c) for i = 0 .. K/32 - 1 (two roundings), then (c1 + c3) + (c2 + c4) over a and hsum8_tinyblas' tree over j.
// A bf16 x bf16 product has at most 16 significant bits: it is EXACT in f32 unless its last bit falls below 2^-149 or it overflows, and where the product is
// exact add(mul(w, x), c) and fma(w, x, c) are the same single rounding.  There the sequential chain of v_mfma_f32_16x16x4_f32,
// D = fma(a3, b3, fma(a2, b2, fma(a1, b1, fma(a0, b0, C)))) (tools/mfma_f32_probe.hip; bamd_prefill2_flt.hip), is the reference's chain bit for bit.  So a
// 16 x 16 output tile is 32 accumulator tiles, one per chain lane c, and MFMA step s of tile c takes k = 32 (4 s + kk) + c for kk = 0..3: the links
// i = 4 s .. 4 s + 3 of chain c, in order, chained through C.  No split over K; the 32 tiles are combined element-wise in the tree above after the last step.
//
// The guard.  A bf16 pattern h with exponent field E = (h >> 7) & 0xff is an integer of fewer than 8 bits times 2^(e - 7), e = max(E, 1) - 127 (subnormals
// too), so a product is an integer of at most 16 bits times 2^(e_w + e_x - 14): exact iff that unit is >= 2^-149 and the magnitude stays under 2^128.
// Sufficient for a set of weights and a set of activations: emin_w + emin_x >= -135 over the nonzero values, emax_w + emax_x <= 126, no E == 255 on either
// side; a side without a nonzero value is safe.  A range is one word (bamd_bf16_range.h): the matrix's is computed once where its stream is packed
// (bamd_bf16_weight_range), a token's is written by the bf16 activation pass from the bits it stores (act_batch_flt_kernel).  The decision is made on the
// device, once per workgroup, before the K loop, from the matrix's word and the words of the workgroup's tokens — the host never waits for it.  A workgroup
// that is not safe runs the same loop over the same staged LDS data with bf_step on the vector ALUs: a lane's D registers are 4 outputs x 32 chains, so
// accumulators and epilogue are shared.  That path is slow, rare and exact; such a workgroup adds 1 to a device counter (bamd_prefill_bf16_fallback_tiles:
// tests and tools tell the two paths apart by it).
//
// Layout.  Lane maps of the instruction: A lane = (row m = lane & 15, kk = lane >> 4), B lane = (kk, token n = lane & 15), D register v of a lane = row 4 kk + v
// of token n.  Both operands are staged in LDS widened to f32 in the order [row or token][c][kk], 132 dwords per row and 128 of K: one stage is ONE MFMA step
// of all 32 chains.  That is the order the data lies in already: wave-stream lane (h, c) of request q of a record (bamd_formats.h) holds the eight links
// i = 0..7 of chain c of row 2 q + h as one 16-byte piece, and the bf16 activation rows of act_batch_flt_kernel are [record][c][i] as well — a piece is
// widened with shifts into the four kk of step 2 r (stage 0) and of step 2 r + 1 (stage 1) of record r.  No side table, no second activation pass.  An MFMA
// lane reads its operand of chain c as one dword at row * 132 + c * 4 + kk: the 64 lanes of a read fall on the 64 banks (4 m + kk).
// A workgroup is four waves = 32 rows x 32 tokens, a wave owns ONE tile of 16 rows x 16 tokens = 32 accumulator tiles, 128 registers (two token tiles per wave,
// 256 accumulator registers, left the compiler no in-place accumulators: it rotated them through copies and spilled).  Bytes moved per FLOP are those of the
// F32 kernel: half the tile, operands half as wide.  Per record the next one travels global -> registers while the MFMAs of this one run; its first half is
// stored into stage 0 between the two steps (behind the barrier that ends step 2 r), its second half into stage 1 behind the barrier that ends step 2 r + 1.  Consecutive MFMAs
// always write different accumulators: an accumulator is revisited after 31 others (the dependent latency is 40 cycles against a 32-cycle issue).
#include "bamd_flt_device.h"
#include "bamd_kernels.h"
#include "bamd_mfma_common.h"
#include "bamd_mv_select.h"
#include "bamd_bf16_range.h"

#define B_ROWS 32                                          /* rows of a workgroup: two wave rows x 16 */
#define B_TOK 32                                           /* tokens of a workgroup: two wave columns x 16 */
#define B_LD 132                                           /* LDS dwords between consecutive rows / tokens of a stage (4 mod 64) */
#define B_B_OFF (B_ROWS * B_LD)                            /* dword offset of the activations in a stage */
#define B_STAGE ((B_ROWS + B_TOK) * B_LD)                  /* dwords of a stage: 8 448 = 33 792 B */
#define B_LDS_BYTES (2 * B_STAGE * 4)                      /* 67 584 B */

struct bamd_mma_bf16_args {
    const uint8_t * w;               // wave-stream records (bamd_formats.h)
    const uint8_t * blob;            // [T][K] bf16 activations in the mat-vec's lane order (act_batch_flt_kernel)
    const uint32_t * xrange;         // [T] range word of every token's activations (bamd_bf16_range.h)
    unsigned int * fallback;         // counter of the workgroups that took the VALU step
    float * out; const float * res;  // [T][ldo]
    uint32_t wrange;                 // range word of the matrix
    int K, T, nrows, nrows_pad, ldo;
};

// the K loop and the epilogue of a workgroup, MM: on the matrix cores / on the vector ALUs.  Two instances of ONE body, so that each keeps its accumulators in
// one register class: with the choice inside the loop the compiler moved them between accumulation and vector registers at every step and spilled
template <int EPI, bool MM>
__device__ __forceinline__ void mma_bf16_body(const bamd_mma_bf16_args & a, float * smem) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = lane & 15, kk = lane >> 4;
    const int wm = wave & 1, wn = wave >> 1;
    const int nrec = a.K >> 8;
    const int row0 = blockIdx.x * B_ROWS, t0 = blockIdx.y * B_TOK;
    const int nrg = a.nrows_pad >> 3;
    const size_t rgb = (size_t) nrec * BAMD_RECB_BF16;
    // staging plan.  Weights: piece it * 256 + tid of a record of the workgroup's 4 row-groups (rows behind the matrix: the last row-group again, never stored):
    // row-group it, request q = wave, rows 2 q + (lane >> 5), chain lane & 31
    const uint8_t * wsrc[4]; uint32_t wdst[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int rg = (row0 >> 3) + it < nrg ? (row0 >> 3) + it : nrg - 1;
        wsrc[it] = a.w + (size_t) rg * rgb + wave * 1024 + lane * 16;
        wdst[it] = (uint32_t) ((it * 8 + 2 * wave + (lane >> 5)) * B_LD + (lane & 31) * 4);
    }
    // activations: token it * 8 + tid / 32, chain tid & 31 of its 512 bytes of a record (tokens behind T: the last token again, never stored)
    const uint8_t * xsrc[4]; uint32_t xdst[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int tok = it * 8 + (tid >> 5), tg = t0 + tok < a.T ? t0 + tok : a.T - 1;
        xsrc[it] = a.blob + (size_t) tg * a.K * 2 + (tid & 31) * 16;
        xdst[it] = (uint32_t) (B_B_OFF + tok * B_LD + (tid & 31) * 4);
    }
    uint4 stw[4], stx[4];
    // (macros, not lambdas: see bamd_prefill2_flt.hip)
#define B_STAGE_LOAD(r_) do { \
        _Pragma("unroll") for (int it = 0; it < 4; ++it) stw[it] = *(const uint4 *) (wsrc[it] + (size_t) (r_) * BAMD_RECB_BF16); \
        _Pragma("unroll") for (int it = 0; it < 4; ++it) stx[it] = *(const uint4 *) (xsrc[it] + (size_t) (r_) * 512); } while (0)
    // half 0: the links i = 0..3 (words x, y) of every piece into stage 0; half 1: i = 4..7 (words z, w) into stage 1.  Widened exactly
#define B_WIDE(lo_, hi_) ((bamd_f4) { bf2f_lo(lo_), bf2f_hi(lo_), bf2f_lo(hi_), bf2f_hi(hi_) })
#define B_STAGE_STORE(half_) do { \
        float * d = smem + (half_) * B_STAGE; \
        _Pragma("unroll") for (int it = 0; it < 4; ++it) *(bamd_f4 *) (d + wdst[it]) = (half_) ? B_WIDE(stw[it].z, stw[it].w) : B_WIDE(stw[it].x, stw[it].y); \
        _Pragma("unroll") for (int it = 0; it < 4; ++it) *(bamd_f4 *) (d + xdst[it]) = (half_) ? B_WIDE(stx[it].z, stx[it].w) : B_WIDE(stx[it].x, stx[it].y); } while (0)
    bamd_f4 acc[32];                                       // [chain c]
#pragma unroll
    for (int c = 0; c < 32; ++c) acc[c] = (bamd_f4) { 0.f, 0.f, 0.f, 0.f };
    const uint32_t ra = (uint32_t) ((wm * 16 + m) * B_LD + kk), rb = (uint32_t) (B_B_OFF + (wn * 16 + m) * B_LD + kk);
    // the VALU step reads whole links: the four rows 4 kk + v of the lane's D registers, and its token
    const uint32_t fa = (uint32_t) ((wm * 16 + 4 * kk) * B_LD), fb = (uint32_t) (B_B_OFF + (wn * 16 + m) * B_LD);
    // one step of all 32 chains from a stage: four links of each chain, in order
#define B_STEP(st_) do { \
        if constexpr (MM) { \
            _Pragma("unroll") for (int c = 0; c < 32; ++c) \
                acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32((st_)[ra + c * 4], (st_)[rb + c * 4], acc[c], 0, 0, 0); \
        } else { \
            _Pragma("unroll") for (int c = 0; c < 32; ++c) { \
                const bamd_f4 xv = *(const bamd_f4 *) ((st_) + fb + c * 4); \
                _Pragma("unroll") for (int v = 0; v < 4; ++v) { \
                    const bamd_f4 wv = *(const bamd_f4 *) ((st_) + fa + v * B_LD + c * 4); \
                    _Pragma("unroll") for (int l = 0; l < 4; ++l) acc[c][v] = bf_step(acc[c][v], wv[l], xv[l]); \
                } \
                __builtin_amdgcn_sched_barrier(0);         /* (one chain's operands at a time: hoisted, the 160 reads of a step do not fit the registers) */ \
            } \
        } } while (0)
    B_STAGE_LOAD(0);
    B_STAGE_STORE(0);
    B_STAGE_STORE(1);
    __syncthreads();
    for (int r = 0; r < nrec; ++r) {
        B_STAGE_LOAD(r + 1 < nrec ? r + 1 : r);            // (the last record is staged once more into the stages nobody reads again)
        __builtin_amdgcn_sched_barrier(0);                 // the requests in front of the MFMAs they travel under
        B_STEP(smem);
        __syncthreads();                                   // every wave is past stage 0 of record r
        B_STAGE_STORE(0);
        B_STEP(smem + B_STAGE);
        __syncthreads();                                   // every wave is past stage 1 of record r, and stage 0 of record r + 1 is written
        B_STAGE_STORE(1);                                  // (read behind the first barrier of the next round)
    }
    {
        const bamd_f4 * c = acc;
        bamd_f4 l[8];                                      // (c1 + c3) + (c2 + c4) over the four accumulators a of lane j: chain c = 8 a + j
#pragma unroll
        for (int j = 0; j < 8; ++j) l[j] = (c[j] + c[16 + j]) + (c[8 + j] + c[24 + j]);
        const bamd_f4 val = ((l[0] + l[4]) + (l[2] + l[6])) + ((l[1] + l[5]) + (l[3] + l[7]));      // hsum8_tinyblas' tree, element-wise
        const int t = t0 + wn * 16 + m;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int row = row0 + wm * 16 + 4 * kk + v;
            if (row >= a.nrows || t >= a.T) continue;
            const size_t o = (size_t) t * a.ldo + row;
            a.out[o] = EPI == BAMD_EPI_ADD ? val[v] + a.res[o] : EPI == BAMD_EPI_SILU_MUL ? v_silu(a.res[o]) * val[v] : val[v];
        }
    }
}

#undef B_STAGE_LOAD
#undef B_STAGE_STORE
#undef B_WIDE
#undef B_STEP

template <int EPI>
__global__ void __launch_bounds__(256) matmul_mfma_bf16_kernel(bamd_mma_bf16_args a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ uint32_t s_rng[2];
    const int tid = threadIdx.x, t0 = blockIdx.y * B_TOK;
    // the guard: the union of the range words of the workgroup's tokens (a token past T repeats the last one) against the matrix's
    if (tid == 0) { s_rng[0] = BAMD_BF16_RANGE_NONE & 0xffffu; s_rng[1] = 0u; }
    __syncthreads();
    if (tid < B_TOK) {
        const uint32_t r = a.xrange[t0 + tid < a.T ? t0 + tid : a.T - 1];
        atomicMin(&s_rng[0], r & 0xffffu); atomicMax(&s_rng[1], r >> 16);
    }
    __syncthreads();
    if (bamd_bf16_ranges_safe(a.wrange, s_rng[0] | s_rng[1] << 16)) mma_bf16_body<EPI, true>(a, smem);      // (workgroup-uniform)
    else {
        if (tid == 0) atomicAdd(a.fallback, 1u);
        mma_bf16_body<EPI, false>(a, smem);
    }
}

// ---- the range word of a matrix --------------------------------------------------------------------------------------------------------------------
// over the bf16 patterns of a wave-stream copy (the zero records of padded rows hold no nonzero value); out[0] = lowest, out[1] = highest exponent
__global__ void __launch_bounds__(256) bf16_weight_range_kernel(const uint4 * __restrict__ w, size_t n16, uint32_t * out) {
    uint32_t lo = BAMD_BF16_RANGE_NONE & 0xffffu, hi = 0u;
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t) gridDim.x * blockDim.x) {
        const uint4 v = w[i];
        bamd_bf16_range_add2(lo, hi, v.x); bamd_bf16_range_add2(lo, hi, v.y); bamd_bf16_range_add2(lo, hi, v.z); bamd_bf16_range_add2(lo, hi, v.w);
    }
    for (int o = 32; o; o >>= 1) { const uint32_t l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o); lo = l2 < lo ? l2 : lo; hi = h2 > hi ? h2 : hi; }
    if ((threadIdx.x & 63) == 0) { atomicMin(out, lo); atomicMax(out + 1, hi); }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------
// per device: the fallback counter and the two words the range kernel reduces into (12 bytes, allocated at the first use on that device, kept for the process)
static unsigned int * g_dev_words[64] = { nullptr };
static unsigned int * dev_words() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { (void) hipGetLastError(); return nullptr; }
    if (!g_dev_words[dev]) {
        unsigned int * p = nullptr;
        if (hipMalloc((void **) &p, 16) != hipSuccess || hipMemset(p, 0, 16) != hipSuccess) { (void) hipGetLastError(); return nullptr; }
        g_dev_words[dev] = p;
    }
    return g_dev_words[dev];
}
int bamd_bf16_weight_range(const void * w_stream, size_t bytes, uint32_t * word, hipStream_t s) {
    unsigned int * p = dev_words();
    if (!p || (bytes & 15)) return 1;
    const uint32_t init[2] = { BAMD_BF16_RANGE_NONE & 0xffffu, 0u }; uint32_t got[2];
    if (hipMemcpyAsync(p + 1, init, 8, hipMemcpyHostToDevice, s) != hipSuccess) { (void) hipGetLastError(); return 1; }
    const size_t n16 = bytes >> 4;
    if (n16) hipLaunchKernelGGL(bf16_weight_range_kernel, dim3((unsigned) std::min<size_t>((n16 + 255) / 256, 2048)), dim3(256), 0, s, (const uint4 *) w_stream, n16, p + 1);
    if (hipMemcpyAsync(got, p + 1, 8, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) { (void) hipGetLastError(); return 1; }
    *word = got[0] | got[1] << 16;
    return 0;
}
unsigned long long bamd_bf16_fallback_tiles_all(void) {
    int cur = 0; unsigned long long n = 0;
    if (hipGetDevice(&cur) != hipSuccess) { (void) hipGetLastError(); return 0; }
    for (int d = 0; d < 64; ++d) if (g_dev_words[d]) {
        unsigned int v = 0;
        if (hipSetDevice(d) == hipSuccess && hipDeviceSynchronize() == hipSuccess && hipMemcpy(&v, g_dev_words[d], 4, hipMemcpyDeviceToHost) == hipSuccess) n += v;
        else (void) hipGetLastError();
    }
    (void) hipSetDevice(cur);
    return n;
}

// (the callers ask the family's switch at each launch: bamd_prefill_mfma_type_notable, bamd_prefill_family.h)
template <int EPI> static int launch_bf16(const bamd_mma_bf16_args & a, dim3 grid, hipStream_t s) {
    // (once per device and instance: the attribute belongs to the current device, and the stages of a layer-split model launch on several)
    static bool set[64] = { false };
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { (void) hipGetLastError(); return 1; }
    if (!set[dev]) {
        if (hipFuncSetAttribute((const void *) matmul_mfma_bf16_kernel<EPI>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) B_LDS_BYTES) != hipSuccess) { (void) hipGetLastError(); return 1; }
        set[dev] = true;
    }
    hipLaunchKernelGGL((matmul_mfma_bf16_kernel<EPI>), grid, dim3(256), B_LDS_BYTES, s, a);
    return 0;
}
// one BF16 matrix; the epilogues of bamd_launch_matmul_mfma2.  blob: the bf16 activation rows of bamd_launch_act_batch_flt, xrange: the range words it wrote
// beside them, wrange: the matrix's (bamd_bf16_weight_range).  1 = shape not supported
int bamd_launch_matmul_mfma_bf16(const void * w_stream, uint32_t wrange, int nrows, int nrows_pad, int K, const void * blob, const uint32_t * xrange, int T, float * out,
                                 const float * res, int epi, int ldo, hipStream_t s) {
    if (T < 1 || nrows < 1 || nrows > nrows_pad || nrows_pad < 8 || (nrows_pad & 7) || K <= 0 || (K & 255) || K > bamd_flt_max_k(BAMD_BF16) || !xrange) return 1;
    if (epi != BAMD_EPI_STORE && epi != BAMD_EPI_ADD && epi != BAMD_EPI_SILU_MUL) return 1;
    if ((epi != BAMD_EPI_STORE) != (res != nullptr)) return 1;
    bamd_mma_bf16_args a; a.w = (const uint8_t *) w_stream; a.blob = (const uint8_t *) blob; a.xrange = xrange; a.out = out; a.res = res; a.wrange = wrange;
    a.K = K; a.T = T; a.nrows = nrows; a.nrows_pad = nrows_pad; a.ldo = ldo;
    if (!(a.fallback = dev_words())) return 1;
    const dim3 grid((nrows_pad + B_ROWS - 1) / B_ROWS, (T + B_TOK - 1) / B_TOK);
    int rc = 1;
    with_const(consts<BAMD_EPI_ADD, BAMD_EPI_SILU_MUL, BAMD_EPI_STORE>(), epi, [&](auto E) -> bool {
        rc = launch_bf16<decltype(E)::value>(a, grid, s);
        return true; });
    if (!rc) bamd_prefill_mfma_count(BAMD_BF16);
    return rc;
}
