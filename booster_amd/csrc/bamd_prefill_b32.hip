// bamd_prefill_b32.hip — batched prompt evaluation for the 32-weight block formats: per-token Q8_0 (Q8_0 / Q4_0 / Q5_0 weights) or Q8_1 (Q4_1 / Q5_1) quantisation
// into the activation blobs and the integer-dot batched mat-mul (the counterpart of quantize_batch_kernel / matmul_batch_kernel, bamd_prefill.hip).  Per (row,
// token) the arithmetic is exactly the single-token chain (with a minimum: pair of chains) of bamd_b32_device.h: the reference quantises every activation row and
// runs the same block chain per output element, for one token and for many (without a minimum tinyBLAS_Q0_AVX::gemm, sgemm.cpp:711-759: the tile shape never
// changes the order of an element's chain; with a minimum ggml_vec_dot_q4_1_q8_1 / _q5_1_q8_1 per output element: llamafile_sgemm has no case for these types,
// sgemm.cpp:961-1007).  The matrix-core kernel of these types is bamd_prefill2_b32.hip, behind two switches (bamd_prefill_mfma_type); this file also writes its
// f16 activation records.
#include "bamd_b32_device.h"

// one workgroup per token: RMSNorm (optional) + Q8_0 / Q8_1 (MIN) of row t of x[T][K] -> blob[t], the LDS image of the mat-vec prologue (q8 | block scales as
// f32, or the blocks' {f16 d, f16 s} pairs), with the stride of the Q8_K blobs.
// blob16 (may be null): the same values for the matrix-core kernel, per 256 values one BAMD_B16_REC record of which 544 (MIN: 576) bytes are used — the 256 quants
// as exact f16 in the order its A operand reads them, element 4e + k of block c at half c * 32 + (e & 3) * 8 + (e >> 2) * 4 + k, then the eight block scales d_x as
// f32 at byte 512 and, MIN, the eight s_x as f32 at byte 544.  s_x is the f16 s of the image widened: finish_q0<true> rounded it twice (d to f16, the product to
// f16), and it is not computed again here
template <bool NORM, bool MIN>
__global__ void __launch_bounds__(512) quantize_batch_b32_kernel(const float * __restrict__ x, const float * __restrict__ nw, float eps, int K, uint8_t * __restrict__ blob,
                                                                 uint8_t * __restrict__ blob16) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nb = K >> 8, t = blockIdx.x;
    uint32_t * q8 = (uint32_t *) smem; float * ys = (float *) (q8 + nb * 64);
    double * red = (double *) (smem + BAMD_ACT_RED_OFF(nb));
    const float * xt = x + (size_t) t * K;
    for (int i = threadIdx.x; i < nb; i += blockDim.x) ys[nb * 8 + i] = 0.f;            // the yd slots of the image: unused by these types, written so that the blob is defined
    ActProQ0<NORM> ap; ap.issue(xt, nw, K, wave_id()); ap.template finish_q0<MIN>(xt, nw, eps, K, q8, ys, red);
    const size_t bb = BAMD_BLOB_BYTES(nb);
    const uint4 * src = (const uint4 *) smem; uint4 * dst = (uint4 *) (blob + (size_t) t * bb);
    for (int i = threadIdx.x; i < (int) (bb / 16); i += blockDim.x) dst[i] = src[i];
    if (blob16) {
        uint8_t * o = blob16 + (size_t) t * BAMD_BLOB16_BYTES(nb);
        for (int i = threadIdx.x; i < nb * 64; i += blockDim.x) {          // q8[ci*64 + e*8 + c] = block c, chunk e, 4 int8 (never -128)
            const int ci = i >> 6, e = (i >> 3) & 7, c = i & 7;
            const uint32_t w = q8[i];
            const unsigned short h0 = f2h((float) (int8_t) (w)), h1 = f2h((float) (int8_t) (w >> 8)), h2 = f2h((float) (int8_t) (w >> 16)), h3 = f2h((float) (int8_t) (w >> 24));
            uint2 v; v.x = (uint32_t) h0 | ((uint32_t) h1 << 16); v.y = (uint32_t) h2 | ((uint32_t) h3 << 16);
            *(uint2 *) (o + (size_t) ci * BAMD_B16_REC + c * 64 + (e & 3) * 16 + (e >> 2) * 8) = v;
        }
        if (MIN) {
            const uint32_t * yp = (const uint32_t *) ys;                   // {f16 d, f16 s} of block i
            for (int i = threadIdx.x; i < nb * 8; i += blockDim.x) {
                float * rec = (float *) (o + (size_t) (i >> 3) * BAMD_B16_REC + 512);
                rec[i & 7] = h2f(yp[i] & 0xffffu); rec[8 + (i & 7)] = h2f(yp[i] >> 16);
            }
        } else {
            for (int i = threadIdx.x; i < nb * 8; i += blockDim.x) *(float *) (o + (size_t) (i >> 3) * BAMD_B16_REC + 512 + (i & 7) * 4) = ys[i];
        }
    }
}

template <int TYPE, int D, int EPI, int TT>
__device__ __forceinline__ void batch_segment_b32(const uint8_t * __restrict__ wA, const uint8_t * __restrict__ wB, int nb, int first, int count, int stride,
                                                  float * __restrict__ out, const float * __restrict__ res, int ldo, int t0, int nt,
                                                  const unsigned char * acts, size_t bb, int nvalid) {
    constexpr int RECB = BAMD_RECB_OF(TYPE);
    constexpr bool MIN = b32_has_min(TYPE);
    constexpr bool PAIR = EPI == BAMD_EPI_SILU_MUL;
    constexpr int NPARTS = PAIR ? 2 : 1;
    const int lane = threadIdx.x & 63;
    const bamd_rsrc rsA = weight_rsrc(wA), rsB = PAIR ? weight_rsrc(wB) : rsA, rsN = null_rsrc(wA);
    const int rgb = nb * RECB, rg_step = stride * rgb;
    const int chunks = nb / D;
    RecB32<TYPE> ring[D];
#pragma unroll
    for (int s = 0; s < D; ++s) load_rec(ring[s], rsA, first * rgb + s * RECB, lane);
    for (int r = 0; r < count; ++r) {
        const int rg = first + r * stride;
        const int row = rg * 8 + (lane >> 3);
        const int rowoff = rg * rgb;
        float gate_val[TT];
#pragma unroll
        for (int part = 0; part < NPARTS; ++part) {
            const bool last = !(PAIR && part == 0) && r + 1 >= count;
            const bool after_b = PAIR && part == 0;
            const int after_off = (PAIR && part == 0) ? rowoff : rowoff + rg_step;
            float acc[TT], summs[TT];
#pragma unroll
            for (int u = 0; u < TT; ++u) { acc[u] = 0.f; summs[u] = 0.f; }
            for (int c = 0; c < chunks; ++c) {
                const bool inrow = c + 1 < chunks;
                const bool tail = !inrow && last;                // behind the wave's last chunk: the zero-record descriptor
                const bamd_rsrc nrs = tail ? rsN : (inrow ? part == 1 : after_b) ? rsB : rsA;
                const int nxt = tail ? 0 : inrow ? rowoff + (c + 1) * (D * RECB) : after_off;
#pragma unroll
                for (int s = 0; s < D; ++s) {
                    pin_rec(ring[s]);
#pragma unroll
                    for (int u = 0; u < TT; ++u) {               // tokens beyond nt read the last token's copy and are never stored
                        const unsigned char * au = acts + (size_t) u * bb;
                        const uint32_t * q8 = (const uint32_t *) au; const float * ys = (const float *) (q8 + nb * 64);
                        float sc[8], fd[8], ms[8];
                        b32_terms(ring[s], c * D + s, lane, q8, ys, sc, fd, ms);
                        b32_chain8(acc[u], sc, fd);
                        if (MIN) b32_summs8(summs[u], ms);
                    }
                    load_rec(ring[s], nrs, nxt + s * RECB, lane);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
#pragma unroll
            for (int u = 0; u < TT; ++u) {
                const float val = b32_finish_row<MIN>(acc[u], summs[u]);
                if (PAIR && part == 0) { gate_val[u] = val; continue; }
                if ((lane & 7) == 0 && row < nvalid && u < nt) {
                    const size_t o = (size_t) (t0 + u) * ldo + row;
                    float y = val;
                    if (PAIR) y = v_silu(gate_val[u]) * val;
                    if (EPI == BAMD_EPI_ADD) y = val + res[o];
                    out[o] = y;
                }
            }
        }
    }
}

// grid (token tiles, row slots) and the tile sizes of matmul_batch_kernel: the blob has its stride, so TT tokens take the same LDS.  MIN: the family of the launch
template <bool MIN, int EPI, int TT>
__global__ void __launch_bounds__(512) matmul_batch_b32_kernel(bamd_mm_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nb = a.K >> 8;
    const size_t bb = BAMD_BLOB_BYTES(nb);
    const int t0 = blockIdx.x * TT;
    const int nt = a.T - t0 < TT ? a.T - t0 : TT;
    {   // this tile's activations -> LDS (rows past T: repeat the last token; results discarded)
        const int n16 = (int) (bb / 16);
        for (int i = threadIdx.x; i < n16 * TT; i += blockDim.x) {
            const int u = i / n16, k = i - u * n16;
            const int tu = t0 + (u < nt ? u : nt - 1);
            ((uint4 *) smem)[(size_t) u * n16 + k] = ((const uint4 *) (a.blob + (size_t) tu * bb))[k];
        }
    }
    __syncthreads();
    const int wave = wave_id(), nwaves = blockDim.x >> 6;
    const int slot = blockIdx.y + gridDim.y * wave, stride = gridDim.y * nwaves;
    constexpr bool PAIR = EPI == BAMD_EPI_SILU_MUL;
    int off = 0;
    const int nseg = PAIR ? 1 : a.nseg;
    for (int s = 0; s < nseg; ++s) {
        const int nrg = a.seg[s].nrows >> 3;
        const int k0 = off <= slot ? 0 : (off - slot + stride - 1) / stride;
        const int g0 = slot + k0 * stride;
        const int count = g0 < off + nrg ? (off + nrg - 1 - g0) / stride + 1 : 0;
        if (count > 0) {
            const int t = a.seg[s].type;
            const uint8_t * wA = (const uint8_t *) a.seg[s].w;
            const uint8_t * wB = PAIR ? (const uint8_t *) a.seg[1].w : wA;
            const int nv = a.seg[s].nvalid > 0 ? a.seg[s].nvalid : a.seg[s].nrows;
            // ring depth 2 where the record count is even — but, with a minimum, not in the gate/up instance at 8 tokens, whose gate values leave no room for a
            // second record (with it the compiler spills: 8 bytes of scratch per lane)
#define BAMD_B32_SEG(TYPE_, D_) batch_segment_b32<TYPE_, D_, EPI, TT>(wA, wB, nb, g0 - off, count, stride, a.seg[s].out, a.res, a.ldo, t0, nt, smem, bb, nv)
#define BAMD_B32_TYPES(D_) do { \
                if constexpr (MIN) { \
                    if (t == BAMD_Q4_1)      BAMD_B32_SEG(BAMD_Q4_1, D_); \
                    else if (t == BAMD_Q5_1) BAMD_B32_SEG(BAMD_Q5_1, D_); \
                    else __builtin_trap();                   /* the launcher checks the types: never a silent read as another format */ \
                } else { \
                    if (t == BAMD_Q8_0)      BAMD_B32_SEG(BAMD_Q8_0, D_); \
                    else if (t == BAMD_Q4_0) BAMD_B32_SEG(BAMD_Q4_0, D_); \
                    else if (t == BAMD_Q5_0) BAMD_B32_SEG(BAMD_Q5_0, D_); \
                    else __builtin_trap(); \
                } } while (0)
            if ((nb & 1) == 0 && !(MIN && PAIR && TT == 8)) BAMD_B32_TYPES(2);
            else                                            BAMD_B32_TYPES(1);
#undef BAMD_B32_TYPES
#undef BAMD_B32_SEG
        }
        off += nrg;
    }
}

// ===========================================================================================================
// launchers
// ===========================================================================================================
// form: BAMD_ACT_Q8_0 or BAMD_ACT_Q8_1
void bamd_launch_quantize_batch_b32(int form, const float * x, const float * nw, float eps, int K, int T, void * blob, hipStream_t s, void * blob16) {
#define BAMD_QB32(NORM_, MIN_) hipLaunchKernelGGL((quantize_batch_b32_kernel<NORM_, MIN_>), dim3(T), dim3(512), act_lds_bytes(K), s, x, nw, eps, K, (uint8_t *) blob, (uint8_t *) blob16)
    if (form == BAMD_ACT_Q8_1) { if (nw) BAMD_QB32(true, true); else BAMD_QB32(false, true); }
    else                       { if (nw) BAMD_QB32(true, false); else BAMD_QB32(false, false); }
#undef BAMD_QB32
}
// every segment of the family of segment 0; a.blob in that family's form (bamd_launch_quantize_batch_b32).  1 = shape not supported
int bamd_launch_matmul_batch_b32(const bamd_mm_args & a, int epi, int n_cu, hipStream_t s) {
    const bool has_min = a.nseg > 0 && bamd_is_q1(a.seg[0].type);
    int nrg = 0;
    if (epi == BAMD_EPI_SILU_MUL) nrg = a.seg[0].nrows >> 3; else for (int i = 0; i < a.nseg; ++i) nrg += a.seg[i].nrows >> 3;
    const int tt = (size_t) BAMD_TT * BAMD_BLOB_BYTES(a.K >> 8) <= 160 * 1024 ? BAMD_TT : 4;
    const size_t lds = (size_t) tt * BAMD_BLOB_BYTES(a.K >> 8);
    if (lds > 160 * 1024) return 1;
    for (int i = 0; i < a.nseg; ++i) if (!(has_min ? bamd_is_q1(a.seg[i].type) : bamd_is_q0(a.seg[i].type))) return 1;
    const int tiles = (a.T + tt - 1) / tt;
    int gy = (4 * (n_cu > 0 ? n_cu : 256) + tiles - 1) / tiles;
    if (gy * 8 > nrg) gy = (nrg + 7) / 8;
    if (gy < 1) gy = 1;
    dim3 grid(tiles, gy);
#define BAMD_MB32_(MIN_, EPI_) do { if (tt == BAMD_TT) hipLaunchKernelGGL((matmul_batch_b32_kernel<MIN_, EPI_, BAMD_TT>), grid, dim3(512), lds, s, a); else hipLaunchKernelGGL((matmul_batch_b32_kernel<MIN_, EPI_, 4>), grid, dim3(512), lds, s, a); } while (0)
#define BAMD_MB32(EPI_) do { if (has_min) BAMD_MB32_(true, EPI_); else BAMD_MB32_(false, EPI_); } while (0)
    switch (epi) {
        case BAMD_EPI_STORE:    BAMD_MB32(BAMD_EPI_STORE); break;
        case BAMD_EPI_ADD:      BAMD_MB32(BAMD_EPI_ADD); break;
        case BAMD_EPI_SILU_MUL: BAMD_MB32(BAMD_EPI_SILU_MUL); break;
        default: return 1;
    }
#undef BAMD_MB32
#undef BAMD_MB32_
    return 0;
}
