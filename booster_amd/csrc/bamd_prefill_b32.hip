// bamd_prefill_b32.hip — batched prompt evaluation for the 32-weight block formats: per-token Q8_0 (Q8_0 / Q4_0 / Q5_0 weights) or Q8_1 (Q4_1 / Q5_1) quantisation
// into the activation blobs and the integer-dot batched mat-mul (the counterpart of quantize_batch_kernel / matmul_batch_kernel, bamd_prefill.hip).  Per (row,
// token) the arithmetic is exactly the single-token chain (with a minimum: pair of chains) of bamd_b32_device.h: the reference quantises every activation row and
// runs the same block chain per output element, for one token and for many (without a minimum tinyBLAS_Q0_AVX::gemm, sgemm.cpp:711-759: the tile shape never
// changes the order of an element's chain; with a minimum ggml_vec_dot_q4_1_q8_1 / _q5_1_q8_1 per output element: llamafile_sgemm has no case for these types,
// sgemm.cpp:961-1007; IQ4_NL, Q8_0 activations: ggml_vec_dot_iq4_nl_q8_0 per output element, two chains per (row, token), in a kernel of its own whose type list
// also holds Q8_0 / Q4_0 / Q5_0: the two earlier kernels stay what they were).  The matrix-core kernel of these types and of IQ4_NL is bamd_prefill2_b32.hip, behind three switches (bamd_prefill_family.h); this file also writes its
// f16 activation records.
#include "bamd_prefill_b32.h"

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
            *(uint2 *) (o + (size_t) ci * BAMD_B16_REC + c * 64 + (e & 3) * 16 + (e >> 2) * 8) = i8x4_halves(q8[i]);
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
// the family of segment 0 decides; without a minimum, a launch with an IQ4_NL segment anywhere takes the kernel that has the type (bamd_prefill_b32_nl.hip)
int bamd_launch_matmul_batch_b32(const bamd_mm_args & a, int epi, int n_cu, hipStream_t s) {
    for (int i = 0; i < a.nseg; ++i) if (a.seg[i].type == BAMD_IQ4_NL && !bamd_is_q1(a.seg[0].type)) return bamd_launch_matmul_batch_b32_nl(a, epi, n_cu, s);
    return launch_matmul_batch_b32<>(a, epi, n_cu, s);
}
