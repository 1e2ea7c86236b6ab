// bamd_prefill.hip — batched prefill: per-token Q8_K quantisation into global blobs (and their f16 copy for the matrix-core kernels of bamd_prefill2.hip), the
// integer-dot batched mat-mul of the K-quants (row policy and type list here, the body in bamd_prefill_valu.h), batched embedding.  Helpers: bamd_device.h.
#include "bamd_prefill_valu.h"
#include "bamd_prefill_family.h"

// ===========================================================================================================
// Batched prefill (T > 1 tokens per call; reference: llama_decode with a micro-batch, ggml_compute_forward_mul_mat with
// ne11 = T, ggml.c:12277-12492).  Per (row, token) the arithmetic is EXACTLY the single-token chain of the mat-vec kernels (bamd_device.h) — the reference
// quantises each activation row to Q8_K and runs the same vec_dot per (row, column).  Two implementations, bit-identical:
//   the matrix-core kernels of bamd_prefill2.hip (default, for a model whose side tables were built): the integer sums of a super-block on
//     the matrix cores, exactly, and the f32 chains on the VALU;
//   matmul_batch_kernel (BAMD_PREFILL_MFMA=0; the second implementation the first is tested against): block_terms / chain_step /
//     finish_row of the decode path, the weights of a record unpacked once for BAMD_TT tokens whose Q8_K activations sit in LDS.
// ===========================================================================================================

// one workgroup per token: RMSNorm (optional) + Q8_K of row t of x[T][K] -> blob[t]
// f16 copy of a token's Q8_K row for the MFMA path.  Per super-block BAMD_B16_REC = 608 B: 8 (e) x 4 (g) groups of 8 halves — group
// (e, g) = the int8 of sub-blocks 2g and 2g+1, chunk e, as exact f16: one 16-byte B operand of v_mfma_f32_16x16x32_f16 per lane —
// then, per pair l of sub-blocks, the four halves {S_h(2l), S_h(2l+1), S_l(2l), S_l(2l+1)} of the block sums split as S = 2 S_h + S_l
// (the B operand of the Q4_K min-term MFMA), then the four i16 pairs (S_2l, S_2l+1) (Q5_K), then the block scale d_y (f32, byte 560), then the sixteen sums of sixteen activations as f16 (bytes 576..607: Q2_K's min term); after the nb super-blocks, yd[nb] f32 again.
template <bool NORM>
__global__ void __launch_bounds__(512) quantize_batch_kernel(const float * __restrict__ x, const float * __restrict__ nw, float eps, int K,
                                                             uint8_t * __restrict__ blob, uint8_t * __restrict__ blob16) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nb = K >> 8, t = blockIdx.x;
    uint32_t * q8 = (uint32_t *) smem; int * S = (int *) (q8 + nb * 64); float * yd = (float *) (S + nb * 8);
    double * red = (double *) (smem + BAMD_ACT_RED_OFF(nb));
    const float * xt = x + (size_t) t * K;
    ActPro<NORM> ap; ap.issue(xt, nw, K, wave_id()); ap.finish(xt, nw, eps, K, q8, S, yd, red);
    const size_t bb = BAMD_BLOB_BYTES(nb);
    if (blob) {
        const uint4 * src = (const uint4 *) smem; uint4 * dst = (uint4 *) (blob + (size_t) t * bb);
        for (int i = threadIdx.x; i < (int) (bb / 16); i += blockDim.x) dst[i] = src[i];
    }
    if (blob16) {
        uint8_t * o = blob16 + (size_t) t * BAMD_BLOB16_BYTES(nb);
        for (int i = threadIdx.x; i < nb * 64; i += blockDim.x) {          // q8[ci*64 + e*8 + c] = sub-block c, chunk e, 4 int8
            const int ci = i >> 6, e = (i >> 3) & 7, c = i & 7;
            *(uint2 *) (o + (size_t) ci * BAMD_B16_REC + (size_t) (e * 4 + (c >> 1)) * 16 + (c & 1) * 8) = i8x4_halves(q8[i]);
        }
        for (int i = threadIdx.x; i < nb * 4; i += blockDim.x) {
            const int ci = i >> 2, l = i & 3;
            const int sa = S[ci * 8 + 2 * l], sb = S[ci * 8 + 2 * l + 1];          // block sums of sub-blocks 2l, 2l+1: |S| <= 32 * 127
            // operands of the min-term MFMA (Q4_K): S = 2 S_h + S_l with S_h = S >> 1 (|.| <= 2048) and S_l = S & 1 both exact in f16
            uint2 mf;
            mf.x = (uint32_t) f2h((float) (sa >> 1)) | ((uint32_t) f2h((float) (sb >> 1)) << 16);
            mf.y = (uint32_t) f2h((float) (sa & 1)) | ((uint32_t) f2h((float) (sb & 1)) << 16);
            *(uint2 *) (o + (size_t) ci * BAMD_B16_REC + 512 + l * 8) = mf;
            // (S_2l, S_2l+1) as i16 pairs (Q5_K: v_dot2_i32_i16)
            *(uint32_t *) (o + (size_t) ci * BAMD_B16_REC + 544 + l * 4) = ((uint32_t) sa & 0xffffu) | ((uint32_t) sb << 16);
        }
        for (int i = threadIdx.x; i < nb * 16; i += blockDim.x) {          // Q2_K min term: the sums of sixteen activations (Q8_K's bsums), sixteen f16 at bytes 576..607
            const int ci = i >> 4, sb = i & 15, c = sb >> 1, h = sb & 1;     // sub-block sb = bytes 0..15 (h = 0: chunks e = 0..3) or 16..31 (h = 1) of the 32 of chunk row c
            int b = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) b = __builtin_amdgcn_sdot4((int) q8[ci * 64 + (4 * h + e) * 8 + c], 0x01010101, b, false);
            *(unsigned short *) (o + (size_t) ci * BAMD_B16_REC + 576 + sb * 2) = f2h((float) b);                  // |b| <= 2048: exact
        }
        float * oyd = (float *) (o + (size_t) nb * BAMD_B16_REC);
        for (int i = threadIdx.x; i < nb; i += blockDim.x) { oyd[i] = yd[i]; *(float *) (o + (size_t) i * BAMD_B16_REC + 560) = yd[i]; }   // d_y also inside the record (bamd_prefill2.hip: no separate copy)
    }
}


// the row policy of a K-quant: block_terms / chain_step / finish_row of the decode path over the Q8_K image q8 | S | yd; one accumulator (a pair of chains), no
// temporaries.  Behind a wave's last chunk the row's last record is read again (step 0)
// (the unnamed RowAcc & and kq_none & parameters: valu_segment hands every policy three accumulators and three temporaries, because the storage of the 32-weight
// block types has to be declared there for their kernels to stay what they are, bamd_prefill_valu.h; a K-quant needs one accumulator, the rest is never touched)
struct kq_none {};
template <int TYPE, typename REC> struct KqRow {
    typedef REC Rec;
    typedef RowAcc Acc;
    typedef kq_none Work;
    static constexpr int RECB = BAMD_RECB_OF(TYPE);
    static constexpr bool NULL_TAIL = false;
    static __device__ __forceinline__ void zero(RowAcc & A, RowAcc &, RowAcc &) { A.acc = 0.f; A.accm = 0.f; }
    static __device__ __forceinline__ void step(const REC & R, int ci, int lane, const unsigned char * au, int nb, RowAcc & A, RowAcc &, RowAcc &, kq_none &, kq_none &, kq_none &) {
        const uint32_t * q8 = (const uint32_t *) au; const int * S = (const int *) (q8 + nb * 64); const float * yd = (const float *) (S + nb * 8);
        const Terms T = block_terms(R, ci, lane, q8, S, yd);
        chain_step<TYPE>(A, T.d, T.fs, T.dmin, T.pm);
    }
    static __device__ __forceinline__ float finish(const RowAcc & A, const RowAcc &, const RowAcc &) { return finish_row<TYPE>(A); }
};
// the type list (BAMD_VALU_MM_KERNEL_BODY): ring depth 4 when it divides the row (it does for every K % 1024 == 0), else 1
#define BAMD_KQ_TYPES_D(SEG, D) { \
    if (t == BAMD_Q4_K)      SEG(D, KqRow<BAMD_Q4_K, RecQ4K>); \
    else if (t == BAMD_Q5_K) SEG(D, KqRow<BAMD_Q5_K, RecQ5K>); \
    else if (t == BAMD_Q6_K) SEG(D, KqRow<BAMD_Q6_K, RecQ6K>); \
    else if (t == BAMD_Q3_K) SEG(D, KqRow<BAMD_Q3_K, RecQ3K>); \
    else if (t == BAMD_Q2_K) SEG(D, KqRow<BAMD_Q2_K, RecQ2K>); \
    else if (t == BAMD_IQ4_XS) SEG(D, KqRow<BAMD_IQ4_XS, RecIQ4XS>); \
    else __builtin_trap();                       /* the launcher checks the types: never a silent read as another format */ \
}
#define BAMD_KQ_TYPES(SEG) if ((nb & 3) == 0) BAMD_KQ_TYPES_D(SEG, 4) else BAMD_KQ_TYPES_D(SEG, 1)

// (Rounds 2-5 kept a first generation of matrix-core mat-mul kernels here — every wave expanding its own 16 rows — and a second one in bamd_prefill2.hip;
// round 6 measured what bounds them (profiles/r06_prefill_ceiling.txt) and kept ONE: bamd_prefill2.hip.  This file keeps the integer-dot kernel — the second
// implementation the matrix-core kernels are tested against, and what a matrix without a side table runs on — and the plumbing.)

template <int EPI, int TT>
__global__ void __launch_bounds__(512) matmul_batch_kernel(bamd_mm_args a) {
    BAMD_VALU_MM_KERNEL_BODY(BAMD_KQ_TYPES)
}

// batched prefill: one workgroup per token of the micro-batch
__global__ void __launch_bounds__(256) embed_batch_kernel(const int32_t * __restrict__ tokens, const uint8_t * embd, int embd_type, int E, int V, float * x) {
    int tok = tokens[blockIdx.x];
    if (tok < 0 || tok >= V) tok = 0;
    embed_row(embd, embd_type, E, tok, x + (size_t) blockIdx.x * E);
}


// ===========================================================================================================
// launchers
// ===========================================================================================================
// ---- batched prefill launchers ------------------------------------------------------------------------------------------
size_t bamd_blob_bytes(int K) { return BAMD_BLOB_BYTES(K >> 8); }
size_t bamd_blob16_bytes(int K) { return BAMD_BLOB16_BYTES(K >> 8); }
void bamd_launch_quantize_batch(const float * x, const float * nw, float eps, int K, int T, void * blob, void * blob16, hipStream_t s, int form, uint32_t * bf16_range) {
    if (form == BAMD_ACT_F32 || form == BAMD_ACT_BF16) { bamd_launch_act_batch_flt(form, x, nw, eps, K, T, blob, s, bf16_range); return; }
    if (form == BAMD_ACT_Q8_1 || form == BAMD_ACT_Q8_0) { bamd_launch_quantize_batch_b32(form, x, nw, eps, K, T, blob, s, bamd_prefill_reads_act16(form) ? blob16 : nullptr); return; }
    if (nw) hipLaunchKernelGGL((quantize_batch_kernel<true>),  dim3(T), dim3(512), act_lds_bytes(K), s, x, nw, eps, K, (uint8_t *) blob, (uint8_t *) blob16);
    else    hipLaunchKernelGGL((quantize_batch_kernel<false>), dim3(T), dim3(512), act_lds_bytes(K), s, x, nw, eps, K, (uint8_t *) blob, (uint8_t *) blob16);
}
int bamd_launch_matmul_batch(const bamd_mm_args & a, int epi, int n_cu, hipStream_t s) {
    if (a.nseg > 0 && bamd_is_flt(a.seg[0].type)) return bamd_launch_matmul_batch_flt(a, epi, n_cu, s);      // f32 / bf16 activations (bamd_prefill_flt.hip)
    if (a.nseg > 0 && bamd_is_b32(a.seg[0].type)) return bamd_launch_matmul_batch_b32(a, epi, n_cu, s);      // Q8_0 / Q8_1 activations: kernels of their own; a launch that mixes the forms has none
    valu_mm_geom g;
    if (!valu_mm_geometry(a, epi, n_cu, g)) return 1;                 // K > 35840
    for (int i = 0; i < a.nseg; ++i) if (!bamd_is_kquant(a.seg[i].type)) return 1;
#define BAMD_MB(EPI_) do { if (g.tt == BAMD_TT) hipLaunchKernelGGL((matmul_batch_kernel<EPI_, BAMD_TT>), g.grid, dim3(512), g.lds, s, a); else hipLaunchKernelGGL((matmul_batch_kernel<EPI_, 4>), g.grid, dim3(512), g.lds, s, a); } while (0)
    switch (epi) {
        case BAMD_EPI_STORE:    BAMD_MB(BAMD_EPI_STORE); break;
        case BAMD_EPI_ADD:      BAMD_MB(BAMD_EPI_ADD); break;
        case BAMD_EPI_SILU_MUL: BAMD_MB(BAMD_EPI_SILU_MUL); break;
        default: return 1;
    }
#undef BAMD_MB
    return 0;
}
void bamd_launch_embed_batch(const int32_t * tokens, int T, const void * embd, int embd_type, int E, int V, float * x, hipStream_t s) {
    hipLaunchKernelGGL(embed_batch_kernel, dim3(T), dim3(256), 0, s, tokens, (const uint8_t *) embd, embd_type, E, V, x);
}
