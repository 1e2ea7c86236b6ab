// bamd_matvec_flt.hip — single-token mat-vec for unquantised weights (F32 / F16 with f32 activations, BF16 with bf16 activations) and the family's load-time
// repack.  Numerics, activation order and the chains: bamd_flt_device.h; records: bamd_formats.h.
//
// One wave carries TWO row-groups at once (a unit): the chain of a lane is strictly serial over K, so the two chains (BF16: eight, four rows per lane and
// row-group) interleave, and the activations a lane reads from LDS serve both.  A gate/up launch pairs the gate and the up row-group of the same rows.  No
// split-K: a partial sum per wave would change the bits.  Each row-group is a sequential stream of 4 KiB chunks, the next chunk requested before the current
// one is consumed.  The kernels keep the inter-kernel rules of bamd_device.h (ik_* for activations, residual, outputs; nt buffer loads for weights only) and
// launch through BAMD_LAUNCH, so a float model's greedy loop replays from the own AQL queue.
#include "bamd_flt_device.h"
#include "bamd_aql.h"
#include "bamd_kernels.h"
#include "bamd_mv_select.h"

// ---- repack: GGUF row-major -> records.  One thread per 16-byte request of a record ----
__global__ void __launch_bounds__(256) repack_flt_kernel(const uint8_t * __restrict__ raw, uint8_t * __restrict__ dst, int type, int nrows, int K) {
    const int recb = bamd_record_bytes_repack(type), per = recb >> 4, nb = K >> 8;
    const int64_t idx = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = (int64_t) ((nrows + 7) >> 3) * nb * per;
    if (idx >= total) return;
    const int u = (int) (idx % per), q = u >> 6, lane = u & 63;
    const int64_t rec = idx / per;
    const int ib = (int) (rec % nb), rg = (int) (rec / nb);
    uint32_t out[4] = { 0u, 0u, 0u, 0u };
    if (type == BAMD_F32) {
        const int row = rg * 8 + (lane >> 3), j = lane & 7;
        if (row < nrows) for (int t = 0; t < 4; ++t) out[t] = ((const uint32_t *) raw)[(int64_t) row * K + ib * 256 + 8 * (4 * q + t) + j];
    } else if (type == BAMD_F16) {
        const int row = rg * 8 + (lane >> 3), j = lane & 7;
        if (row < nrows) for (int t = 0; t < 8; ++t) out[t >> 1] |= (uint32_t) ((const unsigned short *) raw)[(int64_t) row * K + ib * 256 + 8 * (8 * q + t) + j] << (16 * (t & 1));
    } else {
        const int row = rg * 8 + 2 * q + (lane >> 5), c = lane & 31;
        if (row < nrows) for (int t = 0; t < 8; ++t) out[t >> 1] |= (uint32_t) ((const unsigned short *) raw)[(int64_t) row * K + ib * 256 + 32 * t + c] << (16 * (t & 1));
    }
    *(uint4 *) (dst + rec * recb + (int64_t) q * 1024 + lane * 16) = make_uint4(out[0], out[1], out[2], out[3]);
}
void bamd_launch_repack_flt(const void * raw, void * dst, int type, int nrows, int K, hipStream_t s) {
    const int64_t n = (int64_t) ((nrows + 7) >> 3) * (K >> 8) * (bamd_record_bytes(type) >> 4);
    BAMD_LAUNCH(repack_flt_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, s, (const uint8_t *) raw, (uint8_t *) dst, type, nrows, K);
}

// ---- one unit: row-group rgA of wA and row-group rgB of wB (hasB false: none, its requests go through the zero-record descriptor) ----
template <int WT, int EPI>
__device__ __forceinline__ void flt_unit(const uint8_t * __restrict__ wA, const uint8_t * __restrict__ wB, int rgA, int rgB, bool hasB, int K, const unsigned char * act,
                                         float * __restrict__ out, const float * __restrict__ res, int nvalid, unsigned long long & best) {
    constexpr bool BF = WT == BAMD_BF16, PAIR = EPI == BAMD_EPI_SILU_MUL;
    constexpr int KC = BAMD_FLT_CHUNK_K(WT);
    const int lane = threadIdx.x & 63;
    const int nch = K / KC, rgb = nch * BAMD_FLT_CHB;
    const bamd_rsrc rsA = weight_rsrc(wA), rsN = null_rsrc(wA), rsB = hasB ? weight_rsrc(wB) : rsN;
    const int offA = rgA * rgb, offB = hasB ? rgB * rgb : 0;
    // residual first: by the epilogue it is the oldest outstanding load
    float resA[4] = { 0.f, 0.f, 0.f, 0.f }, resB[4] = { 0.f, 0.f, 0.f, 0.f };
    if (EPI == BAMD_EPI_ADD) {
        if (BF) {
            if ((lane & 31) == 0) for (int q = 0; q < 4; ++q) {
                const int ra = rgA * 8 + 2 * q + (lane >> 5), rb = rgB * 8 + 2 * q + (lane >> 5);
                if (ra < nvalid) resA[q] = ik_ld(res + ra);
                if (hasB && rb < nvalid) resB[q] = ik_ld(res + rb);
            }
        } else if ((lane & 7) == 0) {
            const int ra = rgA * 8 + (lane >> 3), rb = rgB * 8 + (lane >> 3);
            if (ra < nvalid) resA[0] = ik_ld(res + ra);
            if (hasB && rb < nvalid) resB[0] = ik_ld(res + rb);
        }
    }
    FltChunk A0, B0, A1, B1;
    flt_load(A0, rsA, offA, lane); flt_load(B0, rsB, offB, lane);
    float accA[4] = { 0.f, 0.f, 0.f, 0.f }, accB[4] = { 0.f, 0.f, 0.f, 0.f };
    const float4 * X4 = (const float4 *) act + (lane & 7);
    const uint4 * XB = (const uint4 *) act + (lane & 31);
    auto consume = [&](const FltChunk & CA, const FltChunk & CB, int c) {
        if constexpr (BF) {
            const uint4 xa = XB[c * 32];
            flt_chain_bf(accA, CA, xa); flt_chain_bf(accB, CB, xa);
        } else {
            accA[0] = flt_chain<WT, 8>(accA[0], CA, X4 + c * (KC / 4));
            accB[0] = flt_chain<WT, 8>(accB[0], CB, X4 + c * (KC / 4));
        }
    };
    for (int c = 0; c < nch; c += 2) {
        const bool m1 = c + 1 < nch, m2 = c + 2 < nch;               // wave-uniform
        flt_load(A1, m1 ? rsA : rsN, m1 ? offA + (c + 1) * BAMD_FLT_CHB : 0, lane);
        flt_load(B1, m1 ? rsB : rsN, m1 ? offB + (c + 1) * BAMD_FLT_CHB : 0, lane);
        consume(A0, B0, c);
        flt_load(A0, m2 ? rsA : rsN, m2 ? offA + (c + 2) * BAMD_FLT_CHB : 0, lane);
        flt_load(B0, m2 ? rsB : rsN, m2 ? offB + (c + 2) * BAMD_FLT_CHB : 0, lane);
        if (m1) consume(A1, B1, c + 1);
    }
    auto emit = [&](int row, float v, float r) {
        if (row < nvalid) {
            const float o = EPI == BAMD_EPI_ADD ? v + r : v;
            ik_st(out + row, o);
            if (EPI == BAMD_EPI_ARGMAX) { const unsigned long long k = argmax_key(o, row); best = k > best ? k : best; }
        }
    };
    if constexpr (BF) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float va = flt_finish_bf(accA[q]), vb = flt_finish_bf(accB[q]);
            if ((lane & 31) == 0) {
                const int ra = rgA * 8 + 2 * q + (lane >> 5);
                if (PAIR) { if (ra < nvalid) ik_st(out + ra, v_silu(va) * vb); }
                else { emit(ra, va, resA[q]); if (hasB) emit(rgB * 8 + 2 * q + (lane >> 5), vb, resB[q]); }
            }
        }
    } else {
        const float va = hsum8_tinyblas(accA[0]), vb = hsum8_tinyblas(accB[0]);
        if ((lane & 7) == 0) {
            const int ra = rgA * 8 + (lane >> 3);
            if (PAIR) { if (ra < nvalid) ik_st(out + ra, v_silu(va) * vb); }
            else { emit(ra, va, resA[0]); if (hasB) emit(rgB * 8 + (lane >> 3), vb, resB[0]); }
        }
    }
}

// BF: the activation form of the launch (every segment BF16) — otherwise every segment is F32 or F16, a run-time property of the segment
template <bool BF, int PRO, int EPI>
__global__ void __launch_bounds__(512) matvec_flt_kernel(bamd_mv_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool PAIR = EPI == BAMD_EPI_SILU_MUL;
    const int K = a.K;
    double * red = (double *) (smem + (size_t) K * (BF ? 2 : 4));
    flt_act<PRO == BAMD_PRO_NORM, BF>(a.x, a.normw, a.eps, K, smem, red);
    const int wave = wave_id(), nwaves = (int) (blockDim.x >> 6);
    const int slot = blockIdx.x + gridDim.x * wave, stride = gridDim.x * nwaves;      // consecutive units land on different CUs
    unsigned long long best = 0ull;
    int off = 0;
    const int nseg = PAIR ? 1 : a.nseg;
    for (int s = 0; s < nseg; ++s) {
        const int nrg = a.seg[s].nrows >> 3, nu = PAIR ? nrg : (nrg + 1) >> 1;
        const int k0 = off <= slot ? 0 : (off - slot + stride - 1) / stride;
        const int t = a.seg[s].type;
        const uint8_t * wA = (const uint8_t *) a.seg[s].w;
        const uint8_t * wB = PAIR ? (const uint8_t *) a.seg[1].w : wA;
        const int nv = a.seg[s].nvalid > 0 ? a.seg[s].nvalid : a.seg[s].nrows;
        for (int g = slot + k0 * stride; g < off + nu; g += stride) {
            const int u = g - off;
            const int rgA = PAIR ? u : 2 * u, rgB = PAIR ? u : 2 * u + 1;
            const bool hasB = PAIR || rgB < nrg;
            if constexpr (BF) flt_unit<BAMD_BF16, EPI>(wA, wB, rgA, rgB, hasB, K, smem, a.seg[s].out, a.res, nv, best);
            else if (t == BAMD_F32) flt_unit<BAMD_F32, EPI>(wA, wB, rgA, rgB, hasB, K, smem, a.seg[s].out, a.res, nv, best);
            else flt_unit<BAMD_F16, EPI>(wA, wB, rgA, rgB, hasB, K, smem, a.seg[s].out, a.res, nv, best);
        }
        off += nu;
    }
    if (EPI == BAMD_EPI_ARGMAX) {
        for (int o = 32; o; o >>= 1) { const unsigned long long ob = __shfl_xor(best, o); best = ob > best ? ob : best; }
        unsigned long long * wb = (unsigned long long *) (red + 16);
        if ((threadIdx.x & 63) == 0) wb[wave] = best;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long b = 0ull;
            for (int w = 0; w < nwaves; ++w) b = wb[w] > b ? wb[w] : b;
            if (b) atomicMax(a.best_key, b);
        }
    }
}

// test entry: the bf16 activation form out of the prologue, in the order of the vector (bamd_op_act_bf16)
__global__ void __launch_bounds__(512) act_bf16_test_kernel(const float * x, const float * nw, float eps, int K, int norm, unsigned short * out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double * red = (double *) (smem + (size_t) K * 2);
    if (norm) flt_act<true, true>(x, nw, eps, K, smem, red); else flt_act<false, true>(x, nw, eps, K, smem, red);
    const unsigned short * a = (const unsigned short *) smem;
    for (int k = threadIdx.x; k < K; k += blockDim.x) out[k] = a[((k >> 8) << 8) + ((k >> 5) & 7) + ((k & 31) << 3)];
}
// a workgroup that keeps more than 64 KiB of activations in LDS (K beyond 16 128 as f32): HIP launches need the kernel's limit raised (an own-queue packet carries
// its LDS size itself)
template <typename KERNEL> static void flt_allow_lds(KERNEL kernel, size_t lds) {
    if (lds > 64 * 1024 && !bamd_aql_rec) (void) hipFuncSetAttribute((const void *) kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) BAMD_LDS_CU_BYTES);
}
void bamd_launch_act_bf16_test(const float * x, const float * nw, float eps, int K, int norm, void * out, hipStream_t s) {
    flt_allow_lds(act_bf16_test_kernel, flt_lds_bytes(true, K));
    BAMD_LAUNCH(act_bf16_test_kernel, dim3(1), dim3(512), flt_lds_bytes(true, K), s, x, nw, eps, K, norm, (unsigned short *) out);
}

// every segment of the activation form of segment 0 (F32 | F16 together, or BF16), K within what the LDS holds; 1 = otherwise (nothing launched)
int bamd_launch_matvec_flt(const bamd_mv_args & a, int pro, int epi, int n_cu, hipStream_t s) {
    if (a.nseg < 1 || !bamd_is_flt(a.seg[0].type)) return 1;
    const int form = bamd_act_form_of(a.seg[0].type);
    for (int i = 0; i < a.nseg; ++i) if (!bamd_is_flt(a.seg[i].type) || bamd_act_form_of(a.seg[i].type) != form) return 1;
    if (epi == BAMD_EPI_SILU_MUL && (a.nseg != 2 || a.seg[1].type != a.seg[0].type)) return 1;
    if (a.K <= 0 || a.K % 256 || a.K > bamd_flt_max_k(a.seg[0].type)) return 1;
    const bool bf = form == BAMD_ACT_BF16;
    static_assert(flt_lds_bytes(false, 40704) <= (size_t) BAMD_LDS_CU_BYTES && flt_lds_bytes(true, 65536) <= (size_t) BAMD_LDS_CU_BYTES, "the activation vector fits the LDS of a CU (bamd_flt_max_k)");
    int nu = 0;
    if (epi == BAMD_EPI_SILU_MUL) nu = a.seg[0].nrows >> 3;
    else for (int i = 0; i < a.nseg; ++i) nu += ((a.seg[i].nrows >> 3) + 1) >> 1;
    const int cus = n_cu > 0 ? n_cu : 256;
    const int grid = nu < 1 ? 1 : nu < cus ? nu : cus;
    const size_t lds = flt_lds_bytes(bf, a.K);
    typedef consts<BAMD_PRO_NORM, BAMD_PRO_PLAIN> pros;
    typedef consts<BAMD_EPI_STORE, BAMD_EPI_ADD, BAMD_EPI_SILU_MUL, BAMD_EPI_ARGMAX> epis;
    if (bf) return with_const(pros(), pro, [&](auto P) -> bool { return with_const(epis(), epi, [&](auto E) -> bool {
        flt_allow_lds(matvec_flt_kernel<true, decltype(P)::value, decltype(E)::value>, lds);
        BAMD_LAUNCH((matvec_flt_kernel<true, decltype(P)::value, decltype(E)::value>), dim3(grid), dim3(512), lds, s, a); return true; }); }) ? 0 : 1;
    return with_const(pros(), pro, [&](auto P) -> bool { return with_const(epis(), epi, [&](auto E) -> bool {
        flt_allow_lds(matvec_flt_kernel<false, decltype(P)::value, decltype(E)::value>, lds);
        BAMD_LAUNCH((matvec_flt_kernel<false, decltype(P)::value, decltype(E)::value>), dim3(grid), dim3(512), lds, s, a); return true; }); }) ? 0 : 1;
}
