// bamd_prefill_flt.hip — batched prompt path of the unquantised weight family (F32 / F16 / BF16): the activation pass for T rows and a VALU mat-mul for 1..512
// tokens.  Every output runs the chain of the mat-vec (bamd_flt_device.h) — the reference's per-element chain does not depend on the number of tokens either
// (tinyBLAS tiles differ only in which outputs share a loop) — so a batched prompt gives the bits of token by token.  F32 / F16: bamd_prefill2_flt.hip runs the same chains on the matrix cores (BAMD_PREFILL_FLT); BF16: bamd_prefill2_bf16.hip (BAMD_PREFILL_BF16).
#include "bamd_flt_device.h"
#include "bamd_kernels.h"

// one workgroup per token: RMSNorm * norm_w (or the plain row) -> the row in the form's order (f32: 4 K bytes, bf16: 2 K bytes per token)
// xrange (bf16 form only; null: none): [T] the range word of every token's stored patterns (bamd_bf16_range.h), for the guard of bamd_prefill2_bf16.hip
template <bool NORM, bool BF>
__global__ void __launch_bounds__(512) act_batch_flt_kernel(const float * __restrict__ x, const float * __restrict__ nw, float eps, int K, unsigned char * __restrict__ blob, uint32_t * __restrict__ xrange) {
    __shared__ double red[16];
    const size_t t = blockIdx.x;
    if constexpr (BF) {
        __shared__ uint32_t rng[2];
        if (xrange) {                                     // (kernel-uniform)
            if (threadIdx.x == 0) { rng[0] = BAMD_BF16_RANGE_NONE & 0xffffu; rng[1] = 0u; }
            __syncthreads();
        }
        flt_act<NORM, true>(x + t * (size_t) K, nw, eps, K, blob + t * (size_t) K * 2, red, xrange ? rng : nullptr);
        if (xrange && threadIdx.x == 0) xrange[t] = rng[0] | rng[1] << 16;
    } else flt_act<NORM, false>(x + t * (size_t) K, nw, eps, K, blob + t * (size_t) K * 4, red);
}
void bamd_launch_act_batch_flt(int form, const float * x, const float * nw, float eps, int K, int T, void * blob, hipStream_t s, uint32_t * xrange) {
    unsigned char * b = (unsigned char *) blob;
    if (form == BAMD_ACT_BF16) {
        if (nw) hipLaunchKernelGGL((act_batch_flt_kernel<true, true>),  dim3(T), dim3(512), 0, s, x, nw, eps, K, b, xrange);
        else    hipLaunchKernelGGL((act_batch_flt_kernel<false, true>), dim3(T), dim3(512), 0, s, x, nw, eps, K, b, xrange);
    } else {
        if (nw) hipLaunchKernelGGL((act_batch_flt_kernel<true, false>),  dim3(T), dim3(512), 0, s, x, nw, eps, K, b, (uint32_t *) nullptr);
        else    hipLaunchKernelGGL((act_batch_flt_kernel<false, false>), dim3(T), dim3(512), 0, s, x, nw, eps, K, b, (uint32_t *) nullptr);
    }
}

#define BAMD_FLT_TT 4                    /* tokens per wave tile: each weight chunk is requested once per tile */
// the values of row-group rg of w for the tokens t0 .. t0 + TT - 1 (a token past T repeats the last one; its values are not stored).
// F32 / F16: val[t][0] in lanes (r, 0); BF16: val[t][q] = row 2q + h in lanes (h, 0, 0)
template <int WT>
__device__ __forceinline__ void flt_mm_rows(const uint8_t * __restrict__ w, int rg, int K, const unsigned char * __restrict__ blob, int t0, int T, float (&val)[BAMD_FLT_TT][4]) {
    constexpr bool BF = WT == BAMD_BF16;
    constexpr int KC = BAMD_FLT_CHUNK_K(WT);
    const int lane = threadIdx.x & 63;
    const int nch = K / KC, rgb = nch * BAMD_FLT_CHB;
    const bamd_rsrc rs = weight_rsrc(w), rsN = null_rsrc(w);
    const int off = rg * rgb;
    const unsigned char * xt[BAMD_FLT_TT];
#pragma unroll
    for (int t = 0; t < BAMD_FLT_TT; ++t) {
        const int tt = t0 + t < T ? t0 + t : T - 1;
        xt[t] = blob + (size_t) tt * K * (BF ? 2 : 4) + (BF ? (lane & 31) * 16 : (lane & 7) * 16);
    }
    float acc[BAMD_FLT_TT][4];
#pragma unroll
    for (int t = 0; t < BAMD_FLT_TT; ++t) { acc[t][0] = 0.f; acc[t][1] = 0.f; acc[t][2] = 0.f; acc[t][3] = 0.f; }
    FltChunk C0, C1;
    flt_load(C0, rs, off, lane);
    auto consume = [&](const FltChunk & C, int c) {
#pragma unroll
        for (int t = 0; t < BAMD_FLT_TT; ++t) {
            if constexpr (BF) flt_chain_bf(acc[t], C, *((const uint4 *) xt[t] + c * 32));
            else acc[t][0] = flt_chain<WT, 8>(acc[t][0], C, (const float4 *) xt[t] + c * (KC / 4));
        }
    };
    for (int c = 0; c < nch; c += 2) {
        const bool m1 = c + 1 < nch, m2 = c + 2 < nch;
        flt_load(C1, m1 ? rs : rsN, m1 ? off + (c + 1) * BAMD_FLT_CHB : 0, lane);
        consume(C0, c);
        flt_load(C0, m2 ? rs : rsN, m2 ? off + (c + 2) * BAMD_FLT_CHB : 0, lane);
        if (m1) consume(C1, c + 1);
    }
#pragma unroll
    for (int t = 0; t < BAMD_FLT_TT; ++t) {
        if constexpr (BF) { for (int q = 0; q < 4; ++q) val[t][q] = flt_finish_bf(acc[t][q]); }
        else val[t][0] = hsum8_tinyblas(acc[t][0]);
    }
}

// grid (units, token tiles); a wave per row-group (gate/up: the gate and the up row-group of the same rows, one after the other)
template <bool BF, int EPI>
__global__ void __launch_bounds__(256) matmul_batch_flt_kernel(bamd_mm_args a) {
    constexpr bool PAIR = EPI == BAMD_EPI_SILU_MUL;
    const int lane = threadIdx.x & 63, wave = wave_id(), nwaves = (int) (blockDim.x >> 6);
    const int t0 = blockIdx.y * BAMD_FLT_TT;
    int u = blockIdx.x * nwaves + wave;
    const int nseg = PAIR ? 1 : a.nseg;
    for (int s = 0; s < nseg; ++s) {
        const int nrg = a.seg[s].nrows >> 3;
        if (u >= nrg) { u -= nrg; continue; }
        const int ty = a.seg[s].type;
        const int nv = a.seg[s].nvalid > 0 ? a.seg[s].nvalid : a.seg[s].nrows;
        float v[BAMD_FLT_TT][4], g[BAMD_FLT_TT][4];
        auto rows = [&](const void * w, float (&o)[BAMD_FLT_TT][4]) {
            if constexpr (BF) flt_mm_rows<BAMD_BF16>((const uint8_t *) w, u, a.K, a.blob, t0, a.T, o);
            else if (ty == BAMD_F32) flt_mm_rows<BAMD_F32>((const uint8_t *) w, u, a.K, a.blob, t0, a.T, o);
            else flt_mm_rows<BAMD_F16>((const uint8_t *) w, u, a.K, a.blob, t0, a.T, o);
        };
        rows(a.seg[s].w, v);
        if (PAIR) { for (int t = 0; t < BAMD_FLT_TT; ++t) for (int q = 0; q < 4; ++q) g[t][q] = v[t][q]; rows(a.seg[1].w, v); }
        const bool owner = BF ? (lane & 31) == 0 : (lane & 7) == 0;
        if (owner) {
#pragma unroll
            for (int t = 0; t < BAMD_FLT_TT; ++t) {
                if (t0 + t >= a.T) break;
#pragma unroll
                for (int q = 0; q < (BF ? 4 : 1); ++q) {
                    const int row = BF ? u * 8 + 2 * q + (lane >> 5) : u * 8 + (lane >> 3);
                    if (row >= nv) continue;
                    const size_t o = (size_t) (t0 + t) * a.ldo + row;
                    float r = v[t][q];
                    if (PAIR) r = v_silu(g[t][q]) * r;
                    else if (EPI == BAMD_EPI_ADD) r = r + a.res[o];
                    a.seg[s].out[o] = r;
                }
            }
        }
        return;
    }
}

// every segment of the activation form of segment 0, a.blob in that form (bamd_launch_act_batch_flt); 1 = otherwise
int bamd_launch_matmul_batch_flt(const bamd_mm_args & a, int epi, int n_cu, hipStream_t s) {
    (void) n_cu;
    if (a.nseg < 1 || !bamd_is_flt(a.seg[0].type) || a.T < 1) return 1;
    const int form = bamd_act_form_of(a.seg[0].type);
    for (int i = 0; i < a.nseg; ++i) if (!bamd_is_flt(a.seg[i].type) || bamd_act_form_of(a.seg[i].type) != form) return 1;
    if (epi == BAMD_EPI_SILU_MUL && (a.nseg != 2 || a.seg[1].type != a.seg[0].type)) return 1;
    if (epi != BAMD_EPI_STORE && epi != BAMD_EPI_ADD && epi != BAMD_EPI_SILU_MUL) return 1;
    if (a.K <= 0 || a.K % 256) return 1;
    int nrg = 0;
    if (epi == BAMD_EPI_SILU_MUL) nrg = a.seg[0].nrows >> 3; else for (int i = 0; i < a.nseg; ++i) nrg += a.seg[i].nrows >> 3;
    const dim3 grid((unsigned) ((nrg + 3) / 4), (unsigned) ((a.T + BAMD_FLT_TT - 1) / BAMD_FLT_TT));
    const bool bf = form == BAMD_ACT_BF16;
#define BAMD_FLT_MM(BF_, EPI_) hipLaunchKernelGGL((matmul_batch_flt_kernel<BF_, EPI_>), grid, dim3(256), 0, s, a)
    if (bf) { if (epi == BAMD_EPI_STORE) BAMD_FLT_MM(true, BAMD_EPI_STORE); else if (epi == BAMD_EPI_ADD) BAMD_FLT_MM(true, BAMD_EPI_ADD); else BAMD_FLT_MM(true, BAMD_EPI_SILU_MUL); }
    else    { if (epi == BAMD_EPI_STORE) BAMD_FLT_MM(false, BAMD_EPI_STORE); else if (epi == BAMD_EPI_ADD) BAMD_FLT_MM(false, BAMD_EPI_ADD); else BAMD_FLT_MM(false, BAMD_EPI_SILU_MUL); }
#undef BAMD_FLT_MM
    return 0;
}
