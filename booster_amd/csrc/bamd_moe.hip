// bamd_moe.hip — the mixture-of-experts feed-forward of a Mixtral-style Llama layer for ONE token, three launches in place of the dense gate/up and ffn_down launches:
//   1. router         one workgroup: RMSNorm, the F32 router mat-vec, softmax, top-k, weight normalisation          -> sel[n_used] (i32), w[n_used] (f32)
//   2. routed gate/up grid (row-group tiles, slot): the K-quant stream of expert sel[slot], silu(gate) * up          -> h[slot][F]
//   3. routed down    a workgroup owns a tile of output row-groups for ALL slots, wave s = slot s; w-scaled, summed  -> out[E] = x + sum_s down_s * w_s
// The expert a workgroup streams is a value another launch computed on the device: its weight base is (matrix base + sel x bytes per expert).
// Everything handed from launch to launch (x, sel, w, h, out) is inter-kernel data (bamd_device.h): ik_* only.  Numerics contract: bamd_device.h.
//
// What is restated (cpp/ = the reference):
//   llm_build_moe_ffn                       src/llama.cpp:8087-8186 (norm_w = true, no scale: build_llama :8882-8899)
//   router logits                           llamafile_sgemm F32 x F32, tinyBLAS<8> (ggml/src/llamafile/sgemm.cpp:865-887): the chain of bamd_flt_device.h
//   ggml_compute_forward_soft_max_f32       ggml/src/ggml.c:13682-13778 (scale 1, no mask), ggml_vec_soft_max_f32 :2619-2670 (AVX2 groups of 8; n_expert % 8 == 0)
//   ggml_compute_forward_argsort_f32        ggml/src/ggml.c:15185-15199: an exchange sort, not stable — the loops themselves are restated (router_select)
//   ggml_sum_rows / ggml_div / ggml_mul     f64 sum rounded to f32, f32 division; every expert output times its weight, rounded, then added left to right
//   ggml_compute_forward_mul_mat_id         ggml/src/ggml.c:12494: one vec_dot of a whole row per output, each slot's activations quantised on their own
#include "bamd_moe_device.h"

// LDS of the down launch: one Q8_K blob (q8 | S | yd) per slot, then the weighted outputs [n_used][tile * 8]
constexpr size_t moe_down_slot_bytes(int F) { return BAMD_ACT_RED_OFF(F >> 8); }
constexpr size_t moe_down_lds(int F, int n_used, int tile) { return (size_t) n_used * moe_down_slot_bytes(F) + (size_t) n_used * tile * 8 * 4; }
#define BAMD_MOE_DOWN_TILE_MAX 8

// ===========================================================================================================
// 1. router
// ===========================================================================================================
// (the one-lane selection behind it, router_select: bamd_moe_device.h, shared with the batched router)
__global__ void __launch_bounds__(512) moe_router_kernel(bamd_moe_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int K = a.E, lane = threadIdx.x & 63, wave = wave_id();
    double * red = (double *) (smem + (size_t) K * 4);
    float * lg = (float *) (smem + (size_t) K * 4 + 16 * sizeof(double));
    float * pv = lg + BAMD_MOE_MAX_EXPERT; int * idx = (int *) (pv + BAMD_MOE_MAX_EXPERT);
    flt_act<true, false>(a.x, a.normw, a.eps, K, smem, red);               // cur = rms_norm(x) * ffn_norm, in the order the chain lanes read it; ends with a barrier
    if (wave * 8 < a.n_expert) {                                             // eight lanes per expert row: wave w = experts 8 w .. 8 w + 7 (one F32 row-group)
        const int nch = K / BAMD_FLT_CHUNK_K(BAMD_F32), off = wave * nch * BAMD_FLT_CHB;
        const bamd_rsrc rs = weight_rsrc(a.gate_inp), rsN = null_rsrc(a.gate_inp);
        const float4 * X4 = (const float4 *) smem + (lane & 7);
        FltChunk A0, A1;
        flt_load(A0, rs, off, lane);
        float acc = 0.f;
        for (int c = 0; c < nch; c += 2) {                                   // the next chunk requested before the current one is consumed (flt_unit)
            const bool m1 = c + 1 < nch, m2 = c + 2 < nch;
            flt_load(A1, m1 ? rs : rsN, m1 ? off + (c + 1) * BAMD_FLT_CHB : 0, lane);
            acc = flt_chain<BAMD_F32, 8>(acc, A0, X4 + c * (BAMD_FLT_CHUNK_K(BAMD_F32) / 4));
            flt_load(A0, m2 ? rs : rsN, m2 ? off + (c + 2) * BAMD_FLT_CHB : 0, lane);
            if (m1) acc = flt_chain<BAMD_F32, 8>(acc, A1, X4 + (c + 1) * (BAMD_FLT_CHUNK_K(BAMD_F32) / 4));
        }
        const float v = hsum8_tinyblas(acc);
        if ((lane & 7) == 0) lg[wave * 8 + (lane >> 3)] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) router_select(lg, pv, idx, a.n_expert, a.n_used, a.sel, a.w);
}

// ===========================================================================================================
// 2. routed gate/up: blockIdx.y = slot, blockIdx.x = a tile of the F / 8 row-group pairs, one wave per pair (mode A, bamd_matvec_core.h)
// ===========================================================================================================
template <int TYPE>
__global__ void __launch_bounds__(512) moe_gate_up_kernel(bamd_moe_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nb = a.E >> 8;
    ProArgs pa;
    pa.x = a.x; pa.nw = a.normw; pa.eps = a.eps; pa.K = a.E; pa.tl = nullptr;
    pa.q8 = (uint32_t *) smem; pa.S = (int *) (pa.q8 + nb * 64); pa.yd = (float *) (pa.S + nb * 8); pa.red = (double *) (smem + BAMD_ACT_RED_OFF(nb));
    // the activation requests go out first, the expert id right behind them: both round trips run together, and the weight ring — which needs the id — is
    // requested in front of the RMSNorm + Q8_K arithmetic as in every mode-A launch
    ActPro<true> ap;
    BAMD_PRO_ISSUE(ap, pa);
    const int slot = blockIdx.y, e = moe_expert_of(a.sel, slot, a.n_expert);
    const uint8_t * wG = (const uint8_t *) a.wg + (size_t) e * a.stride_gu, * wU = (const uint8_t *) a.wu + (size_t) e * a.stride_gu;
    float * out = a.h + (size_t) slot * a.F;
    const int wave = wave_id(), nrg = a.F >> 3;
    const int first = blockIdx.x + gridDim.x * wave, stride = gridDim.x * (int) (blockDim.x >> 6);      // consecutive pairs land on different CUs
    const int count = first < nrg ? (nrg - 1 - first) / stride + 1 : 0;
    unsigned long long best = 0ull;
    if (count == 0) BAMD_PRO_FINISH(ap, pa);                                 // idle waves still owe the block its barriers
    else if ((nb & 7) == 0) stream_segment<TYPE, 8, BAMD_EPI_SILU_MUL, BAMD_PRO_NORM>(wG, wU, nb, first, count, stride, out, nullptr, pa, ap, false, true, best, a.F);
    else if ((nb & 3) == 0) stream_segment<TYPE, 4, BAMD_EPI_SILU_MUL, BAMD_PRO_NORM>(wG, wU, nb, first, count, stride, out, nullptr, pa, ap, false, true, best, a.F);
    else if ((nb & 1) == 0) stream_segment<TYPE, 2, BAMD_EPI_SILU_MUL, BAMD_PRO_NORM>(wG, wU, nb, first, count, stride, out, nullptr, pa, ap, false, true, best, a.F);
    else                    stream_segment<TYPE, 1, BAMD_EPI_SILU_MUL, BAMD_PRO_NORM>(wG, wU, nb, first, count, stride, out, nullptr, pa, ap, false, true, best, a.F);
}

// ===========================================================================================================
// 3. routed down + combine: blockDim = 64 x n_used, wave s = slot s; blockIdx.x = a tile of a.tile consecutive output row-groups
// ===========================================================================================================
// One wave: ring of D records requested, its slot's activations h[s][F] quantised to Q8_K in its own LDS blob (no barrier: nobody else reads it), then the rows
// of row-groups rg0 .. rg0 + count - 1 of its expert streamed in order (they are consecutive in the matrix: one cursor, D records ahead), each output times wgt
// into prod[r * 8 + row].  D divides nb
template <int TYPE, int D>
__device__ __forceinline__ void moe_down_stream(const uint8_t * __restrict__ w, const float * __restrict__ x, int K, int rg0, int count, ActPro<false> & ap,
                                                uint32_t * q8, int * S, float * yd, float wgt, float * prod) {
    typedef typename RecOf<TYPE>::type REC;
    constexpr int RECB = BAMD_RECB_OF(TYPE); static_assert(RECB > 0, "no wave-stream record for this type");
    const int lane = threadIdx.x & 63, nb = K >> 8;
    const bamd_rsrc rs = weight_rsrc(w), rsN = null_rsrc(w);
    const int rgb = nb * RECB, chunks = nb / D;
    REC ring[D];
#pragma unroll
    for (int s = 0; s < D; ++s) load_rec(ring[s], rs, rg0 * rgb + s * RECB, lane);
    // the next batch is requested before the current one is quantised, so a batch's round trip runs behind the arithmetic of the one in front of it; the
    // request behind the last batch is unconditional like every other (issue clamps it to the last block, nobody uses it): the waits stay counted
    for (int i0 = 0; i0 < nb; i0 += BAMD_ACT_BATCH) {
        ActPro<false> nx; nx.template issue<BAMD_ACT_BATCH>(x, nullptr, K, i0 + BAMD_ACT_BATCH, 1, nb);
        ap.template quantize_batch<BAMD_ACT_BATCH>(1.0f, K, i0, q8, S, yd, 1, nb);
        ap = nx;
    }
    for (int r = 0; r < count; ++r) {
        const int rowoff = (rg0 + r) * rgb;
        const bool last = r + 1 >= count;
        RowAcc A = { 0.f, 0.f };
        for (int c = 0; c < chunks; ++c) {
            // the chunk that follows in this wave's sequence: the next one of the row, else the first of the next row-group; behind the wave's last chunk the
            // requests go through the zero-record descriptor (they stay unconditional so that the waits stay counted: stream_segment)
            const bool tail = c + 1 >= chunks && last;
            const bamd_rsrc nrs = tail ? rsN : rs;
            const int nxt = tail ? rowoff : rowoff + (c + 1) * (D * RECB), step = tail ? 0 : RECB;
#pragma unroll
            for (int s = 0; s < D; ++s) {
                pin_rec(ring[s]);
                const Terms T = block_terms(ring[s], c * D + s, lane, q8, S, yd);
                chain_step<TYPE>(A, T.d, T.fs, T.dmin, T.pm);
                load_rec(ring[s], nrs, nxt + s * step, lane);
                if ((s & (BAMD_SCHED_GROUP - 1)) == BAMD_SCHED_GROUP - 1) __builtin_amdgcn_sched_barrier(0);
            }
        }
        const float val = finish_row<TYPE>(A);
        if ((lane & 7) == 0) prod[r * 8 + (lane >> 3)] = val * wgt;          // ggml_mul(experts, weights): rounded before any add
    }
}

template <int TYPE>
__global__ void __launch_bounds__(512) moe_down_kernel(bamd_moe_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int s = wave_id(), lane = threadIdx.x & 63, K = a.F, nb = K >> 8, nrg = a.E >> 3;
    const size_t blob = moe_down_slot_bytes(K);
    uint32_t * q8 = (uint32_t *) (smem + (size_t) s * blob); int * S = (int *) (q8 + nb * 64); float * yd = (float *) (S + nb * 8);
    float * prod0 = (float *) (smem + (size_t) a.n_used * blob), * prod = prod0 + s * a.tile * 8;
    const float * x = a.h + (size_t) s * K;
    ActPro<false> ap;
    ap.template issue<BAMD_ACT_BATCH>(x, nullptr, K, 0, 1, nb);              // the first activation blocks, then the slot's expert id and weight: one round trip
    const int e = moe_expert_of(a.sel, s, a.n_expert);
    const float wgt = ik_ld(a.w + s);
    const uint8_t * w = (const uint8_t *) a.wd + (size_t) e * a.stride_d;
    const int rg0 = blockIdx.x * a.tile, count = nrg - rg0 < a.tile ? nrg - rg0 : a.tile;
    if ((nb & 7) == 0)      moe_down_stream<TYPE, 8>(w, x, K, rg0, count, ap, q8, S, yd, wgt, prod);
    else if ((nb & 3) == 0) moe_down_stream<TYPE, 4>(w, x, K, rg0, count, ap, q8, S, yd, wgt, prod);
    else if ((nb & 1) == 0) moe_down_stream<TYPE, 2>(w, x, K, rg0, count, ap, q8, S, yd, wgt, prod);
    else                    moe_down_stream<TYPE, 1>(w, x, K, rg0, count, ap, q8, S, yd, wgt, prod);
    __syncthreads();
    // the slots' products meet here: one wave adds them in slot order (llama.cpp:8169-8178), then the residual (ggml_add(cur, ffn_inp), :8902)
    if (s == 0) for (int i = lane; i < count * 8; i += 64) {
        float o = prod0[i];
        for (int t = 1; t < a.n_used; ++t) o = o + prod0[t * a.tile * 8 + i];
        const int row = rg0 * 8 + i;
        ik_st(a.out + row, o + ik_ld(a.x + row));
    }
}

// ===========================================================================================================
// launchers
// ===========================================================================================================
static bool moe_shape_ok(const bamd_moe_args & a) {
    return a.E > 0 && a.E % 256 == 0 && a.F > 0 && a.F % 256 == 0 && a.n_expert >= 8 && a.n_expert % 8 == 0 && a.n_expert <= BAMD_MOE_MAX_EXPERT &&
           a.n_used >= 1 && a.n_used <= BAMD_MOE_MAX_USED && a.n_used <= a.n_expert;
}
static int moe_down_tile(int E, int n_cu) {
    const int nrg = E >> 3, cus = n_cu > 0 ? n_cu : 256;
    const int t = (nrg + cus - 1) / cus;
    return t < 1 ? 1 : t < BAMD_MOE_DOWN_TILE_MAX ? t : BAMD_MOE_DOWN_TILE_MAX;
}
int bamd_moe_shape_supported(int E, int F, int n_expert, int n_used, int type_d) {
    bamd_moe_args a; memset(&a, 0, sizeof a); a.E = E; a.F = F; a.n_expert = n_expert; a.n_used = n_used;
    return moe_shape_ok(a) && E <= bamd_flt_max_k(BAMD_F32) && moe_router_lds(E) <= (size_t) BAMD_LDS_CU_BYTES &&
           (bamd_is_flt(type_d) ? bamd_moe_flt_down_fits(type_d, F, n_used) : moe_down_lds(F, n_used, BAMD_MOE_DOWN_TILE_MAX) <= (size_t) BAMD_LDS_CU_BYTES);
}
int bamd_launch_moe_router(const bamd_moe_args & a, hipStream_t s) {
    if (!bamd_moe_shape_supported(a.E, a.F, a.n_expert, a.n_used)) return 1;
    const size_t lds = moe_router_lds(a.E);
    bamd_allow_lds(moe_router_kernel, lds);
    BAMD_LAUNCH(moe_router_kernel, dim3(1), dim3(512), lds, s, a);
    return 0;
}
int bamd_launch_moe_gate_up(const bamd_moe_args & a, int n_cu, hipStream_t s) {
    if (!bamd_moe_shape_supported(a.E, a.F, a.n_expert, a.n_used, a.type_d) || a.stride_gu >= (size_t) 0x7fffffff) return 1;
    // pairs per wave so that slots x tiles fills the chip's wave slots once: tiles = the row-group pairs of a slot over (8 waves x pairs per wave)
    const int nrg = a.F >> 3, cus = n_cu > 0 ? n_cu : 256;
    const int per_wave = (nrg * a.n_used + 8 * cus - 1) / (8 * cus);
    const int tiles = (nrg + 8 * per_wave - 1) / (8 * per_wave);
    if (bamd_is_flt(a.type_gu)) return bamd_launch_moe_gate_up_flt(a, tiles, s);      // F16 / F32 / BF16 experts: bamd_moe_flt.hip
    // the 32-weight block families: bamd_moe_b32.h, a code object each
    if (bamd_is_b32(a.type_gu)) return bamd_is_q1(a.type_gu) ? bamd_launch_moe_gate_up_b32_q1(a, tiles, s) : a.type_gu == BAMD_IQ4_NL ? bamd_launch_moe_gate_up_b32_nl(a, tiles, s) : bamd_launch_moe_gate_up_b32_q0(a, tiles, s);
    return with_kquant(a.type_gu, [&](auto T) -> bool {
        BAMD_LAUNCH((moe_gate_up_kernel<decltype(T)::value>), dim3(tiles, a.n_used), dim3(512), act_lds_bytes(a.E), s, a); return true; }) ? 0 : 1;
}
int bamd_launch_moe_down(const bamd_moe_args & a0, int n_cu, hipStream_t s) {
    if (!bamd_moe_shape_supported(a0.E, a0.F, a0.n_expert, a0.n_used, a0.type_d) || a0.stride_d >= (size_t) 0x7fffffff) return 1;
    bamd_moe_args a = a0;
    a.tile = moe_down_tile(a.E, n_cu);
    if (bamd_is_flt(a.type_d)) return bamd_launch_moe_down_flt(a, s);
    if (bamd_is_b32(a.type_d)) return bamd_is_q1(a.type_d) ? bamd_launch_moe_down_b32_q1(a, s) : a.type_d == BAMD_IQ4_NL ? bamd_launch_moe_down_b32_nl(a, s) : bamd_launch_moe_down_b32_q0(a, s);
    const int nrg = a.E >> 3, grid = (nrg + a.tile - 1) / a.tile;
    const size_t lds = moe_down_lds(a.F, a.n_used, a.tile);
    return with_kquant(a.type_d, [&](auto T) -> bool {
        bamd_allow_lds(moe_down_kernel<decltype(T)::value>, lds);
        BAMD_LAUNCH((moe_down_kernel<decltype(T)::value>), dim3(grid), dim3(64 * a.n_used), lds, s, a); return true; }) ? 0 : 1;
}
