// bamd_moe_flt.hip — the routed launches of a mixture-of-experts decode step (bamd_moe.hip: what they compute) for UNQUANTISED experts, F16 / F32 / BF16, and the
// load-time repack of such an expert matrix.  Numerics, the chain lanes, the activation images and the tail: bamd_moe_flt_device.h.  The router launch is the
// K-quant one (it reads no expert matrix).  type_gu and type_d are independent: a launch of either kind may be of another family while the other comes here
// (bamd_launch_moe_gate_up / bamd_launch_moe_down route by family).
//   routed gate/up  grid (row-group tiles, slot), 8 waves.  The first activation requests go out first, the expert id right behind them, and the first chunks of the
//                   weight stream — which needs the id — are requested from base + sel[slot] * stride_gu in front of the prologue's arithmetic.  The prologue leaves
//                   ONE image of the normed row in LDS, in the type's form (f16, f32 or bf16 bits; there is no block quantiser).  A wave carries the gate and the
//                   up row-group of the same rows: one LDS read of a chunk's activations serves both chains, eight accumulators per lane.  Its row-groups are one
//                   sequence of chunks, each slot of the ring requested again as soon as it is consumed; behind the last one the requests go through the
//                   zero-record descriptor.  silu(gate) * up -> h[slot][F]
//   routed down     block = 64 x n_used, wave s = slot s.  A wave converts its own h[s] row into its own image (nobody else reads it: no workgroup barrier in front
//                   of the stream), then streams the rows of its expert, each product times the slot weight before any add; one barrier; wave 0 adds the slots in
//                   order and the residual last (the statement order of bamd_moe.hip)
// LDS: gate/up keeps one image of E values and 16 reduction slots; down keeps n_used images of F values (2 or 4 bytes a value) and the product tile.  The images of
// the down launch are what bounds the shape: bamd_moe_flt_down_fits, asked by the loader.  The kernels keep the inter-kernel rules of bamd_device.h (ik_* for
// activations, outputs and residual, nt buffer loads for weights only) and launch through BAMD_LAUNCH.
#include "bamd_moe_device.h"
#include "bamd_moe_flt_device.h"
#include "bamd_aql.h"
#include "bamd_kernels.h"
#include "bamd_mv_select.h"

// ---- repack: one expert matrix, GGUF row-major -> records of 8 rows x 256 weights.  Request q of a chunk at q * 1024 + lane * 16, wave lane (h, c) = row 2q + h,
// chain lane c.  F16: a record is one chunk, the lane's eight halves are w[row][256b + 32i + c], i = 0..7 — the dense BF16 record, which BF16 experts take from
// the dense repack.  F32: a record is two chunks n = 0, 1, the lane's four floats are w[row][256b + 128n + 32i + c], i = 0..3.  One thread per request ----
__global__ void __launch_bounds__(256) repack_moe_flt_kernel(const uint8_t * __restrict__ raw, uint8_t * __restrict__ dst, int type, int nrows, int K) {
    const int recb = bamd_record_bytes_repack(type), per = recb >> 4, nb = K >> 8;
    const int64_t idx = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = (int64_t) ((nrows + 7) >> 3) * nb * per;
    if (idx >= total) return;
    const int u = (int) (idx % per), rq = u >> 6, lane = u & 63, q = rq & 3, n = rq >> 2;
    const int64_t rec = idx / per;
    const int ib = (int) (rec % nb), rg = (int) (rec / nb);
    const int row = rg * 8 + 2 * q + (lane >> 5), c = lane & 31;
    uint32_t out[4] = { 0u, 0u, 0u, 0u };
    if (row < nrows) {
        if (type == BAMD_F32) for (int t = 0; t < 4; ++t) out[t] = ((const uint32_t *) raw)[(int64_t) row * K + ib * 256 + n * 128 + 32 * t + c];
        else for (int t = 0; t < 8; ++t) out[t >> 1] |= (uint32_t) ((const unsigned short *) raw)[(int64_t) row * K + ib * 256 + 32 * t + c] << (16 * (t & 1));
    }
    *(uint4 *) (dst + rec * recb + (int64_t) rq * 1024 + lane * 16) = make_uint4(out[0], out[1], out[2], out[3]);
}
void bamd_launch_repack_expert(const void * raw, void * dst, int type, int nrows, int K, hipStream_t s) {
    if (type != BAMD_F32 && type != BAMD_F16) { bamd_launch_repack(raw, dst, type, nrows, K, s); return; }      // every other type: the record of the dense matrices
    const int64_t n = (int64_t) ((nrows + 7) >> 3) * (K >> 8) * (bamd_record_bytes(type) >> 4);
    hipLaunchKernelGGL(repack_moe_flt_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, s, (const uint8_t *) raw, (uint8_t *) dst, type, nrows, K);
}

// LDS of the gate/up launch: the image, 16 f64 reduction slots.  Of the down launch: one image per slot, then the weighted outputs [n_used][tile * 8]
constexpr size_t moe_flt_gu_lds(int wt, int E) { return xf_image_bytes(wt, E) + 16 * sizeof(double); }
constexpr size_t moe_flt_down_lds(int wt, int F, int n_used, int tile) { return (size_t) n_used * xf_image_bytes(wt, F) + (size_t) n_used * tile * 8 * 4; }
#define BAMD_MOE_FLT_DOWN_TILE_MAX 8
int bamd_moe_flt_down_fits(int type, int F, int n_used) {
    return bamd_is_flt(type) && F > 0 && n_used >= 1 && moe_flt_down_lds(type, F, n_used, BAMD_MOE_FLT_DOWN_TILE_MAX) <= (size_t) BAMD_LDS_CU_BYTES;
}

// ===========================================================================================================
// routed gate/up: the pairs first, first + stride, .. of expert matrices wG / wU.  ap holds the first activation requests
// ===========================================================================================================
template <int WT, int D>
__device__ __forceinline__ void moe_flt_gate_up_stream(const uint8_t * __restrict__ wG, const uint8_t * __restrict__ wU, int first, int count, int stride,
                                                       float * __restrict__ out, XfActPro<WT> & ap, const bamd_moe_args & a, unsigned char * img, double * red) {
    const int lane = threadIdx.x & 63;
    const int nch = a.E / xf_chunk_k(WT), rgb = nch * BAMD_FLT_CHB, rg_step = stride * rgb, groups = nch / D;
    const bamd_rsrc rsG = weight_rsrc(wG), rsU = weight_rsrc(wU), rsN = null_rsrc(wG);
    FltChunk G[D], U[D];
#pragma unroll
    for (int s = 0; s < D; ++s) { flt_load(G[s], rsG, first * rgb + s * BAMD_FLT_CHB, lane); flt_load(U[s], rsU, first * rgb + s * BAMD_FLT_CHB, lane); }
    ap.template finish<true>(a.x, a.normw, a.eps, a.E, img, red);
    const uint4 * X = (const uint4 *) img + (lane & 31);
    for (int r = 0; r < count; ++r) {
        const int rg = first + r * stride, rowoff = rg * rgb;
        const bool last = r + 1 >= count;
        float accG[4] = { 0.f, 0.f, 0.f, 0.f }, accU[4] = { 0.f, 0.f, 0.f, 0.f };
        for (int c = 0; c < groups; ++c) {
            // what follows in the wave's sequence: the row-group's next chunks, behind its last ones the first of the wave's next row-group, behind the wave's last
            // ones the zero-record descriptor (the requests stay unconditional)
            const bool inrow = c + 1 < groups, tail = !inrow && last;
            const bamd_rsrc nG = tail ? rsN : rsG, nU = tail ? rsN : rsU;
            const int nxt = tail ? 0 : inrow ? rowoff + (c + 1) * (D * BAMD_FLT_CHB) : rowoff + rg_step;
#pragma unroll
            for (int s = 0; s < D; ++s) {
                float x[xf_steps(WT)];
                xf_widen<WT>(x, X[(c * D + s) * 32]);
                XfChunkW<WT> W;
                xf_widen_chunk<WT>(W, G[s]); xf_chain<WT>(accG, W, x);
                flt_load(G[s], nG, nxt + s * BAMD_FLT_CHB, lane);
                xf_widen_chunk<WT>(W, U[s]); xf_chain<WT>(accU, W, x);
                flt_load(U[s], nU, nxt + s * BAMD_FLT_CHB, lane);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float vg = xf_finish<WT>(accG[q]), vu = xf_finish<WT>(accU[q]);
            if ((lane & 31) == 0) ik_st(out + rg * 8 + 2 * q + (lane >> 5), v_silu(vg) * vu);
        }
    }
}

template <int WT>
__global__ void __launch_bounds__(512) moe_flt_gate_up_kernel(bamd_moe_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double * red = (double *) (smem + xf_image_bytes(WT, a.E));
    XfActPro<WT> ap;
    ap.issue(a.x, a.E);                                                      // the activation requests, then the expert id: one round trip
    const int slot = blockIdx.y, e = moe_expert_of(a.sel, slot, a.n_expert), wave = wave_id();
    const uint8_t * wG = (const uint8_t *) a.wg + (size_t) e * a.stride_gu, * wU = (const uint8_t *) a.wu + (size_t) e * a.stride_gu;
    float * out = a.h + (size_t) slot * a.F;
    const int nrg = a.F >> 3, nch = a.E / xf_chunk_k(WT);
    const int first = blockIdx.x + gridDim.x * wave, stride = gridDim.x * (int) (blockDim.x >> 6);      // consecutive pairs land on different CUs
    const int count = first < nrg ? (nrg - 1 - first) / stride + 1 : 0;
    if (count == 0) ap.template finish<true>(a.x, a.normw, a.eps, a.E, smem, red);                      // idle waves still owe the block its barriers
    else if ((nch & 1) == 0) moe_flt_gate_up_stream<WT, 2>(wG, wU, first, count, stride, out, ap, a, smem, red);
    else                     moe_flt_gate_up_stream<WT, 1>(wG, wU, first, count, stride, out, ap, a, smem, red);
}

// ===========================================================================================================
// routed down + combine
// ===========================================================================================================
// One wave: the ring requested, its slot's row x[K] converted into its own image (four requests in flight per lane), then the rows of row-groups rg0 .. rg0 + count - 1
// of its expert (consecutive in the matrix: one cursor), each output times wgt into prod
template <int WT, int D>
__device__ __forceinline__ void moe_flt_down_stream(const uint8_t * __restrict__ w, const float * __restrict__ x, int K, int rg0, int count, unsigned char * img,
                                                    float wgt, float * prod) {
    const int lane = threadIdx.x & 63, n4 = K >> 2;
    const int nch = K / xf_chunk_k(WT), rgb = nch * BAMD_FLT_CHB, groups = nch / D;
    const bamd_rsrc rs = weight_rsrc(w), rsN = null_rsrc(w);
    FltChunk R[D];
#pragma unroll
    for (int s = 0; s < D; ++s) flt_load(R[s], rs, rg0 * rgb + s * BAMD_FLT_CHB, lane);
    const bamd_ik_rsrc rx = ik_rsrc(x);
    for (int k0 = 0; k0 < n4; k0 += 256) {                                   // (K is a multiple of 256: n4 of 64, a lane's requests are inside the row or skipped whole)
        float4 v[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) { const int k4 = k0 + t * 64 + lane; v[t] = ik_ld128f(rx, (uint32_t) (k4 < n4 ? k4 : n4 - 1) * 16u); }
#pragma unroll
        for (int t = 0; t < 4; ++t) { const int k4 = k0 + t * 64 + lane; if (k4 < n4) xf_store4<WT>(img, k4 << 2, v[t]); }
    }
    // the image is this wave's own and LDS keeps a wave's accesses in order: the compiler only has to keep the stores in front of the loads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint4 * X = (const uint4 *) img + (lane & 31);
    for (int r = 0; r < count; ++r) {
        const int rowoff = (rg0 + r) * rgb;
        const bool last = r + 1 >= count;
        float acc[4] = { 0.f, 0.f, 0.f, 0.f };
        for (int c = 0; c < groups; ++c) {
            const bool tail = c + 1 >= groups && last;                       // behind the wave's last chunks: the zero-record descriptor
            const bamd_rsrc nrs = tail ? rsN : rs;
            const int nxt = tail ? 0 : rowoff + (c + 1) * (D * BAMD_FLT_CHB);      // (behind a row-group's last chunks this is the first of the next row-group)
#pragma unroll
            for (int s = 0; s < D; ++s) {
                float xv[xf_steps(WT)];
                xf_widen<WT>(xv, X[(c * D + s) * 32]);
                XfChunkW<WT> W;
                xf_widen_chunk<WT>(W, R[s]); xf_chain<WT>(acc, W, xv);
                flt_load(R[s], nrs, nxt + s * BAMD_FLT_CHB, lane);
                if ((s & 1) == 1) __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float val = xf_finish<WT>(acc[q]);
            if ((lane & 31) == 0) prod[r * 8 + 2 * q + (lane >> 5)] = val * wgt;      // ggml_mul(experts, weights): rounded before any add
        }
    }
}

template <int WT>
__global__ void __launch_bounds__(512) moe_flt_down_kernel(bamd_moe_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int s = wave_id(), lane = threadIdx.x & 63, K = a.F, nrg = a.E >> 3, nch = K / xf_chunk_k(WT);
    const size_t ib = xf_image_bytes(WT, K);
    unsigned char * img = smem + (size_t) s * ib;
    float * prod0 = (float *) (smem + (size_t) a.n_used * ib), * prod = prod0 + s * a.tile * 8;
    const float * x = a.h + (size_t) s * K;
    const int e = moe_expert_of(a.sel, s, a.n_expert);                       // the slot's expert id and weight: one round trip, the ring and the row behind it
    const float wgt = ik_ld(a.w + s);
    const uint8_t * w = (const uint8_t *) a.wd + (size_t) e * a.stride_d;
    const int rg0 = blockIdx.x * a.tile, count = nrg - rg0 < a.tile ? nrg - rg0 : a.tile;
    if ((nch & 3) == 0)      moe_flt_down_stream<WT, 4>(w, x, K, rg0, count, img, wgt, prod);
    else if ((nch & 1) == 0) moe_flt_down_stream<WT, 2>(w, x, K, rg0, count, img, wgt, prod);
    else                     moe_flt_down_stream<WT, 1>(w, x, K, rg0, count, img, wgt, prod);
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
// launchers.  The callers (bamd_moe.hip) have checked shape and strides and hand over the grid / a.tile
// ===========================================================================================================
typedef consts<BAMD_F16, BAMD_F32, BAMD_BF16> moe_flt_types;
int bamd_launch_moe_gate_up_flt(const bamd_moe_args & a, int tiles, hipStream_t s) {
    const size_t lds = moe_flt_gu_lds(a.type_gu, a.E);
    if (!bamd_is_flt(a.type_gu) || lds > (size_t) BAMD_LDS_CU_BYTES) return 1;
    return with_const(moe_flt_types(), a.type_gu, [&](auto T) -> bool {
        bamd_allow_lds(moe_flt_gate_up_kernel<decltype(T)::value>, lds);
        BAMD_LAUNCH((moe_flt_gate_up_kernel<decltype(T)::value>), dim3(tiles, a.n_used), dim3(512), lds, s, a); return true; }) ? 0 : 1;
}
int bamd_launch_moe_down_flt(const bamd_moe_args & a, hipStream_t s) {
    if (a.tile < 1 || a.tile > BAMD_MOE_FLT_DOWN_TILE_MAX || !bamd_moe_flt_down_fits(a.type_d, a.F, a.n_used)) return 1;
    const int nrg = a.E >> 3, grid = (nrg + a.tile - 1) / a.tile;
    const size_t lds = moe_flt_down_lds(a.type_d, a.F, a.n_used, a.tile);
    return with_const(moe_flt_types(), a.type_d, [&](auto T) -> bool {
        bamd_allow_lds(moe_flt_down_kernel<decltype(T)::value>, lds);
        BAMD_LAUNCH((moe_flt_down_kernel<decltype(T)::value>), dim3(grid), dim3(64 * a.n_used), lds, s, a); return true; }) ? 0 : 1;
}
