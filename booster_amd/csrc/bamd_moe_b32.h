// bamd_moe_b32.h — the routed launches of a mixture-of-experts decode step (bamd_moe.hip: what they compute, what is restated) for experts of the 32-weight block
// formats: Q8_0 / Q4_0 / Q5_0 and IQ4_NL on Q8_0 activations, Q4_1 / Q5_1 on Q8_1 activations.  The router launch is the K-quant one (it reads no expert matrix).
//   routed gate/up  grid (row-group tiles, slot), 8 waves, one wave per row-group pair (mode A of bamd_matvec_b32.h).  The activation requests of RMSNorm + Q8_0 / Q8_1
//                   go out first, the expert id right behind them; the weight ring — which needs the id — is requested from base + sel[slot] * stride_gu in front of the
//                   prologue's arithmetic.  silu(gate) * up -> h[slot][F]
//   routed down     block = 64 x n_used, wave s = slot s.  A wave quantises its own h[s] row into its own LDS image: ActProQ0's per-block arithmetic with the blocks
//                   of the row dealt to ONE wave (block stride 1), so a block's maximum, its bytes and — Q8_1 — its quant sum never leave the wave and no workgroup
//                   barrier stands between the quantiser and the stream (nobody else reads the image).  Then the rows of its expert, each product times the slot
//                   weight before any add; one barrier; wave 0 adds the slots in order and the residual last
// The image of a slot is the b32 form, q8[nb][64] | ys[nb][8]: 288 bytes per 256 values (the Q8_K form keeps 4 more), and the LDS of the down launch is sized by it.
// ONE source, THREE translation units, a code object per family as the dense mat-vec has them: bamd_moe_b32_q0.hip (Q8_0 / Q4_0 / Q5_0), bamd_moe_b32_q1.hip
// (Q4_1 / Q5_1), bamd_moe_b32_nl.hip (IQ4_NL, two accumulators per lane).  type_gu and type_d are independent: a launch of either kind may be K-quant while the
// other comes here (bamd_launch_moe_gate_up / bamd_launch_moe_down route by family).  Numerics, records and the chains: bamd_b32_device.h.
#pragma once
#include "bamd_moe_device.h"
#include "bamd_b32_device.h"

// LDS of the down launch: one image per slot, then the weighted outputs [n_used][tile * 8]
constexpr size_t moe_b32_slot_bytes(int F) { return (size_t) (F >> 8) * (256 + 32); }
constexpr size_t moe_b32_down_lds(int F, int n_used, int tile) { return (size_t) n_used * moe_b32_slot_bytes(F) + (size_t) n_used * tile * 8 * 4; }
#define BAMD_MOE_B32_DOWN_TILE_MAX 8

// one record of the ring against the image: the lane's chain(s) and, with a minimum, the row's scalar chain (the statements of b32_stream, bamd_matvec_b32.h).
// Uses lane, q8, ys and the accumulators acc, acc2, summs of the loop it stands in.  A macro, not a force-inlined helper that takes the accumulators by reference:
// as bamd_matvec_b32.h notes for its own loop, that costs registers in the family with a minimum (measured here: gate/up Q4_1 213 -> 222 VGPRs, Q5_1 250 -> 253,
// down Q5_1 209 -> 211; the other instances unchanged)
#define BAMD_MOE_B32_STEP(R_, CI_) do { \
        float sc[8], fd[8]; \
        if constexpr (b32_has_min(TYPE)) { \
            float ms[8]; \
            b32_terms(R_, CI_, lane, q8, ys, sc, fd, ms); \
            b32_chain8(acc, sc, fd); \
            b32_summs8(summs, ms); \
        } else { \
            b32_terms(R_, CI_, lane, q8, ys, sc, fd); \
            if constexpr (b32_two_acc(TYPE)) b32_chain8(acc, acc2, sc, fd); \
            else b32_chain8(acc, sc, fd); \
        } } while (0)

// ===========================================================================================================
// routed gate/up: the pairs first, first + stride, .. of expert matrices wG / wU.  ap holds the wave's first activation batch, already requested
// ===========================================================================================================
template <int TYPE, int D>
__device__ __forceinline__ void moe_b32_gate_up_stream(const uint8_t * __restrict__ wG, const uint8_t * __restrict__ wU, int nb, int first, int count, int stride,
                                                       float * __restrict__ out, ActProQ0<true> & ap, const bamd_moe_args & a, uint32_t * q8, float * ys, double * red) {
    constexpr int RECB = BAMD_RECB_OF(TYPE);
    constexpr bool MIN = b32_has_min(TYPE);
    const int lane = threadIdx.x & 63;
    const bamd_rsrc rsG = weight_rsrc(wG), rsU = weight_rsrc(wU), rsN = null_rsrc(wG);
    const int rgb = nb * RECB, rg_step = stride * rgb, chunks = nb / D;
    RecB32<TYPE> ring[D];
#pragma unroll
    for (int s = 0; s < D; ++s) load_rec(ring[s], rsG, first * rgb + s * RECB, lane);
    ap.template finish_q0<MIN>(a.x, a.normw, a.eps, a.E, q8, ys, red);
    for (int r = 0; r < count; ++r) {
        const int rg = first + r * stride, rowoff = rg * rgb;
        float gate_val = 0.f;
#pragma unroll
        for (int part = 0; part < 2; ++part) {
            const bool last = part == 1 && r + 1 >= count;
            float acc = 0.f, acc2 = 0.f, summs = 0.f;
            for (int c = 0; c < chunks; ++c) {
                // what follows this chunk in the wave's sequence: the row's next chunk; behind the gate row the up row of the pair; behind the up row the gate row
                // of the wave's next pair; behind the wave's last chunk the zero-record descriptor (the requests stay unconditional: the waits stay counted)
                const bool inrow = c + 1 < chunks, tail = !inrow && last;
                const bamd_rsrc nrs = tail ? rsN : (inrow ? part == 1 : part == 0) ? rsU : rsG;
                const int nxt = tail ? 0 : inrow ? rowoff + (c + 1) * (D * RECB) : part == 0 ? rowoff : rowoff + rg_step;
#pragma unroll
                for (int s = 0; s < D; ++s) {
                    pin_rec(ring[s]);
                    BAMD_MOE_B32_STEP(ring[s], c * D + s);
                    load_rec(ring[s], nrs, nxt + s * RECB, lane);
                    if ((s & (BAMD_SCHED_GROUP - 1)) == BAMD_SCHED_GROUP - 1) __builtin_amdgcn_sched_barrier(0);
                }
            }
            const float val = b32_finish_row<MIN>(b32_two_acc(TYPE) ? acc + acc2 : acc, summs);
            if (part == 0) gate_val = val;
            else if ((lane & 7) == 0) ik_st(out + rg * 8 + (lane >> 3), v_silu(gate_val) * val);
        }
    }
}

template <int TYPE>
__global__ void __launch_bounds__(512) moe_b32_gate_up_kernel(bamd_moe_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nb = a.E >> 8, wave = wave_id();
    uint32_t * q8 = (uint32_t *) smem; float * ys = (float *) (q8 + nb * 64); double * red = (double *) (smem + BAMD_ACT_RED_OFF(nb));
    ActProQ0<true> ap;
    ap.issue(a.x, a.normw, a.E, wave);                                       // the activation requests, then the expert id: one round trip
    const int slot = blockIdx.y, e = moe_expert_of(a.sel, slot, a.n_expert);
    const uint8_t * wG = (const uint8_t *) a.wg + (size_t) e * a.stride_gu, * wU = (const uint8_t *) a.wu + (size_t) e * a.stride_gu;
    float * out = a.h + (size_t) slot * a.F;
    const int nrg = a.F >> 3;
    const int first = blockIdx.x + gridDim.x * wave, stride = gridDim.x * (int) (blockDim.x >> 6);      // consecutive pairs land on different CUs
    const int count = first < nrg ? (nrg - 1 - first) / stride + 1 : 0;
    if (count == 0) ap.template finish_q0<b32_has_min(TYPE)>(a.x, a.normw, a.eps, a.E, q8, ys, red);   // idle waves still owe the block its barriers
    else if ((nb & 3) == 0) moe_b32_gate_up_stream<TYPE, 4>(wG, wU, nb, first, count, stride, out, ap, a, q8, ys, red);
    else if ((nb & 1) == 0) moe_b32_gate_up_stream<TYPE, 2>(wG, wU, nb, first, count, stride, out, ap, a, q8, ys, red);
    else                    moe_b32_gate_up_stream<TYPE, 1>(wG, wU, nb, first, count, stride, out, ap, a, q8, ys, red);
}

// ===========================================================================================================
// routed down + combine
// ===========================================================================================================
// One wave: the ring requested, its slot's row x[K] quantised into its own image (a batch of four blocks at a time, the next batch requested before the current one
// is quantised), then the rows of row-groups rg0 .. rg0 + count - 1 of its expert (consecutive in the matrix: one cursor), each output times wgt into prod
template <int TYPE, int D>
__device__ __forceinline__ void moe_b32_down_stream(const uint8_t * __restrict__ w, const float * __restrict__ x, int K, int rg0, int count, ActProQ0<false> & ap,
                                                    uint32_t * q8, float * ys, float wgt, float * prod) {
    constexpr int RECB = BAMD_RECB_OF(TYPE);
    constexpr bool MIN = b32_has_min(TYPE);
    const int lane = threadIdx.x & 63, nb = K >> 8;
    const bamd_rsrc rs = weight_rsrc(w), rsN = null_rsrc(w);
    const int rgb = nb * RECB, chunks = nb / D;
    RecB32<TYPE> ring[D];
#pragma unroll
    for (int s = 0; s < D; ++s) load_rec(ring[s], rs, rg0 * rgb + s * RECB, lane);
    // the one-wave quantiser: blocks i0 .. i0 + 3 of the row (block stride 1, limit nb); a request past the row is clamped to its last block and never stored
    for (int i0 = 0; i0 < nb; i0 += BAMD_ACT_BATCH) {
        ActProQ0<false> nx; nx.template issue<BAMD_ACT_BATCH>(x, nullptr, K, i0 + BAMD_ACT_BATCH, 1, nb);
        ap.template quantize_batch_q0<BAMD_ACT_BATCH, MIN>(1.0f, K, i0, q8, ys, 1, nb);
        ap = nx;
    }
    for (int r = 0; r < count; ++r) {
        const int rowoff = (rg0 + r) * rgb;
        const bool last = r + 1 >= count;
        float acc = 0.f, acc2 = 0.f, summs = 0.f;
        for (int c = 0; c < chunks; ++c) {
            const bool tail = c + 1 >= chunks && last;                       // behind the wave's last chunk: the zero-record descriptor
            const bamd_rsrc nrs = tail ? rsN : rs;
            const int nxt = tail ? 0 : rowoff + (c + 1) * (D * RECB);        // (behind a row's last chunk this is the first chunk of the next row-group)
#pragma unroll
            for (int s = 0; s < D; ++s) {
                pin_rec(ring[s]);
                BAMD_MOE_B32_STEP(ring[s], c * D + s);
                load_rec(ring[s], nrs, nxt + s * RECB, lane);
                if ((s & (BAMD_SCHED_GROUP - 1)) == BAMD_SCHED_GROUP - 1) __builtin_amdgcn_sched_barrier(0);
            }
        }
        const float val = b32_finish_row<MIN>(b32_two_acc(TYPE) ? acc + acc2 : acc, summs);
        if ((lane & 7) == 0) prod[r * 8 + (lane >> 3)] = val * wgt;          // ggml_mul(experts, weights): rounded before any add
    }
}

template <int TYPE>
__global__ void __launch_bounds__(512) moe_b32_down_kernel(bamd_moe_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int s = wave_id(), lane = threadIdx.x & 63, K = a.F, nb = K >> 8, nrg = a.E >> 3;
    const size_t img = moe_b32_slot_bytes(K);
    uint32_t * q8 = (uint32_t *) (smem + (size_t) s * img); float * ys = (float *) (q8 + nb * 64);
    float * prod0 = (float *) (smem + (size_t) a.n_used * img), * prod = prod0 + s * a.tile * 8;
    const float * x = a.h + (size_t) s * K;
    ActProQ0<false> ap;
    ap.template issue<BAMD_ACT_BATCH>(x, nullptr, K, 0, 1, nb);              // the first activation blocks, then the slot's expert id and weight: one round trip
    const int e = moe_expert_of(a.sel, s, a.n_expert);
    const float wgt = ik_ld(a.w + s);
    const uint8_t * w = (const uint8_t *) a.wd + (size_t) e * a.stride_d;
    const int rg0 = blockIdx.x * a.tile, count = nrg - rg0 < a.tile ? nrg - rg0 : a.tile;
    if ((nb & 3) == 0)      moe_b32_down_stream<TYPE, 4>(w, x, K, rg0, count, ap, q8, ys, wgt, prod);
    else if ((nb & 1) == 0) moe_b32_down_stream<TYPE, 2>(w, x, K, rg0, count, ap, q8, ys, wgt, prod);
    else                    moe_b32_down_stream<TYPE, 1>(w, x, K, rg0, count, ap, q8, ys, wgt, prod);
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
// launchers of a family's type list, instantiated by its translation unit.  The callers (bamd_moe.hip) have checked shape and strides and hand over the grid
// ===========================================================================================================
template <int... TYPES> int launch_moe_b32_gate_up(const bamd_moe_args & a, int tiles, hipStream_t s) {
    return with_const(consts<TYPES...>(), a.type_gu, [&](auto T) -> bool {
        BAMD_LAUNCH((moe_b32_gate_up_kernel<decltype(T)::value>), dim3(tiles, a.n_used), dim3(512), act_lds_bytes(a.E), s, a); return true; }) ? 0 : 1;
}
// a.tile set by the caller; 1 also where the images and the product tile do not fit the LDS of a CU
template <int... TYPES> int launch_moe_b32_down(const bamd_moe_args & a, hipStream_t s) {
    const int nrg = a.E >> 3, grid = (nrg + a.tile - 1) / a.tile;
    const size_t lds = moe_b32_down_lds(a.F, a.n_used, a.tile);
    if (a.tile < 1 || a.tile > BAMD_MOE_B32_DOWN_TILE_MAX || lds > (size_t) BAMD_LDS_CU_BYTES) return 1;
    return with_const(consts<TYPES...>(), a.type_d, [&](auto T) -> bool {
        bamd_allow_lds(moe_b32_down_kernel<decltype(T)::value>, lds);
        BAMD_LAUNCH((moe_b32_down_kernel<decltype(T)::value>), dim3(grid), dim3(64 * a.n_used), lds, s, a); return true; }) ? 0 : 1;
}
