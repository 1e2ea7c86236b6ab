// bamd_moe_batch_b32.hip — launches 4 and 6 of a mixture-of-experts prompt micro-batch (bamd_moe_batch.hip: the seven launches, what they compute) for experts of the
// 32-weight block formats, on the integer-dot path: Q8_0 / Q4_0 / Q5_0 / IQ4_NL over Q8_0 images, Q4_1 / Q5_1 over Q8_1 images.  Router, grouping, tile table and
// combine are the launches of bamd_moe_batch.hip unchanged; the images come from bamd_launch_quantize_batch_b32 (launches 3 and 5) and have the stride of the Q8_K
// ones, so a tile is gathered as there: the TOKEN's image for gate/up, the pair's own row of h for down.
// Per (row, pair) the arithmetic is the chain of the routed decode launches (bamd_moe_b32.h): the row policy B32Row (bamd_prefill_b32.h) over the pair's image, every
// weight record unpacked once for the TT pairs of a tile.  Behind a wave's last chunk the requests go through the zero-record descriptor (B32Row::NULL_TAIL).
// Registers: a tile of 8 pairs holds 8 (IQ4_NL: 16; with a minimum: 16) accumulators per lane and, in the gate/up instance, 8 gate values.  The ring is ONE record
// deep at 8 pairs for every type and two deep at 4 pairs where the record count is even: with the pair ids and the scattered stores beside the dense kernel's
// state, a second record at 8 pairs is what bamd_prefill_b32.h records as spilling for the types with a minimum and for IQ4_NL, and one rule for all six types
// keeps every instance free of scratch (profiles/moe_b32_codeobj.txt).
#include "bamd_moe_device.h"
#include "bamd_prefill_b32.h"

// moe_group_segment (bamd_moe_batch.hip) for a row policy with the zero-record tail
template <typename P, int D, bool GU, int TT>
__device__ __forceinline__ void moe_b32_group_segment(const uint8_t * __restrict__ wA, const uint8_t * __restrict__ wB, int nb, int first, int count, int stride,
                                                      float * __restrict__ out, int ldo, const float * __restrict__ wgt, const int * prs, int nt,
                                                      const unsigned char * acts, size_t bb) {
    constexpr int RECB = P::RECB; static_assert(RECB > 0 && P::NULL_TAIL, "a 32-weight block row policy");
    constexpr int NPARTS = GU ? 2 : 1;
    const int lane = threadIdx.x & 63;
    const bamd_rsrc rsA = weight_rsrc(wA), rsB = GU ? weight_rsrc(wB) : rsA, rsN = null_rsrc(wA);
    const int rgb = nb * RECB, rg_step = stride * rgb;
    const int chunks = nb / D;
    typename P::Rec ring[D];
#pragma unroll
    for (int s = 0; s < D; ++s) load_rec(ring[s], rsA, first * rgb + s * RECB, lane);
    for (int r = 0; r < count; ++r) {
        const int rg = first + r * stride;
        const int row = rg * 8 + (lane >> 3);
        const int rowoff = rg * rgb;
        float gate_val[TT];
#pragma unroll
        for (int part = 0; part < NPARTS; ++part) {
            const bool gate = GU && part == 0;
            const bool last = !gate && r + 1 >= count;
            typename P::Acc a0[TT], a1[TT], a2[TT];
#pragma unroll
            for (int u = 0; u < TT; ++u) P::zero(a0[u], a1[u], a2[u]);
            for (int c = 0; c < chunks; ++c) {
                const bool inrow = c + 1 < chunks, tail = !inrow && last;
                const bamd_rsrc nrs = tail ? rsN : (inrow ? part == 1 : gate) ? rsB : rsA;
                const int nxt = tail ? 0 : inrow ? rowoff + (c + 1) * (D * RECB) : gate ? rowoff : rowoff + rg_step;
#pragma unroll
                for (int s = 0; s < D; ++s) {
                    pin_rec(ring[s]);
#pragma unroll
                    for (int u = 0; u < TT; ++u) {               // slots beyond nt hold the last pair's image again and are never stored
                        typename P::Work w0, w1, w2;
                        P::step(ring[s], c * D + s, lane, acts + (size_t) u * bb, nb, a0[u], a1[u], a2[u], w0, w1, w2);
                    }
                    load_rec(ring[s], nrs, nxt + s * RECB, lane);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
#pragma unroll
            for (int u = 0; u < TT; ++u) {
                const float val = P::finish(a0[u], a1[u], a2[u]);
                if (gate) { gate_val[u] = val; continue; }
                if ((lane & 7) == 0 && u < nt) {
                    const int p = prs[u];
                    out[(size_t) p * ldo + row] = GU ? v_silu(gate_val[u]) * val : val * wgt[p];      // ggml_mul(experts, weights): rounded before any add
                }
            }
        }
    }
}

// grid (tile, row slot), 8 waves; wave v of row slot y walks the row-groups y + gridDim.y * v, + gridDim.y * 8, ..  GU: K = E, rows = F, the image of a pair is
// its TOKEN's (pair / n_used); else K = F, rows = E, the image is the pair's own row of h
template <int TYPE, bool GU, int TT>
__global__ void __launch_bounds__(512) moe_b32_group_mm_kernel(bamd_moe_group_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    typedef B32Row<TYPE> P;
    const int npairs = a.T * a.m.n_used;
    if ((int) blockIdx.x >= __builtin_amdgcn_readfirstlane(a.tiles[0])) return;          // past the table: which tiles exist is device data
    const int32_t * te = a.tiles + 4 + 4 * blockIdx.x;
    // what the grouping launch wrote, bounded again where it becomes an address
    int e = __builtin_amdgcn_readfirstlane(te[0]), first = __builtin_amdgcn_readfirstlane(te[1]), nt = __builtin_amdgcn_readfirstlane(te[2]);
    e = e < 0 ? 0 : e; e = e < a.m.n_expert ? e : a.m.n_expert - 1;
    nt = nt < 1 ? 1 : nt; nt = nt < TT ? nt : TT; nt = nt < npairs ? nt : npairs;
    first = first < 0 ? 0 : first; first = first <= npairs - nt ? first : npairs - nt;
    const int K = GU ? a.m.E : a.m.F, nrows = GU ? a.m.F : a.m.E, nb = K >> 8;
    const size_t bb = BAMD_BLOB_BYTES(nb);
    int * prs = (int *) (smem + (size_t) TT * bb);
    if (threadIdx.x < TT) {
        int p = a.lists[first + ((int) threadIdx.x < nt ? (int) threadIdx.x : nt - 1)];
        p = p < 0 ? 0 : p; prs[threadIdx.x] = p < npairs ? p : npairs - 1;
    }
    __syncthreads();
    {   // the tile's images -> LDS
        const int n16 = (int) (bb / 16);
        for (int i = threadIdx.x; i < n16 * TT; i += blockDim.x) {
            const int u = i / n16, k = i - u * n16;
            const int src = GU ? prs[u] / a.m.n_used : prs[u];
            ((uint4 *) smem)[(size_t) u * n16 + k] = ((const uint4 *) (a.blob + (size_t) src * bb))[k];
        }
    }
    __syncthreads();
    const int wave = wave_id(), nwaves = (int) (blockDim.x >> 6), nrg = nrows >> 3;
    const int slot = blockIdx.y + gridDim.y * wave, stride = gridDim.y * nwaves;
    const int count = slot < nrg ? (nrg - 1 - slot) / stride + 1 : 0;
    if (count == 0) return;
    const size_t wstride = GU ? a.m.stride_gu : a.m.stride_d;
    const uint8_t * wA = (const uint8_t *) (GU ? a.m.wg : a.m.wd) + (size_t) e * wstride, * wB = GU ? (const uint8_t *) a.m.wu + (size_t) e * wstride : wA;
    float * out = GU ? a.m.h : a.prod;
    if (TT < 8 && (nb & 1) == 0) moe_b32_group_segment<P, (TT < 8 ? 2 : 1), GU, TT>(wA, wB, nb, slot, count, stride, out, nrows, a.m.w, prs, nt, smem, bb);
    else                         moe_b32_group_segment<P, 1, GU, TT>(wA, wB, nb, slot, count, stride, out, nrows, a.m.w, prs, nt, smem, bb);
}

// gu: launch 4 (type_gu) or 6 (type_d).  grid, lds and a.tt come from bamd_launch_moe_ffn_batch, which sizes them for every family alike; 1 = no such type here
int bamd_launch_moe_group_mm_b32(const bamd_moe_batch_args & a, int gu, dim3 grid, size_t lds, hipStream_t s) {
    if (a.tt != BAMD_TT && a.tt != 4) return 1;
    return with_const(consts<BAMD_Q8_0, BAMD_Q4_0, BAMD_Q5_0, BAMD_Q4_1, BAMD_Q5_1, BAMD_IQ4_NL>(), gu ? a.m.type_gu : a.m.type_d, [&](auto T) -> bool {
        constexpr int TYPE = decltype(T)::value;
        auto go = [&](auto kernel) { bamd_allow_lds(kernel, lds); hipLaunchKernelGGL(kernel, grid, dim3(512), lds, s, a); };
        if (gu) { if (a.tt == BAMD_TT) go(moe_b32_group_mm_kernel<TYPE, true, BAMD_TT>); else go(moe_b32_group_mm_kernel<TYPE, true, 4>); }
        else    { if (a.tt == BAMD_TT) go(moe_b32_group_mm_kernel<TYPE, false, BAMD_TT>); else go(moe_b32_group_mm_kernel<TYPE, false, 4>); }
        return true; }) ? 0 : 1;
}
