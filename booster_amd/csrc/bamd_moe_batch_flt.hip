// bamd_moe_batch_flt.hip — launches 3 / 4 and 5 / 6 of a mixture-of-experts prompt micro-batch (bamd_moe_batch.hip: the seven launches, what they compute) for
// UNQUANTISED experts, F16 / F32 / BF16, on the VALU.  Router, grouping, tile table and combine are the launches of bamd_moe_batch.hip unchanged.
//   3 / 5  one workgroup per row: the prologue of the routed gate/up launch (XfActPro, with ffn_norm for launch 3, plain for the rows of h) leaves the row's image in
//          LDS and the workgroup copies it out: the blob holds one image per row, bamd_moe_flt_image_bytes apart, in the order the chain lanes read it
//   4 / 6  grid (tile, row slot), 8 waves; a tile = up to TT pairs of ONE expert, their images gathered into LDS as the integer-dot kernels gather theirs (the TOKEN's
//          image for gate/up, the pair's own row of h for down).  A wave walks row-groups; every chunk of a weight row is read ONCE, widened once and applied to the TT
//          pairs of the tile.  Per (row, pair) the arithmetic is the chain and the tail of the routed decode launches (bamd_moe_flt_device.h): the bits of token by
//          token.  Behind a wave's last chunk the requests go through the zero-record descriptor
// TT is 8 while eight images of the row length fit the LDS of a CU, else 4 (bamd_moe_flt_group_tt; 0: not even four fit, and the engine goes token by token).
// Registers at TT = 8: 32 accumulators per lane (4 rows x 8 pairs), one chunk widened to 32 floats, a ring of one chunk; at TT = 4 the ring is two chunks deep.  The
// gate values of a row-group wait for its up rows in the wave's own corner of LDS, written and read by the same lanes: held in registers they took the F16 and BF16
// gate/up instances at TT = 8 past 256 VGPRs (40 and 92 bytes of scratch).  There is no matrix-core variant of this kernel: BAMD_PREFILL_MOE leaves these types here.
#include "bamd_moe_device.h"
#include "bamd_moe_flt_device.h"
#include "bamd_kernels.h"
#include "bamd_mv_select.h"

// LDS of a grouped mat-mul workgroup: TT images, the TT pair ids, then per wave the gate values [TT][8] of the row-group in hand
constexpr size_t moe_flt_group_lds(int wt, int K, int tt) { return (size_t) tt * xf_image_bytes(wt, K) + 64 + (size_t) 8 * tt * 8 * 4; }
int bamd_moe_flt_group_tt(int type, int K) {
    return !bamd_is_flt(type) ? 0 : moe_flt_group_lds(type, K, BAMD_TT) <= (size_t) BAMD_LDS_CU_BYTES ? BAMD_TT : moe_flt_group_lds(type, K, 4) <= (size_t) BAMD_LDS_CU_BYTES ? 4 : 0;
}

// ===========================================================================================================
// 3. / 5. the images: blockIdx.x = row
// ===========================================================================================================
template <int WT, bool NORM>
__global__ void __launch_bounds__(512) moe_flt_act_batch_kernel(const float * __restrict__ x, const float * __restrict__ nw, float eps, int K, uint8_t * __restrict__ blob) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double * red = (double *) (smem + xf_image_bytes(WT, K));
    const float * xr = x + (size_t) blockIdx.x * K;
    XfActPro<WT> ap;
    ap.issue(xr, K);
    ap.template finish<NORM>(xr, nw, eps, K, smem, red);
    const int n16 = (int) (xf_image_bytes(WT, K) / 16);
    uint4 * dst = (uint4 *) (blob + (size_t) blockIdx.x * xf_image_bytes(WT, K));
    for (int i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = ((const uint4 *) smem)[i];
}
int bamd_launch_moe_act_batch_flt(int type, const float * x, const float * nw, float eps, int K, int rows, void * blob, hipStream_t s) {
    if (!bamd_is_flt(type) || K <= 0 || K % 256 || rows < 1) return 1;
    const size_t lds = xf_image_bytes(type, K) + 16 * sizeof(double);
    if (lds > (size_t) BAMD_LDS_CU_BYTES) return 1;
    return with_const(consts<BAMD_F16, BAMD_F32, BAMD_BF16>(), type, [&](auto T) -> bool {
        constexpr int WT = decltype(T)::value;
        auto go = [&](auto kernel) { bamd_allow_lds(kernel, lds); hipLaunchKernelGGL(kernel, dim3(rows), dim3(512), lds, s, x, nw, eps, K, (uint8_t *) blob); };
        if (nw) go(moe_flt_act_batch_kernel<WT, true>); else go(moe_flt_act_batch_kernel<WT, false>);
        return true; }) ? 0 : 1;
}

// ===========================================================================================================
// 4. / 6. the grouped mat-muls
// ===========================================================================================================
// the row-groups first, first + stride, .. of one expert.  GU: gate (wA) then up (wB) per row-group, silu(gate) * up stored; else the value times the pair's weight,
// rounded (ggml_mul before any add).  Token u of the tile is pair prs[u], its value goes to row prs[u] of out; slots beyond nt hold the last pair's image again and
// are never stored
template <int WT, int D, bool GU, int TT>
__device__ __forceinline__ void moe_flt_group_segment(const uint8_t * __restrict__ wA, const uint8_t * __restrict__ wB, int nch, int first, int count, int stride,
                                                      float * __restrict__ out, int ldo, const float * __restrict__ wgt, const int * prs, int nt,
                                                      const unsigned char * acts, size_t ib, float * gv) {
    constexpr int NPARTS = GU ? 2 : 1;
    const int lane = threadIdx.x & 63;
    const bamd_rsrc rsA = weight_rsrc(wA), rsB = GU ? weight_rsrc(wB) : rsA, rsN = null_rsrc(wA);
    const int rgb = nch * BAMD_FLT_CHB, rg_step = stride * rgb, groups = nch / D, i16 = (int) (ib >> 4);
    const uint4 * X = (const uint4 *) acts + (lane & 31);
    FltChunk R[D];
#pragma unroll
    for (int s = 0; s < D; ++s) flt_load(R[s], rsA, first * rgb + s * BAMD_FLT_CHB, lane);
    for (int r = 0; r < count; ++r) {
        const int rg = first + r * stride, rowoff = rg * rgb;
#pragma unroll
        for (int part = 0; part < NPARTS; ++part) {
            const bool gate = GU && part == 0;
            const bool last = !gate && r + 1 >= count;
            float acc[TT][4];
#pragma unroll
            for (int u = 0; u < TT; ++u) { acc[u][0] = 0.f; acc[u][1] = 0.f; acc[u][2] = 0.f; acc[u][3] = 0.f; }
            for (int c = 0; c < groups; ++c) {
                const bool inrow = c + 1 < groups, tail = !inrow && last;
                const bamd_rsrc nrs = tail ? rsN : (inrow ? part == 1 : gate) ? rsB : rsA;
                const int nxt = tail ? 0 : inrow ? rowoff + (c + 1) * (D * BAMD_FLT_CHB) : gate ? rowoff : rowoff + rg_step;
#pragma unroll
                for (int s = 0; s < D; ++s) {
                    XfChunkW<WT> W;
                    xf_widen_chunk<WT>(W, R[s]);
                    flt_load(R[s], nrs, nxt + s * BAMD_FLT_CHB, lane);
#pragma unroll
                    for (int u = 0; u < TT; ++u) {
                        float x[xf_steps(WT)];
                        xf_widen<WT>(x, X[u * i16 + (c * D + s) * 32]);
                        xf_chain<WT>(acc[u], W, x);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
#pragma unroll
            for (int u = 0; u < TT; ++u) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float val = xf_finish<WT>(acc[u][q]);
                    if ((lane & 31) != 0) continue;
                    const int r8 = 2 * q + (lane >> 5);
                    if (gate) { gv[u * 8 + r8] = val; continue; }
                    if (u < nt) {
                        const int p = prs[u], row = rg * 8 + r8;
                        out[(size_t) p * ldo + row] = GU ? v_silu(gv[u * 8 + r8]) * val : val * wgt[p];
                    }
                }
            }
        }
    }
}

// GU: K = E, rows = F, the image of a pair is its TOKEN's (pair / n_used); else K = F, rows = E, the image is the pair's own row of h
template <int WT, bool GU, int TT>
__global__ void __launch_bounds__(512) moe_flt_group_mm_kernel(bamd_moe_group_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int npairs = a.T * a.m.n_used;
    if ((int) blockIdx.x >= __builtin_amdgcn_readfirstlane(a.tiles[0])) return;          // past the table: which tiles exist is device data
    const int32_t * te = a.tiles + 4 + 4 * blockIdx.x;
    // what the grouping launch wrote, bounded again where it becomes an address
    int e = __builtin_amdgcn_readfirstlane(te[0]), first = __builtin_amdgcn_readfirstlane(te[1]), nt = __builtin_amdgcn_readfirstlane(te[2]);
    e = e < 0 ? 0 : e; e = e < a.m.n_expert ? e : a.m.n_expert - 1;
    nt = nt < 1 ? 1 : nt; nt = nt < TT ? nt : TT; nt = nt < npairs ? nt : npairs;
    first = first < 0 ? 0 : first; first = first <= npairs - nt ? first : npairs - nt;
    const int K = GU ? a.m.E : a.m.F, nrows = GU ? a.m.F : a.m.E, nch = K / xf_chunk_k(WT);
    const size_t ib = xf_image_bytes(WT, K);
    int * prs = (int *) (smem + (size_t) TT * ib);
    if (threadIdx.x < TT) {
        int p = a.lists[first + ((int) threadIdx.x < nt ? (int) threadIdx.x : nt - 1)];
        p = p < 0 ? 0 : p; prs[threadIdx.x] = p < npairs ? p : npairs - 1;
    }
    __syncthreads();
    {   // the tile's images -> LDS
        const int n16 = (int) (ib / 16);
        for (int i = threadIdx.x; i < n16 * TT; i += blockDim.x) {
            const int u = i / n16, k = i - u * n16;
            const int src = GU ? prs[u] / a.m.n_used : prs[u];
            ((uint4 *) smem)[(size_t) u * n16 + k] = ((const uint4 *) (a.blob + (size_t) src * ib))[k];
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
    float * gv = (float *) (smem + (size_t) TT * ib + 64) + wave * TT * 8;
    if (TT < 8 && (nch & 1) == 0) moe_flt_group_segment<WT, (TT < 8 ? 2 : 1), GU, TT>(wA, wB, nch, slot, count, stride, out, nrows, a.m.w, prs, nt, smem, ib, gv);
    else                          moe_flt_group_segment<WT, 1, GU, TT>(wA, wB, nch, slot, count, stride, out, nrows, a.m.w, prs, nt, smem, ib, gv);
}

// gu: launch 4 (type_gu) or 6 (type_d), a.blob holding that launch's images; grid and a.tt from bamd_launch_moe_ffn_batch.  1 = no such type here, or a tile that
// does not fit (nothing launched)
int bamd_launch_moe_group_mm_flt(const bamd_moe_batch_args & a, int gu, dim3 grid, hipStream_t s) {
    const int type = gu ? a.m.type_gu : a.m.type_d, K = gu ? a.m.E : a.m.F;
    if ((a.tt != BAMD_TT && a.tt != 4) || a.tt > bamd_moe_flt_group_tt(type, K)) return 1;
    const size_t lds = moe_flt_group_lds(type, K, a.tt);
    return with_const(consts<BAMD_F16, BAMD_F32, BAMD_BF16>(), type, [&](auto T) -> bool {
        constexpr int WT = decltype(T)::value;
        auto go = [&](auto kernel) { bamd_allow_lds(kernel, lds); hipLaunchKernelGGL(kernel, grid, dim3(512), lds, s, a); };
        if (gu) { if (a.tt == BAMD_TT) go(moe_flt_group_mm_kernel<WT, true, BAMD_TT>); else go(moe_flt_group_mm_kernel<WT, true, 4>); }
        else    { if (a.tt == BAMD_TT) go(moe_flt_group_mm_kernel<WT, false, BAMD_TT>); else go(moe_flt_group_mm_kernel<WT, false, 4>); }
        return true; }) ? 0 : 1;
}
