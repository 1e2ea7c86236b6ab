// bamd_moe_batch.hip — the mixture-of-experts feed-forward of a Mixtral-style Llama layer for a MICRO-BATCH of up to 512 tokens (the engine sends 8 and more: prefill_batch_supported): seven launches in place of the
// dense batched gate/up and ffn_down mat-muls (bamd_prefill.hip), bit-identical per token to the three routed launches of a decode step (bamd_moe.hip).
//   1. batched router   one workgroup per token: the decode router's body, router_select unchanged                              -> sel[T][n_used], w[T][n_used]
//   2. grouping         one workgroup: pairs (token, slot) per expert, exclusive prefix, every expert's pair list in ascending pair order, the tile table
//   3. activations      bamd_launch_quantize_batch with ffn_norm                                                                    -> [T] Q8_K images of K = E
//   4. grouped gate/up  grid (tile, row slot): a tile = up to TT pairs of ONE expert; their tokens' images gathered into LDS         -> h[pair][F] = silu(gate) * up
//   5. quantise h       bamd_launch_quantize_batch over the T * n_used rows of h, no norm                                           -> [T * n_used] Q8_K images of K = F
//   6. grouped down     the same kernel shape with K = F, the image of the pair itself                                              -> prod[pair][E] = down * w[pair]
//   7. combine          out[t] = (prod[t][0] + prod[t][1] + ..) + x[t], left to right
// Which tokens meet which expert is decided on the device, per layer, and never read back: the tile count is device data, the mat-mul grids are sized by the
// host-known bound T * n_used / TT + n_expert (every expert has at most one tile that is not full) and a workgroup whose tile index is past the count exits.
// Tiles of one expert are adjacent in blockIdx.x: the workgroups that share a row slot's weights run together and meet in L2, as in the dense kernel.
// Per (row, pair) the arithmetic is the chain of the decode path: the row policy KqRow (bamd_prefill_kq.h) over the pair's Q8_K image, every weight record
// unpacked once for the TT pairs of a tile; the products are scaled before any add and added in slot order.  What is restated: bamd_moe.hip.
// Launches 4 and 6 have a matrix-core variant behind BAMD_PREFILL_MOE (bamd_moe_batch_mfma.hip: tiles of 64 pairs, the f16 records in place of the Q8_K images).
#include "bamd_moe_device.h"
#include "bamd_prefill_kq.h"

#define BAMD_MOE_BATCH_MAX_PAIRS 4096                      /* 512 tokens x 8 slots */
// LDS of a grouped mat-mul workgroup: TT Q8_K images, then the TT pair ids
constexpr size_t moe_group_lds(int K, int tt) { return (size_t) tt * BAMD_BLOB_BYTES(K >> 8) + 64; }

// ===========================================================================================================
// 1. batched router: blockIdx.x = token
// ===========================================================================================================
// the body of moe_router_kernel (bamd_moe.hip) on row blockIdx.x of x, sel and w.  It is written out here, not shared: inlined from a common function the decode
// router comes out as another sequence of the same instructions, and the decode kernels keep the code objects they have
__global__ void __launch_bounds__(512) moe_router_batch_kernel(bamd_moe_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int K = a.E, lane = threadIdx.x & 63, wave = wave_id(), t = blockIdx.x;
    double * red = (double *) (smem + (size_t) K * 4);
    float * lg = (float *) (smem + (size_t) K * 4 + 16 * sizeof(double));
    float * pv = lg + BAMD_MOE_MAX_EXPERT; int * idx = (int *) (pv + BAMD_MOE_MAX_EXPERT);
    flt_act<true, false>(a.x + (size_t) t * K, a.normw, a.eps, K, smem, red);
    if (wave * 8 < a.n_expert) {
        const int nch = K / BAMD_FLT_CHUNK_K(BAMD_F32), off = wave * nch * BAMD_FLT_CHB;
        const bamd_rsrc rs = weight_rsrc(a.gate_inp), rsN = null_rsrc(a.gate_inp);
        const float4 * X4 = (const float4 *) smem + (lane & 7);
        FltChunk A0, A1;
        flt_load(A0, rs, off, lane);
        float acc = 0.f;
        for (int c = 0; c < nch; c += 2) {
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
    if (threadIdx.x == 0) router_select(lg, pv, idx, a.n_expert, a.n_used, a.sel + (size_t) t * a.n_used, a.w + (size_t) t * a.n_used);
}

// ===========================================================================================================
// 2. grouping: ONE workgroup of 8 waves, wave v = experts v, v + 8, ..  A wave walks the pairs 64 at a time in pair order: the ballot of "this pair meets my
// expert" gives the count (first pass) and, below a lane, its place in the expert's list (second pass) — ascending pair ids, the same layout on every run
// ===========================================================================================================
__global__ void __launch_bounds__(512) moe_group_kernel(const int32_t * __restrict__ sel, int npairs, int n_expert, int tt, int32_t * __restrict__ lists, int32_t * __restrict__ tiles) {
    __shared__ int ssel[BAMD_MOE_BATCH_MAX_PAIRS];
    __shared__ int cnt[BAMD_MOE_MAX_EXPERT], off[BAMD_MOE_MAX_EXPERT], toff[BAMD_MOE_MAX_EXPERT + 1];
    const int lane = threadIdx.x & 63, wave = wave_id(), nwaves = (int) (blockDim.x >> 6);
    for (int p = threadIdx.x; p < npairs; p += blockDim.x) { int e = sel[p]; e = e < 0 ? 0 : e; ssel[p] = e < n_expert ? e : n_expert - 1; }      // (bounded as moe_expert_of bounds it)
    __syncthreads();
    for (int e = wave; e < n_expert; e += nwaves) {
        int c = 0;
        for (int p0 = 0; p0 < npairs; p0 += 64) c += __popcll(__ballot(p0 + lane < npairs && ssel[p0 + lane] == e));
        if (lane == 0) cnt[e] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int o = 0, t = 0;
        for (int e = 0; e < n_expert; ++e) { off[e] = o; toff[e] = t; o += cnt[e]; t += (cnt[e] + tt - 1) / tt; }
        toff[n_expert] = t;
        tiles[0] = t;
    }
    __syncthreads();
    for (int e = wave; e < n_expert; e += nwaves) {
        int base = off[e];
        for (int p0 = 0; p0 < npairs; p0 += 64) {
            const bool hit = p0 + lane < npairs && ssel[p0 + lane] == e;
            const unsigned long long m = __ballot(hit);
            if (hit) lists[base + __popcll(m & ((1ull << lane) - 1ull))] = p0 + lane;
            base += __popcll(m);
        }
    }
    for (int e = 0; e < n_expert; ++e) {
        const int c = cnt[e], nt = toff[e + 1] - toff[e];
        for (int k = threadIdx.x; k < nt; k += blockDim.x) {
            int32_t * te = tiles + 4 + 4 * (toff[e] + k);
            te[0] = e; te[1] = off[e] + k * tt; te[2] = c - k * tt < tt ? c - k * tt : tt; te[3] = 0;
        }
    }
}

// ===========================================================================================================
// 4. / 6. the grouped mat-muls
// ===========================================================================================================
// valu_segment (bamd_prefill_valu.h) with the stores scattered: token u of the tile is pair prs[u], its value goes to row prs[u] of out.  GU: gate (wA) then up
// (wB) per row-group, silu(gate) * up stored; else: the value times the pair's weight, rounded (ggml_mul before any add).  Behind a wave's last chunk the row's
// last record is read again with step 0 (KqRow::NULL_TAIL is false)
template <typename P, int D, bool GU, int TT>
__device__ __forceinline__ void moe_group_segment(const uint8_t * __restrict__ wA, const uint8_t * __restrict__ wB, int nb, int first, int count, int stride,
                                                  float * __restrict__ out, int ldo, const float * __restrict__ wgt, const int * prs, int nt,
                                                  const unsigned char * acts, size_t bb) {
    constexpr int RECB = P::RECB; static_assert(RECB > 0 && !P::NULL_TAIL, "a K-quant row policy");
    constexpr int NPARTS = GU ? 2 : 1;
    const int lane = threadIdx.x & 63;
    const bamd_rsrc rsA = weight_rsrc(wA), rsB = GU ? weight_rsrc(wB) : rsA;
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
            const bool after_b = gate || (last && part == 1);    // behind the part's last chunk: matrix B? and the record
            const int after_off = gate ? rowoff : (last ? rowoff + (nb - 1) * RECB : rowoff + rg_step);
            typename P::Acc a0[TT], a1[TT], a2[TT];
#pragma unroll
            for (int u = 0; u < TT; ++u) P::zero(a0[u], a1[u], a2[u]);
            for (int c = 0; c < chunks; ++c) {
                const bool inrow = c + 1 < chunks;
                const bamd_rsrc nrs = (inrow ? part == 1 : after_b) ? rsB : rsA;
                const int nxt = inrow ? rowoff + (c + 1) * (D * RECB) : after_off;
                const int step = (inrow || !last) ? RECB : 0;
#pragma unroll
                for (int s = 0; s < D; ++s) {
                    pin_rec(ring[s]);
#pragma unroll
                    for (int u = 0; u < TT; ++u) {               // slots beyond nt hold the last pair's image again and are never stored
                        typename P::Work w0, w1, w2;
                        P::step(ring[s], c * D + s, lane, acts + (size_t) u * bb, nb, a0[u], a1[u], a2[u], w0, w1, w2);
                    }
                    load_rec(ring[s], nrs, nxt + s * step, lane);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
#pragma unroll
            for (int u = 0; u < TT; ++u) {
                const float val = P::finish(a0[u], a1[u], a2[u]);
                if (gate) { gate_val[u] = val; continue; }
                if ((lane & 7) == 0 && u < nt) {
                    const int p = prs[u];
                    out[(size_t) p * ldo + row] = GU ? v_silu(gate_val[u]) * val : val * wgt[p];
                }
            }
        }
    }
}

// grid (tile, row slot), 8 waves; wave v of row slot y walks the row-groups y + gridDim.y * v, + gridDim.y * 8, ..  GU: K = E, rows = F, the image of a pair is
// its TOKEN's (pair / n_used); else K = F, rows = E, the image is the pair's own row of h
template <int TYPE, bool GU, int TT>
__global__ void __launch_bounds__(512) moe_group_mm_kernel(bamd_moe_group_args a) {      // (the launch arguments without the matrix-core path's: the argument block, and with it the code object, stays what it was)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    typedef KqRow<TYPE, typename RecOf<TYPE>::type> P;
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
    if ((nb & 3) == 0) moe_group_segment<P, 4, GU, TT>(wA, wB, nb, slot, count, stride, out, nrows, a.m.w, prs, nt, smem, bb);
    else               moe_group_segment<P, 1, GU, TT>(wA, wB, nb, slot, count, stride, out, nrows, a.m.w, prs, nt, smem, bb);
}

// ===========================================================================================================
// 7. combine: blockIdx.x = token; the slots' products in slot order (llama.cpp:8169-8178), then the residual (ggml_add(cur, ffn_inp), :8902)
// ===========================================================================================================
__global__ void __launch_bounds__(256) moe_combine_kernel(const float * __restrict__ prod, const float * __restrict__ x, int E, int n_used, float * __restrict__ out) {
    const size_t t = blockIdx.x;
    const float * p = prod + t * n_used * E;
    for (int row = threadIdx.x; row < E; row += blockDim.x) {
        float o = p[row];
        for (int s = 1; s < n_used; ++s) o = o + p[(size_t) s * E + row];
        out[t * E + row] = o + x[t * E + row];
    }
}

// ===========================================================================================================
// launchers
// ===========================================================================================================
static long long g_moe_batch_runs = 0;
extern "C" __attribute__((visibility("default"))) long long bamd_moe_batch_runs(void) { return g_moe_batch_runs; }
// pairs per tile, the dense kernel's rule on the longer of the two row lengths (ONE tile table serves both mat-muls): 8 while their images fit the LDS, else 4
static int moe_batch_tt(int E, int F) { return moe_group_lds(E > F ? E : F, BAMD_TT) <= (size_t) BAMD_LDS_CU_BYTES ? BAMD_TT : 4; }
static int moe_batch_tile_bound(int T, int n_expert, int n_used, int tt) { return T * n_used / tt + n_expert; }
int bamd_moe_batch_supported(int E, int F, int n_expert, int n_used, int type_gu, int type_d) {
    if (bamd_is_flt(type_gu) && !bamd_moe_flt_group_tt(type_gu, E)) return 0;      // the unquantised types: four images in their own form (bamd_moe_batch_flt.hip)
    if (bamd_is_flt(type_d) && !bamd_moe_flt_group_tt(type_d, F)) return 0;
    return bamd_moe_shape_supported(E, F, n_expert, n_used, type_d) && moe_group_lds(E > F ? E : F, 4) <= (size_t) BAMD_LDS_CU_BYTES;
}
size_t bamd_moe_batch_tiles_bytes(int T, int n_expert, int n_used) { return (size_t) (1 + moe_batch_tile_bound(T, n_expert, n_used, 4)) * 16; }
size_t bamd_moe_batch_blob_bytes(int T, int E, int F, int n_used, int type_gu, int type_d) {
    const size_t x = (size_t) T * (bamd_is_flt(type_gu) ? bamd_moe_flt_image_bytes(type_gu, E) : bamd_blob_bytes(E));
    const size_t h = (size_t) T * n_used * (bamd_is_flt(type_d) ? bamd_moe_flt_image_bytes(type_d, F) : bamd_blob_bytes(F));
    return x > h ? x : h;
}
size_t bamd_moe_batch_blob16_bytes(int T, int E, int F, int n_used) {
    const size_t x = (size_t) T * bamd_blob16_bytes(E), h = (size_t) T * n_used * bamd_blob16_bytes(F);
    return x > h ? x : h;
}

template <bool GU>
static bool launch_group_mm(const bamd_moe_batch_args & a, int n_cu, hipStream_t s) {
    const int K = GU ? a.m.E : a.m.F, nrg = (GU ? a.m.F : a.m.E) >> 3, npairs = a.T * a.m.n_used, cus = n_cu > 0 ? n_cu : 256;
    // row slots: enough workgroups to fill the chip a few times over at the tiles a batch has at least, at least one row-group per wave (valu_mm_geometry)
    int gy = (4 * cus + (npairs + a.tt - 1) / a.tt - 1) / ((npairs + a.tt - 1) / a.tt);
    if (gy * 8 > nrg) gy = (nrg + 7) / 8;
    const dim3 grid(moe_batch_tile_bound(a.T, a.m.n_expert, a.m.n_used, a.tt), gy);
    const size_t lds = moe_group_lds(K, a.tt);
    if (bamd_is_flt(GU ? a.m.type_gu : a.m.type_d)) return bamd_launch_moe_group_mm_flt(a, GU, grid, s) == 0;           // the unquantised types: bamd_moe_batch_flt.hip
    if (bamd_is_b32(GU ? a.m.type_gu : a.m.type_d)) return bamd_launch_moe_group_mm_b32(a, GU, grid, lds, s) == 0;      // the 32-weight block types: bamd_moe_batch_b32.hip
    return with_kquant(GU ? a.m.type_gu : a.m.type_d, [&](auto T) -> bool {
        constexpr int TYPE = decltype(T)::value;
        if (a.tt == BAMD_TT) { bamd_allow_lds(moe_group_mm_kernel<TYPE, GU, BAMD_TT>, lds); hipLaunchKernelGGL((moe_group_mm_kernel<TYPE, GU, BAMD_TT>), grid, dim3(512), lds, s, a); }
        else                 { bamd_allow_lds(moe_group_mm_kernel<TYPE, GU, 4>, lds);       hipLaunchKernelGGL((moe_group_mm_kernel<TYPE, GU, 4>), grid, dim3(512), lds, s, a); }
        return true; });
}
int bamd_launch_moe_ffn_batch(const bamd_moe_batch_args & a0, int n_cu, hipStream_t s) {
    const bamd_moe_args & m = a0.m;
    if (!bamd_moe_batch_supported(m.E, m.F, m.n_expert, m.n_used, m.type_gu, m.type_d) || a0.T < 1 || a0.T * m.n_used > BAMD_MOE_BATCH_MAX_PAIRS) return 1;
    if (m.stride_gu >= (size_t) 0x7fffffff || m.stride_d >= (size_t) 0x7fffffff || !(bamd_is_kquant(m.type_gu) || bamd_is_b32(m.type_gu) || bamd_is_flt(m.type_gu)) ||
        !(bamd_is_kquant(m.type_d) || bamd_is_b32(m.type_d) || bamd_is_flt(m.type_d))) return 1;
    bamd_moe_batch_args a = a0;
    const bool mfma = bamd_moe_batch_mfma_ready(a0);      // launches 4 and 6 on the matrix cores (bamd_moe_batch_mfma.hip): tiles of 64 pairs, f16 records only
    a.tt = mfma ? 64 : moe_batch_tt(m.E, m.F);
    // ONE tile table serves both mat-muls: an unquantised tensor whose eight images do not fit the LDS brings the tile of both down to 4 pairs
    if (bamd_is_flt(m.type_gu) && bamd_moe_flt_group_tt(m.type_gu, m.E) < a.tt) a.tt = 4;
    if (bamd_is_flt(m.type_d) && bamd_moe_flt_group_tt(m.type_d, m.F) < a.tt) a.tt = 4;
    const int npairs = a.T * m.n_used;
    const size_t rlds = moe_router_lds(m.E);
    bamd_allow_lds(moe_router_batch_kernel, rlds);
    hipLaunchKernelGGL(moe_router_batch_kernel, dim3(a.T), dim3(512), rlds, s, m);
    hipLaunchKernelGGL(moe_group_kernel, dim3(1), dim3(512), 0, s, (const int32_t *) m.sel, npairs, m.n_expert, a.tt, a.lists, a.tiles);
    if (mfma) {
        // the f16 records in the form of the tensor that reads them (Q8_K, or the Q8_0 / Q8_1 form of a 32-weight block type at the same stride).  The quantiser of
        // the latter two always writes its int8 image as well, so it gets a.blob; the Q8_K one writes the records alone
        const int fgu = bamd_act_form_of(m.type_gu), fd = bamd_act_form_of(m.type_d);
        bamd_launch_quantize_batch(m.x, m.normw, m.eps, m.E, a.T, fgu == BAMD_ACT_Q8_K ? nullptr : a.blob, a.blob16, s, fgu);
        bamd_launch_moe_gate_up_mfma(a, s);
        bamd_launch_quantize_batch(m.h, nullptr, 0.f, m.F, npairs, fd == BAMD_ACT_Q8_K ? nullptr : a.blob, a.blob16, s, fd);
        bamd_launch_moe_down_mfma(a, s);
        hipLaunchKernelGGL(moe_combine_kernel, dim3(a.T), dim3(256), 0, s, (const float *) a.prod, m.x, m.E, m.n_used, m.out);
        return 0;
    }
    // launches 3 and 5 in the form of the mat-mul that reads them: Q8_K, or Q8_0 / Q8_1 (bamd_launch_quantize_batch_b32) at the same stride, or the f16 / f32 / bf16
    // image of an unquantised expert tensor (bamd_launch_moe_act_batch_flt) at its own
    if (bamd_is_flt(m.type_gu)) { if (bamd_launch_moe_act_batch_flt(m.type_gu, m.x, m.normw, m.eps, m.E, a.T, a.blob, s)) return 1; }
    else bamd_launch_quantize_batch(m.x, m.normw, m.eps, m.E, a.T, a.blob, nullptr, s, bamd_act_form_of(m.type_gu));
    if (!launch_group_mm<true>(a, n_cu, s)) return 1;
    g_moe_batch_runs += 1;
    if (bamd_is_flt(m.type_d)) { if (bamd_launch_moe_act_batch_flt(m.type_d, m.h, nullptr, 0.f, m.F, npairs, a.blob, s)) return 1; }
    else bamd_launch_quantize_batch(m.h, nullptr, 0.f, m.F, npairs, a.blob, nullptr, s, bamd_act_form_of(m.type_d));
    if (!launch_group_mm<false>(a, n_cu, s)) return 1;
    hipLaunchKernelGGL(moe_combine_kernel, dim3(a.T), dim3(256), 0, s, (const float *) a.prod, m.x, m.E, m.n_used, m.out);
    return 0;
}
