// bamd_attention_mfma_ext.hip — the matrix-core batched-prefill attention (bamd_attention_mfma.hip: its arithmetic contract, its three passes, its LDS map) for the
// shapes that kernel does not take: head_dim 64 at every ratio gq 1 .. 8, and the ratios 3 / 5 / 6 / 7 at head_dim 128.  Behind BAMD_ATTN_MFMA_EXT /
// bamd_set_attn_mfma_ext, default off; the head_dim-128 instances of gq 1 / 2 / 4 / 8 stay in their own file with the code objects they have
// (profiles/attn_mfma_ext_codeobj.txt).
//
// head_dim 64: ggml_vec_dot_f16 over 64 elements is 4 accumulators x 8 SIMD lanes with TWO chain steps each — accumulator (j, e) runs over the elements
//   32 s + 8 j + e, s = 0, 1; in kperm order the row is one 64-group and lane e's eight halves at e * 8 + l are the steps l = 4 s + j, so the operand roles of the
//   128 kernel hold for the k-lanes kq = s in {0, 1}.  v_mfma_f32_16x16x4_f32 is the sequential FOUR-step chain (tools/mfma_f32_probe.hip); the two-step chain is
//   that instruction with BOTH operands of the k-lanes 2 and 3 equal to +0: fma(0, 0, acc) = acc bit for bit (an f32 product of two widened f16 values never
//   underflows and a chain that starts at +0 never holds -0; both operands, not one: 0 x inf would be a NaN).  The spare k-lanes request no K bytes.
//   Geometry: 16 x 32 RoPE pairs (two per thread), q in LDS 2 KB, a tile of 16 K rows is 2 KB — FOUR of them in flight per wave, the bytes of the 128 kernel's two —,
//   the 64 V^T rows are four row tiles, ONE per wave: the named-register V ring and the staged block per wave halve.  LDS at 512 positions: 2 + 9 + 1 + 32 = 44 KB.
//   Four waves and two workgroups per CU as there (BAMD_AM_NW); a third resident workgroup would fit the budget and has not been measured.
// gq 3 / 5 / 6 / 7: a workgroup still has 16 columns, NC = (16 / gq) * gq of them live (15, 15, 12, 14).  A column n >= NC would map to token t0 + 16 / gq — the first
//   token of the NEXT tile, for which this tile's npos is too short, and whose store would race the next workgroup's.  So a dead column takes the inputs of column
//   NC - 1 (q, position), runs every pass like it — the guard's sequential fallback included —, owns its own column of the LDS rows and of the scratch block, and is
//   never stored to `out`.
#include "bamd_attn_mfma.h"

template <int HD, int GQ, bool LONG>
__global__ void __launch_bounds__(64 * BAMD_AM_NW) __attribute__((amdgpu_waves_per_eu(2, 2))) attn_batch_mfma_ext_kernel(bamd_attn_args a, int T, int dbg_exit, int tok0) {
    constexpr int hd = HD, L = hd / 8, HP = hd / 2, TT = 16 / GQ, NC = TT * GQ, NW = BAMD_AM_NW, NT = 64 * NW;
    constexpr int DT = hd / 16 / NW;                                           // 16-row tiles of V^T per wave in the P.V pass: 2 (head_dim 128) or 1 (64)
    constexpr int KS = hd / 32;                                                // chain steps of a score accumulator = live k-lanes of its MFMA: 4 or 2
    constexpr int KD = 256 / hd;                                               // tiles of 16 K rows in flight per wave (pass 1): 4 KB per wave either way
    constexpr int QBYTES = 16 * hd * 2, VBYTES = NW * DT * 16 * BAMD_AM_VROW;
    static_assert((HD == 64 || HD == 128) && GQ >= 1 && GQ <= 8, "head_dim 64 / 128, one to eight query heads per KV head");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned short * q16 = (unsigned short *) smem;                            // [16 columns][hd], chain-major (kperm)
    unsigned char * vst = smem + QBYTES;                                       // [NW waves][DT row tiles][16 rows][BAMD_AM_VROW]
    float * cmaxs = (float *) (smem + QBYTES + VBYTES);                        // [NW waves][16 columns] score maxima; fsv [16]: 1 / sum of every column
    float * fsv = cmaxs + 128;
    float * S = (float *) (smem + QBYTES + VBYTES + BAMD_AM_RBYTES);           // [positions][16]: scores, then exp values (the probabilities are formed in pass 3)
    const int sld = a.lds_ld ? a.lds_ld : a.n_ctx;                              // LONG: floats per column of this workgroup's scratch block
    float * scr = LONG ? a.batch_scratch + (size_t) blockIdx.x * 16 * sld : nullptr;
    const bamd_step_state * st = a.st;
    const int Hkv = a.Hkv, Ekv = Hkv * hd, n_ctx = a.n_ctx;
    const int hk = (int) blockIdx.x % Hkv, tile = (int) blockIdx.x / Hkv;      // consecutive workgroups: different KV heads
    const int t0 = tok0 + tile * TT;                                           // tok0: first token of this launch's slice of the micro-batch (a multiple of TT)
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
    const int P0 = a.batch_pos0p1 > 0 ? a.batch_pos0p1 - 1 : st->pos;
    const int tlast = (t0 + TT - 1 < T ? t0 + TT - 1 : T - 1);
    const int pmax = P0 + tlast;                                               // highest position any LIVE column of this tile attends (dead columns: column NC - 1's)
    int npos = (pmax + 1 + 63) & ~63; npos = npos < n_ctx ? npos : n_ctx;       // positions past a column's own are masked: exact no-ops
    const int mrow = lane & 15, kq = lane >> 4;                                // MFMA operand roles of this lane: A[m = mrow][k = kq], B[k = kq][n = mrow]
    const bool klive = kq < KS;                                                // head_dim 64: the k-lanes 2 and 3 hold +0 in both operands and request nothing
    // the token of column n — dead columns (n >= NC) and tokens past the batch end take a live column's (never stored)
    auto col_tok = [&](int n) { const int nc = (NC < 16 && n >= NC) ? NC - 1 : n; const int tok = t0 + nc / GQ; return tok < T ? tok : T - 1; };
    auto col_head = [&](int n) { const int nc = (NC < 16 && n >= NC) ? NC - 1 : n; return hk * GQ + nc % GQ; };
    // a ring of KD tiles of K rows per wave in flight (64 bytes per live lane and tile: the 8-byte piece of chain steps 4 kq .. 4 kq + 3 of every lane e, kperm
    // order), requested unconditionally (a tile past the end: the last one again) so that the waits stay counted
    const unsigned short * kbase = a.kc + (size_t) hk * hd + (kq >> 1) * BAMD_KGRP + (kq & 1) * 4;
    const int ntile = npos >> 4;
    uint2 ring[KD][8];
#pragma unroll
    for (int d = 0; d < KD; ++d)
#pragma unroll
        for (int e = 0; e < 8; ++e) ring[d][e] = make_uint2(0u, 0u);
    auto kload = [&](uint2 (&dst)[8], int pt) {
        if (klive) {
            const int row = (pt < ntile ? pt : ntile - 1) * 16 + mrow;
            const unsigned short * kp = kbase + (size_t) row * Ekv;
#pragma unroll
            for (int e = 0; e < 8; ++e) dst[e] = *(const uint2 *) (kp + e * 8);
        }
    };
    // ---- RoPE of the 16 query vectors -> f16, chain-major (rope_heads' arithmetic).  16 x hd / 2 pairs: RP per thread, all requested (8-byte loads) before
    //      anything else, the K ring right behind them ----
    constexpr int RP = 16 * HP / NT;
    float2 qx[RP], cs[RP];
#pragma unroll
    for (int it = 0; it < RP; ++it) {
        const int i = tid + it * NT, n = i / HP, p = i % HP;
        const int tok = col_tok(n);
        qx[it] = *(const float2 *) (a.q + (size_t) tok * a.ld_qkv + (size_t) col_head(n) * hd + 2 * p);
        cs[it] = *(const float2 *) (a.rope + (size_t) (P0 + tok) * hd + 2 * p);
    }
#pragma unroll
    for (int d = 0; d < KD; ++d) kload(ring[d], wave + NW * d);
#pragma unroll
    for (int it = 0; it < RP; ++it) {
        const int i = tid + it * NT, n = i / HP, p = i % HP;
        const float x0 = qx[it].x, x1 = qx[it].y, c = cs[it].x, sn = cs[it].y;
        const float u0 = x0 * c, u1 = x1 * sn, u2 = x0 * sn, u3 = x1 * c;
        q16[n * hd + kperm(2 * p, L)] = f2h(u0 - u1); q16[n * hd + kperm(2 * p + 1, L)] = f2h(u2 + u3);
    }
    __syncthreads();
    if (dbg_exit == 1) return;
    // ================= pass 1: scores (and the running maximum of every column) =================
    {
        // B fragments, once: column mrow, elements 32 s + 8 j + e for s = kq — stored at (kq >> 1) * 64 + e * 8 + (kq & 1) * 4 + j (kperm): four consecutive halves per e
        float B[8][4];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            uint2 w = make_uint2(0u, 0u);
            if (klive) w = *(const uint2 *) (q16 + mrow * hd + (kq >> 1) * BAMD_KGRP + e * 8 + (kq & 1) * 4);
            B[e][0] = h2f_lo(w.x); B[e][1] = h2f_hi(w.x); B[e][2] = h2f_lo(w.y); B[e][3] = h2f_hi(w.y);
        }
        const int pcol = P0 + col_tok(mrow);                                   // the position of this lane's column (D layout: column = lane & 15 as well)
        float cmax = -INFINITY;
        for (int pt0 = wave; pt0 < ntile; pt0 += NW * KD) {
#pragma unroll
            for (int d = 0; d < KD; ++d) {
                const int pt = pt0 + NW * d;
                if (pt < ntile) {                                              // wave-uniform; no request inside (short sequences have fewer tiles than ring turns)
                    f32x4_t Se[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const f32x4_t z = { 0.f, 0.f, 0.f, 0.f };
                        const f32x4_t d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(h2f_lo(ring[d][e].x), B[e][0], z, 0, 0, 0);
                        const f32x4_t d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(h2f_hi(ring[d][e].x), B[e][1], z, 0, 0, 0);
                        const f32x4_t d2 = __builtin_amdgcn_mfma_f32_16x16x4f32(h2f_lo(ring[d][e].y), B[e][2], z, 0, 0, 0);
                        const f32x4_t d3 = __builtin_amdgcn_mfma_f32_16x16x4f32(h2f_hi(ring[d][e].y), B[e][3], z, 0, 0, 0);
                        const f32x4_t s02 = d0 + d2, s13 = d1 + d3;             // GGML_F16_VEC_REDUCE: sum[0] += sum[2]; sum[1] += sum[3]; sum[0] += sum[1]
                        Se[e] = s02 + s13;
                    }
                    // the 8-lane horizontal sum of ggml_vec_dot_f16 (hsum8_vecdot): (lo + hi), then two hadd_ps
                    const f32x4_t t0_ = Se[0] + Se[4], t1_ = Se[1] + Se[5], t2_ = Se[2] + Se[6], t3_ = Se[3] + Se[7];
                    const f32x4_t u0 = t0_ + t1_, u2 = t2_ + t3_;
                    const f32x4_t sc = u0 + u2;
                    float vv[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int p = pt * 16 + 4 * kq + r;                    // D layout: register r of lane l = row 4 (l / 16) + r, column l % 16
                        const float v = p <= pcol ? sc[r] : -INFINITY;         // KQ_mask
                        if (!LONG) S[am_sidx(p, mrow)] = v;
                        vv[r] = v;
                        cmax = v > cmax ? v : cmax;
                    }
                    if (LONG) *(float4 *) (scr + am_gidx(pt * 16 + 4 * kq, mrow)) = make_float4(vv[0], vv[1], vv[2], vv[3]);   // four consecutive positions of column mrow
                }
                kload(ring[d], pt + NW * KD);
            }
        }
        // column maxima: across the four k-groups of the wave, then across the waves through LDS
        { const float o = __shfl_xor(cmax, 16); cmax = o > cmax ? o : cmax; }
        { const float o = __shfl_xor(cmax, 32); cmax = o > cmax ? o : cmax; }
        if (lane < 16) cmaxs[wave * 16 + lane] = cmax;
    }
    if (dbg_exit == 2) return;
    // the first blocks of this wave's V^T rows are requested now: they land while the softmax pass runs.  Staging: lane i fetches 16 bytes of row (i >> 3)
    // [+ 8] of each of the wave's DT row tiles, at byte (i & 7) * 16 of the 128-byte block; two blocks in flight in named registers (c, d: the second row tile)
    const int srow = lane >> 3, sby = (lane & 7) * 16;
    const unsigned char * gv = (const unsigned char *) (a.vc + (size_t) (hk * hd + wave * DT * 16 + srow) * n_ctx) + sby;
    const size_t row8 = (size_t) 8 * n_ctx * 2, tile16 = (size_t) 16 * n_ctx * 2;        // bytes between rows r and r + 8, between row tiles
    const int nblk = npos >> 6;
    static_assert(DT == 1 || DT == 2, "the V^T ring is written out for one or two row tiles per wave");
    uint4 v0a, v0b, v0c, v0d, v1a, v1b, v1c, v1d;                              // (named registers: an array ring ends up in scratch memory)
#define BAMD_AX_VLOAD(A_, B_, C_, D_, blk_) do { const int bb_ = ((blk_) < nblk ? (blk_) : nblk - 1) * 128; \
        A_ = *(const uint4 *) (gv + bb_); B_ = *(const uint4 *) (gv + row8 + bb_); \
        if constexpr (DT == 2) { C_ = *(const uint4 *) (gv + tile16 + bb_); D_ = *(const uint4 *) (gv + tile16 + row8 + bb_); } } while (0)
    BAMD_AX_VLOAD(v0a, v0b, v0c, v0d, 0); BAMD_AX_VLOAD(v1a, v1b, v1c, v1d, 1);
    __syncthreads();
    // ================= pass 2: softmax, 16 / NW columns per wave (64 NW / 16 lanes each) — dead columns too: copies of column NC - 1 =================
    {
        constexpr int LPC = 4 * NW;                                            // lanes per column: 16 (a DPP row: two groups of eight positions)
        const int n = (16 / NW) * wave + lane / LPC, pl = lane % LPC, qb = lane - pl;
        const float scale = a.kq_scale;
        float smax = cmaxs[n];
#pragma unroll
        for (int w2 = 1; w2 < NW; ++w2) { const float o = cmaxs[w2 * 16 + n]; smax = o > smax ? o : smax; }
        const float mx = smax * scale;                                         // max_i (s_i * scale): the product is monotonic in s (scale > 0)
        double sum = 0.0;
        float * colv = scr;
        for (int p = pl; p < npos; p += LPC) {                                 // npos % 64 == 0: every 8-lane group is all-active
            const float w = (LONG ? colv[am_gidx(p, n)] : S[am_sidx(p, n)]) * scale;
            const float val = v_expf(w - mx);
            if (LONG) colv[am_gidx(p, n)] = val; else S[am_sidx(p, n)] = val;
            const float c = hsum8_tinyblas(val);                               // the reference's 8-wide partial sum (same tree shape), valid in lane & 7 == 0
            if ((lane & 7) == 0) sum += (double) c;
        }
        // the partial sums of the column's lanes in a fixed order; the reference's order is sequential over the 8-groups: f32_rounding_safe
        // decides whether the order can matter for (float) (1 / sum), and if it can one lane redoes the sum in the reference's order
        double tot = __shfl(sum, qb);
#pragma unroll
        for (int g = 8; g < LPC; g += 8) tot += __shfl(sum, qb + g);
        double rs = 1.0 / tot;
        if (!f32_rounding_safe(rs, BAMD_F64_GUARD_ULPS(npos / 8))) {           // uniform per column; rare
            double sq = 0.0;
            if (LONG) { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); }   // the column's own stores, then one lane's loads
            if (pl == 0) {
                for (int p = 0; p < npos; p += 8) {
                    float x0, x1, x2, x3, x4, x5, x6, x7;
                    if (LONG) { const float4 qa = *(const float4 *) (colv + am_gidx(p, n)), qc = *(const float4 *) (colv + am_gidx(p + 4, n));
                                x0 = qa.x; x1 = qa.y; x2 = qa.z; x3 = qa.w; x4 = qc.x; x5 = qc.y; x6 = qc.z; x7 = qc.w; }
                    else { x0 = S[am_sidx(p, n)]; x1 = S[am_sidx(p + 1, n)]; x2 = S[am_sidx(p + 2, n)]; x3 = S[am_sidx(p + 3, n)];
                           x4 = S[am_sidx(p + 4, n)]; x5 = S[am_sidx(p + 5, n)]; x6 = S[am_sidx(p + 6, n)]; x7 = S[am_sidx(p + 7, n)]; }
                    const float a0 = x0 + x4, a1 = x1 + x5, a2 = x2 + x6, a3 = x3 + x7;
                    const float b0 = a0 + a2, b1 = a1 + a3;
                    sq += (double) (b0 + b1);
                }
            }
            rs = 1.0 / __shfl(sq, qb);
        }
        if (pl == 0) fsv[n] = (float) rs;                                       // the probabilities are formed where they are used: p = e * fs in pass 3
    }
    __syncthreads();
    if (dbg_exit == 3) return;
    // ================= pass 3: P.V — wave w owns the row tiles DT w .. DT w + DT - 1 (16 rows of V^T each), all 16 columns =================
    {
        unsigned char * vs = vst + wave * (DT * 16 * BAMD_AM_VROW);
        const float fs = fsv[mrow];                                            // ggml_vec_scale_f32 by (float) (1 / sum): one multiply per probability
        // where this lane's B operands sit (am_sidx of p = 64 b + 8 (l0 + kq) + e, column mrow): row = 64 b + 32 (l0 / 4) + 4 e + kq and the column
        // swizzle (8 (l0 / 4) + e) & 15 do not depend on b — sixteen lane constants, everything else is an immediate offset of the DS read
        int bcol[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) bcol[c] = kq * 16 + (mrow ^ c);
        f32x4_t acc[DT][8];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[dt][e] = (f32x4_t) { 0.f, 0.f, 0.f, 0.f };
#define BAMD_AX_VSTEP(A_, B_, C_, D_, b_) do { \
            const int b = (b_); \
            if (b < cb1) {                                                     /* wave-uniform; no request inside */ \
                /* (DS operations of one wave execute in order: these stores land behind the previous block's reads) */ \
                *(uint4 *) (vs + srow * BAMD_AM_VROW + sby) = A_; *(uint4 *) (vs + (srow + 8) * BAMD_AM_VROW + sby) = B_; \
                if constexpr (DT == 2) { *(uint4 *) (vs + (16 + srow) * BAMD_AM_VROW + sby) = C_; *(uint4 *) (vs + (16 + srow + 8) * BAMD_AM_VROW + sby) = D_; } \
                const float * Sb = S + (b - cb0) * 64 * 16; \
                const unsigned short * vr0 = (const unsigned short *) (vs + mrow * BAMD_AM_VROW) + kq, * vr1 = (const unsigned short *) (vs + ((DT - 1) * 16 + mrow) * BAMD_AM_VROW) + kq; \
                _Pragma("unroll") for (int l0 = 0; l0 < 8; l0 += 4) { \
                    _Pragma("unroll") for (int e = 0; e < 8; ++e) { \
                        const float bv = Sb[(32 * (l0 / 4) + 4 * e) * 16 + bcol[(8 * (l0 / 4) + e) & 15]] * fs;   /* B[k = kq][n = mrow]: p[64 b + 8 (l0 + kq) + e] of column mrow */ \
                        /* A[m = mrow][k = kq]: V^T[d][64 b + 8 (l0 + kq) + e] sits at 8 e + l0 + kq */ \
                        acc[0][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(__half2float(__ushort_as_half(vr0[8 * e + l0])), bv, acc[0][e], 0, 0, 0); \
                        if constexpr (DT == 2) acc[DT - 1][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(__half2float(__ushort_as_half(vr1[8 * e + l0])), bv, acc[DT - 1][e], 0, 0, 0); \
                    } \
                } \
            } \
            BAMD_AX_VLOAD(A_, B_, C_, D_, b + 2); } while (0)
        for (int cb0 = 0; cb0 < nblk; cb0 += (LONG ? BAMD_AM_CHUNK / 64 : nblk)) {     // !LONG: one turn, everything is in LDS already
            const int cb1 = LONG ? (cb0 + BAMD_AM_CHUNK / 64 < nblk ? cb0 + BAMD_AM_CHUNK / 64 : nblk) : nblk;
            if (LONG) {
                if (cb0) __syncthreads();                                      // every wave is done with the previous chunk
                const int cn = (cb1 - cb0) * 64;                               // positions of this chunk: column tid / 16 walks them 16 at a time, stores them swizzled
                const float * src = scr + (size_t) cb0 * 64 * 16;                   // position quads of the chunk: one 16-byte load per (quad, column)
                for (int i = tid; i < cn * 4; i += NT) {
                    const int quad = i >> 4, n = i & 15;
                    const float4 v = *(const float4 *) (src + (size_t) i * 4);
                    S[am_sidx(4 * quad, n)] = v.x; S[am_sidx(4 * quad + 1, n)] = v.y; S[am_sidx(4 * quad + 2, n)] = v.z; S[am_sidx(4 * quad + 3, n)] = v.w;
                }
                __syncthreads();
            }
            for (int b0 = cb0; b0 < cb1; b0 += 2) { BAMD_AX_VSTEP(v0a, v0b, v0c, v0d, b0); BAMD_AX_VSTEP(v1a, v1b, v1c, v1d, b0 + 1); }     // (chunks hold an even number of blocks, except possibly the last)
        }
#undef BAMD_AX_VSTEP
#undef BAMD_AX_VLOAD
        const int tok = t0 + mrow / GQ;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            // hsum8_tinyblas across the eight e-tiles, element-wise: (a_e + a_{e+4}), then + the tile two over, then + the tile one over
            const f32x4_t t0_ = acc[dt][0] + acc[dt][4], t1_ = acc[dt][1] + acc[dt][5], t2_ = acc[dt][2] + acc[dt][6], t3_ = acc[dt][3] + acc[dt][7];
            const f32x4_t u0 = t0_ + t2_, u1 = t1_ + t3_;
            const f32x4_t o = u0 + u1;
            if (mrow < NC && tok < T) {                                        // a dead column (tok = the next tile's first token) is never stored
                float * out = a.out + (size_t) tok * a.ld_out + (size_t) (hk * GQ + mrow % GQ) * hd + (wave * DT + dt) * 16 + 4 * kq;      // rows d = 16 (DT w + dt) + 4 kq + r
                *(float4 *) out = make_float4(o[0], o[1], o[2], o[3]);
            }
        }
    }
}

// the instances bamd_attention_mfma.hip does not hold (checked by its launcher: hd 64 / 128, gq 1 .. 8, the switch on); lng: more than BAMD_AM_MAXPOS positions
int bamd_launch_attention_batch_mfma_ext(const bamd_attn_args & a, int gq, int T, hipStream_t s, int t0, int Ts, bool lng, int dbg) {
    const int npos = a.lds_ld ? a.lds_ld : a.n_ctx, tt = 16 / gq;
    const size_t lds = (size_t) 16 * a.hd * 2 + (size_t) (a.hd / 16) * 16 * BAMD_AM_VROW + BAMD_AM_RBYTES + (size_t) (lng ? BAMD_AM_CHUNK : npos) * 64;
    const dim3 grid(a.Hkv * ((Ts + tt - 1) / tt)), block(64 * BAMD_AM_NW);
#define BAMD_AX_GO(HD_, GQ_) do { if (lng) hipLaunchKernelGGL((attn_batch_mfma_ext_kernel<HD_, GQ_, true>), grid, block, lds, s, a, T, dbg, t0); \
                                  else     hipLaunchKernelGGL((attn_batch_mfma_ext_kernel<HD_, GQ_, false>), grid, block, lds, s, a, T, dbg, t0); return 0; } while (0)
    if (a.hd == 64) switch (gq) {
        case 1: BAMD_AX_GO(64, 1); case 2: BAMD_AX_GO(64, 2); case 3: BAMD_AX_GO(64, 3); case 4: BAMD_AX_GO(64, 4);
        case 5: BAMD_AX_GO(64, 5); case 6: BAMD_AX_GO(64, 6); case 7: BAMD_AX_GO(64, 7); case 8: BAMD_AX_GO(64, 8);
    }
    if (a.hd == 128) switch (gq) {
        case 3: BAMD_AX_GO(128, 3); case 5: BAMD_AX_GO(128, 5); case 6: BAMD_AX_GO(128, 6); case 7: BAMD_AX_GO(128, 7);
    }
#undef BAMD_AX_GO
    return 1;
}
