// bamd_attention_gs.hip — batched prefill attention on the VALU with its score / probability rows in a global scratch block: what runs beyond the LDS bound
// (two rows of ld floats no longer fit BAMD_ATTN_LDS_MAX: ld > 18432) where the LONG matrix-core kernel (bamd_attention_mfma.hip) does not take the shape.
// A translation unit of its own: the decode step's code objects (bamd_attention.hip, embedded for the own-queue replay) do not change with it.
#include "bamd_device.h"

// attn_batch_kernel's (bamd_attention.hip) arithmetic, operation for operation (q rounded to f16, ggml_vec_dot_f16 order, the reference's softmax with its guard, the tinyBLAS chain per
// SIMD lane over positions 0 .. n_kv), for sequences whose rows no longer fit BAMD_ATTN_LDS_MAX: the fallback of the LONG matrix-core kernel and the only path
// of the head shapes that kernel declines (head_dim 64 / 192 / 256, GQA ratios 3, 5, 6, 7).  One workgroup per (KV head, token) computes ALL GQ query heads of
// the KV head — no ladder: nothing here is sized by the LDS — so every K row and V^T chunk is fetched once for the GQ heads.  Its rows [GQ][ld] sit at workgroup
// index x GQ x ld floats of a.batch_scratch and come back through the CU's vector L1 / the L2 (the same CU wrote them).  Rows are written by one wave and read
// by another of the same workgroup: every phase boundary is a workgroup-scope release, the barrier, a workgroup-scope acquire (wg_sync_global) — the
// workgroup's waves share one CU and its L1, so workgroup scope is the scope that is needed, and no other workgroup ever touches these rows during the launch.
// tok0: first token of this launch's slice of the micro-batch (grid.y = tokens of the slice); positions, q rows and out rows are the micro-batch's.
__device__ __forceinline__ void wg_sync_global() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
template <int GQ>
__global__ void __launch_bounds__(512) attn_batch_gs_kernel(bamd_attn_args a, int tok0) {
    __shared__ __attribute__((aligned(16))) unsigned short q16t[GQ][256];
    __shared__ float redf[GQ][8];
    __shared__ double redd[GQ][8];
    const int ld = a.lds_ld ? a.lds_ld : a.n_ctx;                            // scratch row length: bounds the padded sequence length of the micro-batch
    float * sc = a.batch_scratch + ((size_t) blockIdx.y * gridDim.x + blockIdx.x) * GQ * (size_t) ld;   // [GQ][ld] scores, then exp values, then — IN PLACE —
    float * pt = sc;                                                         // the probabilities in V^T position order (vperm stays inside a 64-block)
    const bamd_step_state * st = a.st;
    const int tokb = tok0 + (int) blockIdx.y;
    const int pos = st->pos + tokb;
    int n_kv = (pos + 1 + 31) / 32 * 32; n_kv = n_kv < st->n_ctx ? n_kv : st->n_ctx;
    const int hd = a.hd, Hkv = a.Hkv, Ekv = Hkv * hd, n_ctx = a.n_ctx, L = hd >> 3;
    const int hk = blockIdx.x, h0 = hk * GQ;
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id(), e = lane & 7;
    const int r_pos = wave * 8 + (lane >> 3);
    const float * q = a.q + (size_t) tokb * a.ld_qkv + (size_t) h0 * hd;
    const float * rope = a.rope + (size_t) pos * hd;
    for (int i = tid; i < GQ * (hd / 2); i += blockDim.x) {                  // RoPE of the GQ query heads -> f16, chain-major (attn_batch_kernel)
        const int hh = i / (hd / 2), p = i - hh * (hd / 2);
        const float c = rope[2 * p], sn = rope[2 * p + 1];
        const float x0 = q[hh * hd + 2 * p], x1 = q[hh * hd + 2 * p + 1];
        const float t0 = x0 * c, t1 = x1 * sn, t2 = x0 * sn, t3 = x1 * c;
        q16t[hh][kperm(2 * p, L)] = f2h(t0 - t1); q16t[hh][kperm(2 * p + 1, L)] = f2h(t2 + t3);
    }
    __syncthreads();
    // ---- scores: K row i once, GQ chains (unconditional requests, the mask is a select: attn_batch_kernel) ----
    for (int t0 = 0; t0 < n_kv; t0 += 64) {
        const int i = t0 + r_pos;
        const bool valid = i < n_kv && i <= pos;
        const unsigned short * krow = a.kc + (size_t) (valid ? i : pos) * Ekv + hk * hd + e * 8;
        uint4 kl[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) kl[g] = g * 8 < L ? *(const uint4 *) (krow + g * BAMD_KGRP) : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int hh = 0; hh < GQ; ++hh) {
            float v = hsum8_vecdot(kq_chain<true>(kl, L, nullptr, &q16t[hh][0] + e * 8));
            v = valid ? v : -INFINITY;                             // masked (KQ_mask, llama.cpp:14152-14200)
            if (e == 0 && i < n_kv) sc[(size_t) hh * ld + i] = v;
        }
    }
    wg_sync_global();
    // ---- softmax per head (ggml.c:13682-13778 + :2619-2671) ----
    const float scale = a.kq_scale;
#pragma unroll
    for (int hh = 0; hh < GQ; ++hh) {
        const float * s_ = sc + (size_t) hh * ld;
        float mx = -INFINITY;
        for (int i = tid; i < n_kv; i += blockDim.x) { const float w = s_[i] * scale; mx = w > mx ? w : mx; }
        uint32_t u = __float_as_uint(mx); u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
        u = wave_max_u32(u);
        if (lane == 0) redf[hh][wave] = __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
    }
    __syncthreads();
#pragma unroll
    for (int hh = 0; hh < GQ; ++hh) {
        float * s_ = sc + (size_t) hh * ld;
        float mx = redf[hh][0];
        for (int w = 1; w < 8; ++w) mx = redf[hh][w] > mx ? redf[hh][w] : mx;
        double sum = 0.0;
        for (int i = tid; i < n_kv; i += blockDim.x) {             // n_kv % 32 == 0: 8-lane groups are all-active or all-idle
            const float w = s_[i] * scale;
            const float val = v_expf(w - mx);
            s_[i] = val;                                           // the element this thread just read
            const float c = hsum8_tinyblas(val);
            if (e == 0) sum += (double) c;
        }
        sum = wave_sum_f64(sum);
        if (lane == 0) redd[hh][wave] = sum;
    }
    wg_sync_global();
#pragma unroll
    for (int hh = 0; hh < GQ; ++hh) {
        const float * s_ = sc + (size_t) hh * ld; float * p_ = pt + (size_t) hh * ld;
        double tot = 0.0;
        for (int w = 0; w < 8; ++w) tot += redd[hh][w];
        double rs = 1.0 / tot;
        float fs = (float) rs;
        if (!f32_rounding_safe(rs, BAMD_F64_GUARD_ULPS(n_kv / 8))) {      // workgroup-uniform, rare: the reference's sequential order (bamd_device.h)
            __syncthreads();
            if (tid == 0) redd[hh][0] = seq_expsum8(s_, n_kv);
            __syncthreads();
            rs = 1.0 / redd[hh][0]; fs = (float) rs;
        }
        // one wave per 64-block: the permuted stores carry the loaded values (a data dependency: every lane's load has returned before any lane of the wave
        // stores), so the block is permuted in place; the idle half of a half-filled last block becomes zeros (exact no-ops in the chains)
        for (int i = tid; i < ((n_kv + 63) & ~63); i += blockDim.x) { const float val = i < n_kv ? s_[i] * fs : 0.f; p_[vperm(i)] = val; }
    }
    wg_sync_global();
    // ---- P.V: V^T chunk once, GQ chains; lane (d, e) carries Cv[e] of output d, up to 4 rows d per lane ----
    float acc[GQ][4];
#pragma unroll
    for (int hh = 0; hh < GQ; ++hh) { acc[hh][0] = 0.f; acc[hh][1] = 0.f; acc[hh][2] = 0.f; acc[hh][3] = 0.f; }
    for (int b0 = 0; b0 < n_kv; b0 += 64) {
#pragma unroll
        for (int dd = 0; dd < 4; ++dd) {
            if (r_pos + 64 * dd < hd) {
                const uint4 vv = *(const uint4 *) (a.vc + (size_t) (hk * hd + r_pos + 64 * dd) * n_ctx + b0 + e * 8);
                const uint32_t w[4] = { vv.x, vv.y, vv.z, vv.w };
                float vf[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) vf[u] = h2f((w[u >> 1] >> (16 * (u & 1))) & 0xffffu);
#pragma unroll
                for (int hh = 0; hh < GQ; ++hh) {
                    const float * p_ = pt + (size_t) hh * ld + b0 + e * 8;
                    const float4 pa = *(const float4 *) p_, pb = *(const float4 *) (p_ + 4);
                    const float pv[8] = { pa.x, pa.y, pa.z, pa.w, pb.x, pb.y, pb.z, pb.w };
                    float c = acc[hh][dd];
#pragma unroll
                    for (int u = 0; u < 8; ++u) c = fmaf(vf[u], pv[u], c);
                    acc[hh][dd] = c;
                }
            }
        }
    }
    float * out = a.out + (size_t) tokb * a.ld_out + (size_t) h0 * hd;
#pragma unroll
    for (int hh = 0; hh < GQ; ++hh) {
#pragma unroll
        for (int dd = 0; dd < 4; ++dd) {
            const int d = r_pos + 64 * dd;
            if (d < hd) { const float v = hsum8_tinyblas(acc[hh][dd]); if (e == 0) out[(size_t) hh * hd + d] = v; }
        }
    }
}

// tokens [t0, t0 + Ts) of the micro-batch (after the KV store); a.batch_scratch holds Hkv x Ts x gq x ld floats (bamd_attention_batch_plan)
void bamd_launch_attention_batch_gs(const bamd_attn_args & a, int gq, int t0, int Ts, hipStream_t s) {
    const dim3 grid(a.Hkv, Ts);
    switch (gq) {
#define CASE(G) case G: BAMD_LAUNCH((attn_batch_gs_kernel<G>), grid, dim3(512), 0, s, a, t0); break;
        CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
#undef CASE
    }
}
