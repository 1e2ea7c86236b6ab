// bamd_attn_batch.h — batched prefill attention on the VALU: one workgroup per (KV head, token) computes G query heads that share the KV head.  The body
// shared by attn_batch_kernel (bamd_attention.hip: score / probability rows in dynamic LDS) and attn_batch_gs_kernel (bamd_attention_gs.hip: rows in a global
// scratch block).  Numerics contract and reference citations: bamd_device.h.
#pragma once
#include "bamd_device.h"

// ROWS: where the [G][ld] score / probability rows of the workgroup live and how a phase boundary that hands rows from one wave to another is crossed.
//   base    the rows
//   sync()  the barrier at such a boundary
// Rows in LDS: the plain barrier.
struct AttnRowsLDS {
    float * base;
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};
// Rows in global memory come back through the CU's vector L1 / the L2 (the same CU wrote them).  They are written by one wave and read by another of the same
// workgroup: every phase boundary is a workgroup-scope release, the barrier, a workgroup-scope acquire — the workgroup's waves share one CU and its L1, so
// workgroup scope is the scope that is needed, and no other workgroup ever touches these rows during the launch.
__device__ __forceinline__ void wg_sync_global() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
struct AttnRowsGlobal {
    float * base;
    __device__ __forceinline__ void sync() const { wg_sync_global(); }
};

// blockDim.x, read as a kernel's own text reads it.  In a __device__ function blockDim.x keeps the runtime's choice between the workgroup size and the size of a
// partial last workgroup (only a kernel carries the uniform-workgroup attribute that folds it), and behind a barrier it came back as a vector load in front of
// the softmax loops: 0.5 - 1.8 % per launch against the kernels with the body written into them
__device__ __forceinline__ unsigned wg_size_x() { return __builtin_amdgcn_workgroup_size_x(); }

// Same arithmetic per (token, head) as attn_fused_kernel in its T > 1 mode (q rounded to f16, ggml_vec_dot_f16 order for the scores, softmax with the
// reference's 8-wide partial sums and its guard, the tinyBLAS chain per SIMD lane over positions 0 .. n_kv for P.V), but every K row and V^T chunk is loaded
// once for the G heads, and the token's own K/V are already in the cache (kv_store_batch_kernel).
// hk: KV head, h0: first of the G query heads (all of KV head hk), tokb: token of the micro-batch — positions, q rows and out rows are the micro-batch's.
// The barriers behind the RoPE and inside the guard's fallback are plain in every instance: q16t and redd are LDS.
template <int G, typename ROWS>
__device__ __forceinline__ void attn_batch_body(const bamd_attn_args & a, int hk, int h0, int tokb, ROWS rows) {
    __shared__ __attribute__((aligned(16))) unsigned short q16t[G][256];
    __shared__ float redf[G][8];
    __shared__ double redd[G][8];
    const int ld = a.lds_ld ? a.lds_ld : a.n_ctx;                            // row length: bounds the padded sequence length of the micro-batch
    float * sc = rows.base;                                                  // [G][ld] scores, then exp values, then — IN PLACE — the
    float * pt = sc;                                                         // probabilities in V^T position order (vperm stays inside a 64-block)
    const bamd_step_state * st = a.st;
    const int pos = st->pos + tokb;
    int n_kv = (pos + 1 + 31) / 32 * 32; n_kv = n_kv < st->n_ctx ? n_kv : st->n_ctx;
    const int hd = a.hd, Hkv = a.Hkv, Ekv = Hkv * hd, n_ctx = a.n_ctx, L = hd >> 3;
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id(), e = lane & 7;
    const int r_pos = wave * 8 + (lane >> 3);
    const float * q = a.q + (size_t) tokb * a.ld_qkv + (size_t) h0 * hd;
    const float * rope = a.rope + (size_t) pos * hd;
    // RoPE of the G query heads -> f16, chain-major (rope_heads arithmetic; only the f16 copy is needed at T > 1)
    for (int i = tid; i < G * (hd / 2); i += wg_size_x()) {
        const int hh = i / (hd / 2), p = i - hh * (hd / 2);
        const float c = rope[2 * p], sn = rope[2 * p + 1];
        const float x0 = q[hh * hd + 2 * p], x1 = q[hh * hd + 2 * p + 1];
        const float t0 = x0 * c, t1 = x1 * sn, t2 = x0 * sn, t3 = x1 * c;
        q16t[hh][kperm(2 * p, L)] = f2h(t0 - t1); q16t[hh][kperm(2 * p + 1, L)] = f2h(t2 + t3);
    }
    __syncthreads();
    // ---- scores: K row i once, G chains ----
    for (int t0 = 0; t0 < n_kv; t0 += 64) {
        const int i = t0 + r_pos;
        const bool valid = i < n_kv && i <= pos;
        // unconditional requests (a masked position reads row `pos`, which this micro-batch stored), every chain runs, the mask is a select:
        // a conditional load is a branch with a full wait at its join
        const unsigned short * krow = a.kc + (size_t) (valid ? i : pos) * Ekv + hk * hd + e * 8;
        uint4 kl[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) kl[g] = g * 8 < L ? *(const uint4 *) (krow + g * BAMD_KGRP) : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int hh = 0; hh < G; ++hh) {
            float v = hsum8_vecdot(kq_chain<true>(kl, L, nullptr, &q16t[hh][0] + e * 8));
            v = valid ? v : -INFINITY;                             // masked (KQ_mask, llama.cpp:14152-14200)
            if (e == 0 && i < n_kv) sc[(size_t) hh * ld + i] = v;
        }
    }
    rows.sync();
    // ---- softmax per head (ggml.c:13682-13778 + :2619-2671) ----
    const float scale = a.kq_scale;
#pragma unroll
    for (int hh = 0; hh < G; ++hh) {
        const float * s_ = sc + (size_t) hh * ld;
        float mx = -INFINITY;
        for (int i = tid; i < n_kv; i += wg_size_x()) { const float w = s_[i] * scale; mx = w > mx ? w : mx; }
        uint32_t u = __float_as_uint(mx); u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
        u = wave_max_u32(u);
        if (lane == 0) redf[hh][wave] = __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
    }
    __syncthreads();
#pragma unroll
    for (int hh = 0; hh < G; ++hh) {
        float * s_ = sc + (size_t) hh * ld;
        float mx = redf[hh][0];
        for (int w = 1; w < 8; ++w) mx = redf[hh][w] > mx ? redf[hh][w] : mx;
        double sum = 0.0;
        for (int i = tid; i < n_kv; i += wg_size_x()) {             // n_kv % 32 == 0: 8-lane groups are all-active or all-idle
            const float w = s_[i] * scale;
            const float val = v_expf(w - mx);
            s_[i] = val;                                           // the element this thread just read
            const float c = hsum8_tinyblas(val);
            if (e == 0) sum += (double) c;
        }
        sum = wave_sum_f64(sum);
        if (lane == 0) redd[hh][wave] = sum;
    }
    rows.sync();
#pragma unroll
    for (int hh = 0; hh < G; ++hh) {
        const float * s_ = sc + (size_t) hh * ld; float * p_ = pt + (size_t) hh * ld;
        double tot = 0.0;
        for (int w = 0; w < 8; ++w) tot += redd[hh][w];
        const float fs = (float) guarded_softmax_rs(tot, n_kv, &redd[hh][0], [=] { return seq_expsum8(s_, n_kv); });
        // one wave per 64-block: the permuted stores carry the loaded values (a data dependency: every lane's load has returned before any lane of the wave
        // stores — in LDS and in global memory alike), so the block is permuted in place; the idle half of a half-filled last block becomes zeros (exact
        // no-ops in the chains)
        for (int i = tid; i < ((n_kv + 63) & ~63); i += wg_size_x()) { const float val = i < n_kv ? s_[i] * fs : 0.f; p_[vperm(i)] = val; }
    }
    rows.sync();
    // ---- P.V: V^T chunk once, G chains; lane (d, e) carries Cv[e] of output d, up to 4 rows d per lane ----
    float acc[G][4];
#pragma unroll
    for (int hh = 0; hh < G; ++hh) { acc[hh][0] = 0.f; acc[hh][1] = 0.f; acc[hh][2] = 0.f; acc[hh][3] = 0.f; }
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
                for (int hh = 0; hh < G; ++hh) {
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
    for (int hh = 0; hh < G; ++hh) {
#pragma unroll
        for (int dd = 0; dd < 4; ++dd) {
            const int d = r_pos + 64 * dd;
            if (d < hd) { const float v = hsum8_tinyblas(acc[hh][dd]); if (e == 0) out[(size_t) hh * hd + d] = v; }
        }
    }
}
