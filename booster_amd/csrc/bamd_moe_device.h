// bamd_moe_device.h — what the two mixture-of-experts translation units share (bamd_moe.hip: one token, the decode step's three launches; bamd_moe_batch.hip:
// a micro-batch): the router's LDS and its one-lane selection, and the bounded read of an expert id.  What is restated: bamd_moe.hip.
#pragma once
#include "bamd_matvec_core.h"
#include "bamd_flt_device.h"

// LDS of the router behind the f32 activation vector [E] and the 16 reduction slots of flt_act: logits | probabilities in sort order | expert ids
#define BAMD_MOE_MAX_EXPERT 64
#define BAMD_MOE_MAX_USED 8
constexpr size_t moe_router_lds(int E) { return (size_t) E * 4 + 16 * sizeof(double) + 3 * BAMD_MOE_MAX_EXPERT * 4; }

__device__ __forceinline__ int moe_expert_of(const int32_t * sel, int slot, int n_expert) {
    int e = __builtin_amdgcn_readfirstlane(ik_ld(sel + slot));
    e = e < 0 ? 0 : e; return e < n_expert ? e : n_expert - 1;      // the router only writes ids below n_expert; an id is an address, so it is bounded here too
}

// softmax over n logits (n % 8 == 0), the first n_used entries of the descending exchange sort, and their normalised weights: ONE lane, in the reference's order
__device__ __forceinline__ void router_select(const float * lg, float * pv, int * idx, int n, int n_used, int32_t * sel, float * w) {
    float mx = -INFINITY;
    for (int i = 0; i < n; ++i) mx = mx > lg[i] ? mx : lg[i];                // ggml_vec_max_f32
    double sum = 0.0;
    for (int i = 0; i < n; i += 8) {                                         // ggml_vec_soft_max_f32, AVX2 branch
        float v[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) { v[t] = v_expf(lg[i + t] - mx); pv[i + t] = v[t]; }
        const float a0 = v[0] + v[4], a1 = v[1] + v[5], a2 = v[2] + v[6], a3 = v[3] + v[7];
        const float b0 = a0 + a2, b1 = a1 + a3;
        sum += (double) (b0 + b1);
    }
    const float sc = (float) (1.0 / sum);                                     // ggml.c:13768-13769: 1.0 / sum in f64, ggml_vec_scale_f32 takes it as f32
    for (int i = 0; i < n; ++i) { pv[i] = pv[i] * sc; idx[i] = i; }
    // ggml.c:15190-15199 with order DESC: for j, for k > j: if (p[idx[j]] < p[idx[k]]) swap(idx[j], idx[k]).  pv[] holds p[idx[]] and is swapped along, entry j stays
    // in registers over its inner loop.  Outer iteration j leaves entry j final and touches no entry below j: the first n_used iterations give the first n_used
    // entries of the whole sort (ggml_top_k is a view of them), ties included
    for (int j = 0; j < n_used; ++j) {
        float cv = pv[j]; int ci = idx[j];
        for (int k = j + 1; k < n; ++k) {
            const float kv = pv[k];
            if (cv < kv) { const int ki = idx[k]; idx[k] = ci; pv[k] = cv; ci = ki; cv = kv; }
        }
        idx[j] = ci; pv[j] = cv;
    }
    double ws = 0.0;                                                          // ggml_sum_rows: ggml_vec_sum_f32 in f64, stored as f32
    for (int s = 0; s < n_used; ++s) ws += (double) pv[s];
    const float wsum = (float) ws;
    for (int s = 0; s < n_used; ++s) { ik_st(sel + s, (int32_t) idx[s]); ik_st(w + s, pv[s] / wsum); }
}
