// bamd_engine_internal.h — what bamd_engine.cpp (the product path) and bamd_ops.cpp (op-level and measurement entry points) share.  Private to the library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

extern thread_local std::string g_err;          // text behind bamd_last_error(), defined in bamd_engine.cpp
inline int fail(const std::string & m) { g_err = m; return 1; }
#define HIPC(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { g_err = std::string(#x) + ": " + hipGetErrorString(e_); return 1; } } while (0)
#define HIPP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { g_err = std::string(#x) + ": " + hipGetErrorString(e_); return nullptr; } } while (0)

#define BAMD_PREFILL_CAP 512            /* tokens of one prompt micro-batch: the reference's default n_batch / n_ubatch */

// owners for the short-lived HIP objects of the measurement entry points (an early error return must not leak them)
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    ~EventPair() { if (a) hipEventDestroy(a); if (b) hipEventDestroy(b); }
    hipError_t create() { hipError_t e = hipEventCreate(&a); return e != hipSuccess ? e : hipEventCreate(&b); }
};
struct OwnedStream { hipStream_t s = nullptr; ~OwnedStream() { if (s) hipStreamDestroy(s); } };
struct OwnedDevMem { void * p = nullptr; ~OwnedDevMem() { if (p) hipFree(p); } };
struct OwnedGraphExec { hipGraphExec_t g = nullptr; ~OwnedGraphExec() { if (g) hipGraphExecDestroy(g); } };

// defined in bamd_engine.cpp: one cos / sin row of the RoPE table on the host; the K-shift's cos / sin table and the row index of every cell (kv_update, bamd_op_k_shift)
void rope_row(float * cache, int32_t pos, int n_dims, float freq_base, float freq_scale, const float * freq_factors,
              float ext_factor, float attn_factor, int n_ctx_orig, float beta_fast, float beta_slow);
void k_shift_table(const int32_t * delta, int n_cells, int n_idx, int hd, float freq_base, float freq_scale, const float * freq_factors,
                   float ext_factor, float attn_factor, int n_ctx_orig, std::vector<int32_t> & idx, std::vector<float> & tab);
// defined in bamd_engine.cpp: one batched prompt mat-mul, each segment routed to the matrix-core kernel (side table aux[i], f16 activations blob16) or to the
// integer-dot kernel — the prompt path's routing, shared with bamd_op_mul_mat_batch_seg.  bf: what BF16 segments on their matrix-core kernel need beside the blob
// (bamd_bf16_range.h): x = [T] the tokens' range words (bamd_launch_quantize_batch), w[i] = the range word of segment i; null: such segments stay on the VALU kernel
struct bamd_mm_args;
struct bamd_bf16_ranges { const uint32_t * x; uint32_t w[3]; };
int bamd_batch_mm(bamd_mm_args a, int epi, const void * blob16, const void * const * aux, int n_cu, hipStream_t s, const bamd_bf16_ranges * bf = nullptr);
