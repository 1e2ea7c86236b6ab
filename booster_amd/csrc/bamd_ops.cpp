// bamd_ops.cpp — op-level entry points (host in / host out) and the mat-vec micro-benchmark of libbooster_amd.so: thin wrappers that run the SAME kernels as the
// model runtime (bamd_engine.cpp) on device 0.  They are what the tests and tools call; nothing here touches bamd_model / bamd_context.
#include "../../include/bamd.h"
#include "bamd_aql.h"
#include "bamd_engine_internal.h"
#include "bamd_formats.h"
#include "bamd_kernels.h"
#include "bamd_prefill_family.h"

#include <math.h>
#include <string.h>
#include <algorithm>

struct Tmp {
    std::vector<void *> p;
    ~Tmp() { for (void * x : p) hipFree(x); }
    void * up(const void * h, size_t n) { void * d = nullptr; if (hipMalloc(&d, n + 4096) != hipSuccess) return nullptr; p.push_back(d); if (h && hipMemcpy(d, h, n, hipMemcpyHostToDevice) != hipSuccess) return nullptr; return d; }
};
static int need_device() {
    if (bamd_device_count() <= 0) return fail("no HIP device available: libbooster_amd has no CPU fallback");
    HIPC(hipSetDevice(0));
    return 0;
}
// the launches went through and ran: `bytes` of their result at `src` to the host
static int finish(void * dst, const void * src, size_t bytes) {
    HIPC(hipGetLastError());
    HIPC(hipDeviceSynchronize());
    HIPC(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return 0;
}
static int n_cu0() { hipDeviceProp_t p; if (hipGetDeviceProperties(&p, 0) != hipSuccess) return 256; return p.multiProcessorCount > 0 ? p.multiProcessorCount : 256; }

extern "C" __attribute__((visibility("default"))) int bamd_op_quantize_q8_K(const float * x, int64_t k, const float * norm_w, float eps, void * out_blocks) {
    if (need_device()) return 1;
    if (k <= 0 || k % 256) return fail("k must be a positive multiple of 256");
    Tmp t; const size_t ob = (size_t) (k / 256) * 292;
    float * dx = (float *) t.up(x, (size_t) k * 4); float * dw = norm_w ? (float *) t.up(norm_w, (size_t) k * 4) : nullptr; void * dout = t.up(nullptr, ob);
    if (!dx || !dout || (norm_w && !dw)) return fail("device alloc/copy failed");
    HIPC(hipMemset(dout, 0, ob));
    bamd_launch_quantize_q8k_test(dx, dw, eps, (int) k, norm_w != nullptr, dout, nullptr);
    return finish(out_blocks, dout, ob);
}

extern "C" __attribute__((visibility("default"))) int bamd_op_quantize_q8_0(const float * x, int64_t k, const float * norm_w, float eps, void * out_blocks) {
    if (need_device()) return 1;
    if (k <= 0 || k % 256) return fail("k must be a positive multiple of 256");
    Tmp t; const size_t ob = (size_t) (k / 32) * 34;
    float * dx = (float *) t.up(x, (size_t) k * 4); float * dw = norm_w ? (float *) t.up(norm_w, (size_t) k * 4) : nullptr; void * dout = t.up(nullptr, ob);
    if (!dx || !dout || (norm_w && !dw)) return fail("device alloc/copy failed");
    HIPC(hipMemset(dout, 0, ob));
    bamd_launch_quantize_q80_test(dx, dw, eps, (int) k, norm_w != nullptr, dout, nullptr);
    return finish(out_blocks, dout, ob);
}

extern "C" __attribute__((visibility("default"))) int bamd_op_quantize_q8_1(const float * x, int64_t k, const float * norm_w, float eps, void * out_blocks) {
    if (need_device()) return 1;
    if (k <= 0 || k % 256) return fail("k must be a positive multiple of 256");
    Tmp t; const size_t ob = (size_t) (k / 32) * 36;
    float * dx = (float *) t.up(x, (size_t) k * 4); float * dw = norm_w ? (float *) t.up(norm_w, (size_t) k * 4) : nullptr; void * dout = t.up(nullptr, ob);
    if (!dx || !dout || (norm_w && !dw)) return fail("device alloc/copy failed");
    HIPC(hipMemset(dout, 0, ob));
    bamd_launch_quantize_q81_test(dx, dw, eps, (int) k, norm_w != nullptr, dout, nullptr);
    return finish(out_blocks, dout, ob);
}

// the activation form of BF16 weights, in the order of the vector: k values of ggml_fp32_to_bf16_row (the sibling of bamd_op_quantize_q8_0)
extern "C" __attribute__((visibility("default"))) int bamd_op_act_bf16(const float * x, int64_t k, const float * norm_w, float eps, uint16_t * out_u16) {
    if (need_device()) return 1;
    if (k <= 0 || k % 256 || k > bamd_flt_max_k(BAMD_BF16)) return fail("k must be a positive multiple of 256 (at most 65536)");
    Tmp t; const size_t ob = (size_t) k * 2;
    float * dx = (float *) t.up(x, (size_t) k * 4); float * dw = norm_w ? (float *) t.up(norm_w, (size_t) k * 4) : nullptr; void * dout = t.up(nullptr, ob);
    if (!dx || !dout || (norm_w && !dw)) return fail("device alloc/copy failed");
    HIPC(hipMemset(dout, 0, ob));
    bamd_launch_act_bf16_test(dx, dw, eps, (int) k, norm_w != nullptr, dout, nullptr);
    return finish(out_u16, dout, ob);
}

static int op_matvec(int type, const void * wA, const void * wB, int nrows, int k, const float * x, const float * norm_w, float eps,
                     const float * residual, float * y, int epi, int mode, unsigned long long * best_key = nullptr) {
    if (need_device()) return 1;
    if (!bamd_has_record(type) || k <= 0 || k % 256 || nrows <= 0) return fail("bad type/shape");
    if (bamd_is_q1(type) && (mode & 15) == 2) return fail("mat-vec: Q4_1 / Q5_1 have no split-K kernel (mode 2): one wave per row-group only");
    if (type == BAMD_IQ4_NL && (mode & 15) == 2) return fail("mat-vec: IQ4_NL has no split-K kernel (mode 2): one wave per row-group only");
    if (bamd_is_flt(type) && k > bamd_flt_max_k(type)) return fail("mat-vec: row length beyond what the F32 / F16 / BF16 kernels hold in LDS");
    const int nrows_pad = (nrows + 7) / 8 * 8;
    Tmp t; const size_t wb = bamd_row_bytes(type, k) * (size_t) nrows, wbp = bamd_stream_bytes(type, k, nrows_pad);
    void * rawA = t.up(wA, wb), * strA = t.up(nullptr, wbp), * rawB = nullptr, * strB = nullptr;
    if (wB) { rawB = t.up(wB, wb); strB = t.up(nullptr, wbp); }
    if (strA) HIPC(hipMemset(strA, 0, wbp));
    if (strB) HIPC(hipMemset(strB, 0, wbp));
    float * dx = (float *) t.up(x, (size_t) k * 4); float * dw = norm_w ? (float *) t.up(norm_w, (size_t) k * 4) : nullptr;
    float * dres = residual ? (float *) t.up(residual, (size_t) nrows * 4) : nullptr; float * dy = (float *) t.up(nullptr, (size_t) nrows * 4);
    unsigned long long * key = (unsigned long long *) t.up(nullptr, 8);
    if (!rawA || !strA || !dx || !dy || !key || (wB && (!rawB || !strB)) || (norm_w && !dw) || (residual && !dres)) return fail("device alloc/copy failed");
    HIPC(hipMemset(key, 0, 8));
    bamd_launch_repack(rawA, strA, type, nrows, k, nullptr);
    if (wB) bamd_launch_repack(rawB, strB, type, nrows, k, nullptr);
    bamd_mv_args a; memset(&a, 0, sizeof a);
    a.seg[0].w = strA; a.seg[0].out = dy; a.seg[0].type = type; a.seg[0].nrows = nrows_pad; a.seg[0].nvalid = nrows; a.nseg = 1;
    if (wB) { a.seg[1] = a.seg[0]; a.seg[1].w = strB; a.nseg = 2; }
    a.x = dx; a.normw = dw; a.eps = eps; a.K = k; a.res = dres; a.best_key = key; a.mode = mode;
    if (bamd_launch_mv(a, norm_w ? BAMD_PRO_NORM : BAMD_PRO_PLAIN, epi, n_cu0(), nullptr)) return fail("mat-vec: type without a kernel");
    if (finish(y, dy, (size_t) nrows * 4)) return 1;
    if (best_key) HIPC(hipMemcpy(best_key, key, 8, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" __attribute__((visibility("default"))) int bamd_op_mul_mat_vec(int type, const void * w_raw, int nrows, int k, const float * x, const float * norm_w, float eps,
                                   const float * residual, float * y, int mode) {
    return op_matvec(type, w_raw, nullptr, nrows, k, x, norm_w, eps, residual, y, residual ? BAMD_EPI_ADD : BAMD_EPI_STORE, mode);
}
// the lm_head launch (enqueue_lm_head) with its arg-max epilogue; the row is decoded from the key as step_begin_kernel decodes it
extern "C" __attribute__((visibility("default"))) int bamd_op_mul_mat_vec_argmax(int type, const void * w_raw, int nrows, int k, const float * x, const float * norm_w,
                                                                                 float eps, float * y, int mode, int32_t * row) {
    unsigned long long key = 0ull;
    if (op_matvec(type, w_raw, nullptr, nrows, k, x, norm_w, eps, nullptr, y, BAMD_EPI_ARGMAX, mode, &key)) return 1;
    *row = key ? (int32_t) (0xffffffffu - (uint32_t) (key & 0xffffffffull)) : -1;
    return 0;
}
// batched mat-mul of T activation rows against one matrix through the prefill kernels: impl 0 = integer-dot kernel, 2 = matrix-core kernel (1 and 3 were the generations removed in round 6)
// (F32 / F16 / BF16: impl 0 = the VALU kernel; impl 2 = the f32 matrix-core kernel, for F32 / F16 only while BAMD_PREFILL_FLT is on, for BF16 only while
// BAMD_PREFILL_BF16 is on)
extern "C" __attribute__((visibility("default"))) int bamd_op_mul_mat_batch(int type, const void * w_raw, int nrows, int k, const float * x, int T, const float * norm_w,
                                                                              float eps, const float * residual, float * y, int impl) {
    if (need_device()) return 1;
    if (!bamd_has_record(type) || k <= 0 || k % 256 || nrows <= 0 || T <= 0) return fail("bad type/shape");
    const int nrows_pad = (nrows + 7) / 8 * 8;
    Tmp t; const size_t wb = bamd_row_bytes(type, k) * (size_t) nrows, wbp = bamd_stream_bytes(type, k, nrows_pad);
    void * raw = t.up(w_raw, wb), * str = t.up(nullptr, wbp);
    float * dx = (float *) t.up(x, (size_t) T * k * 4); float * dw = norm_w ? (float *) t.up(norm_w, (size_t) k * 4) : nullptr;
    float * dres = residual ? (float *) t.up(residual, (size_t) T * nrows * 4) : nullptr; float * dy = (float *) t.up(nullptr, (size_t) T * nrows * 4);
    void * blob = t.up(nullptr, (size_t) T * bamd_act_blob_bytes(bamd_act_form_of(type), k)), * blob16 = t.up(nullptr, (size_t) T * bamd_blob16_bytes(k));
    if (!raw || !str || !dx || !dy || !blob || !blob16 || (norm_w && !dw) || (residual && !dres)) return fail("device alloc/copy failed");
    HIPC(hipMemset(str, 0, wbp));
    bamd_launch_repack(raw, str, type, nrows, k, nullptr);
    const bool flt_mfma = impl == 2 && bamd_prefill_mfma_type_notable(type);      // F32 / F16 with BAMD_PREFILL_FLT on: bamd_prefill2_flt.hip, no side table; BF16 with BAMD_PREFILL_BF16 on: bamd_prefill2_bf16.hip
    uint32_t * xr = flt_mfma && type == BAMD_BF16 ? (uint32_t *) t.up(nullptr, (size_t) T * 4) : nullptr;      // the tokens' range words, beside the blob
    if (flt_mfma && type == BAMD_BF16 && !xr) return fail("device alloc failed");
    bamd_launch_quantize_batch(dx, dw, eps, k, T, blob, blob16, nullptr, bamd_act_form_of(type), xr);
    if (bamd_is_flt(type) && impl != 0 && !flt_mfma) return fail(impl == 2 ? "MFMA path: unsupported type/shape (F32 / F16 / BF16 have no matrix-core kernel)" : "batched mat-mul: impl must be 0 for F32 / F16 / BF16");
    if (flt_mfma && type == BAMD_BF16) {
        uint32_t wr = BAMD_BF16_RANGE_UNKNOWN;                             // measured where the stream is packed, as the loader does
        if (bamd_bf16_weight_range(str, wbp, &wr, nullptr)) return fail("measuring the exponent range failed");
        if (bamd_launch_matmul_mfma_bf16(str, wr, nrows, nrows_pad, k, blob, xr, T, dy, dres, dres ? BAMD_EPI_ADD : BAMD_EPI_STORE, nrows, nullptr)) return fail("MFMA path: unsupported type/shape");
    } else if (flt_mfma) {
        if (bamd_launch_matmul_mfma_flt(str, type, nrows, nrows_pad, k, blob, T, dy, dres, dres ? BAMD_EPI_ADD : BAMD_EPI_STORE, nrows, nullptr)) return fail("MFMA path: unsupported type/shape");
    } else if (impl == 2) {                                             // the matrix-core kernel: side table built here, as the engine builds it at model load
        if (!bamd_prefill_aux_bytes(type, nrows_pad, k)) return fail("MFMA path: unsupported type/shape");      // Q2_K / Q3_K with the switch off (bamd_prefill_mfma_type), IQ4_XS always: the integer-dot kernel only
        void * aux = t.up(nullptr, bamd_prefill_aux_bytes(type, nrows_pad, k));
        if (!aux) return fail("device alloc failed");
        bamd_launch_prefill_aux(str, type, nrows_pad, k, aux, nullptr);
        if (bamd_launch_matmul_mfma2(str, aux, type, nrows, nrows_pad, k, blob16, T, dy, dres, dres ? BAMD_EPI_ADD : BAMD_EPI_STORE, nrows, nullptr)) return fail("MFMA path: unsupported type/shape");
    } else {
        bamd_mm_args a; memset(&a, 0, sizeof a);
        a.seg[0].w = str; a.seg[0].out = dy; a.seg[0].type = type; a.seg[0].nrows = nrows_pad; a.seg[0].nvalid = nrows; a.nseg = 1;
        a.blob = (const uint8_t *) blob; a.K = k; a.T = T; a.ldo = nrows; a.res = dres;
        if (bamd_launch_matmul_batch(a, residual ? BAMD_EPI_ADD : BAMD_EPI_STORE, n_cu0(), nullptr)) return fail("batched mat-mul: unsupported shape");
    }
    return finish(y, dy, (size_t) T * nrows * 4);
}
extern "C" __attribute__((visibility("default"))) int bamd_op_ffn_gate_up(int type, const void * wg_raw, const void * wu_raw, int nrows, int k, const float * x, const float * norm_w,
                                   float eps, float * y) {
    return op_matvec(type, wg_raw, wu_raw, nrows, k, x, norm_w, eps, nullptr, y, BAMD_EPI_SILU_MUL, 0);
}
extern "C" __attribute__((visibility("default"))) int bamd_op_get_row(int type, const void * w_raw, int nrows, int k, int row, float * y) {
    if (need_device()) return 1;
    if (type != BAMD_F32 && type != BAMD_F16 && !bamd_has_record(type)) return fail("bad type");
    if (k <= 0 || (bamd_has_record(type) && type != BAMD_F32 && type != BAMD_F16 && k % 256)) return fail("bad row length");
    if (row < 0 || row >= nrows) return fail("row out of range");
    Tmp t; const size_t wb = bamd_row_bytes(type, k) * (size_t) nrows;
    void * raw = t.up(w_raw, wb); float * dy = (float *) t.up(nullptr, (size_t) k * 4);
    bamd_step_state h; memset(&h, 0, sizeof h); h.n_ctx = 32;
    bamd_step_state * st = (bamd_step_state *) t.up(&h, sizeof h);
    int32_t * forced = (int32_t *) t.up(&row, 4); int32_t * outt = (int32_t *) t.up(nullptr, 64);
    if (!raw || !dy || !st || !forced || !outt) return fail("device alloc/copy failed");
    bamd_launch_step_begin(st, forced, 1, outt, raw, type, k, nrows, dy, 1, nullptr);
    return finish(y, dy, (size_t) k * 4);
}
extern "C" __attribute__((visibility("default"))) int bamd_op_rope_row(int pos, int n_dims, float freq_base, float freq_scale, const float * freq_factors, float * row) {
    rope_row(row, pos, n_dims, freq_base, freq_scale, freq_factors, 0.0f, 1.0f, 8192, 32.0f, 1.0f);
    return 0;
}

// reference layout <-> chain-major device layout of the KV cache (bamd_device.h, "Attention": kperm / vperm)
static inline int kperm_host(int n) { const int l = n >> 3; return ((l >> 3) << 6) + ((n & 7) << 3) + (l & 7); }
static inline int vperm_host(int p) { return (p & ~63) + ((p & 7) << 3) + ((p & 63) >> 3); }

// What the attention ops (and, for its K half, the K-shift op) share: the temporaries of one call with ONE record of whether every upload worked, the KV cache
// of one layer carried to the device in chain-major order and back, and the bamd_attn_args fields that every path sets the same way
struct AttnFixture {
    Tmp t; bool good = true;
    const int n_ctx, Hkv, hd, n_ctx_pad; const size_t kvb;
    std::vector<uint16_t> kd, vd;
    unsigned short * kc = nullptr, * vc = nullptr;
    AttnFixture(int n_ctx_, int Hkv_, int hd_) : n_ctx(n_ctx_), Hkv(Hkv_), hd(hd_), n_ctx_pad((n_ctx_ + 63) / 64 * 64), kvb((size_t) n_ctx_pad * Hkv_ * hd_ * 2) {}
    void * up(const void * h, size_t n) { void * d = t.up(h, n); if (!d) good = false; return d; }
    bool ok() const { return good; }
    // reference order -> device order (to_device) or back; v_ref null: the K cache only
    void reorder(bool to_device, uint16_t * k_ref, uint16_t * v_ref) {
        const int Ekv = Hkv * hd;
        for (int i = 0; i < n_ctx; ++i) for (int h = 0; h < Hkv; ++h) for (int n = 0; n < hd; ++n) {
            uint16_t & r = k_ref[(size_t) i * Ekv + h * hd + n], & d = kd[(size_t) i * Ekv + h * hd + kperm_host(n)];
            if (to_device) d = r; else r = d;
        }
        if (v_ref) for (int r = 0; r < Ekv; ++r) for (int p = 0; p < n_ctx; ++p) {
            uint16_t & x = v_ref[(size_t) r * n_ctx + p], & d = vd[(size_t) r * n_ctx_pad + vperm_host(p)];
            if (to_device) d = x; else x = d;
        }
    }
    void kv_up(uint16_t * k_ref, uint16_t * v_ref) {
        kd.assign((size_t) n_ctx_pad * Hkv * hd, 0); vd.assign(v_ref ? (size_t) n_ctx_pad * Hkv * hd : 0, 0);
        reorder(true, k_ref, v_ref);
        kc = (unsigned short *) up(kd.data(), kvb);
        if (v_ref) vc = (unsigned short *) up(vd.data(), kvb);
    }
    int kv_down(uint16_t * k_ref, uint16_t * v_ref) {
        HIPC(hipMemcpy(kd.data(), kc, kvb, hipMemcpyDeviceToHost));
        if (v_ref) HIPC(hipMemcpy(vd.data(), vc, kvb, hipMemcpyDeviceToHost));
        reorder(false, k_ref, v_ref);
        return 0;
    }
    void args(bamd_attn_args & a, int prefill_mode) const { a.kc = kc; a.vc = vc; a.hd = hd; a.Hkv = Hkv; a.n_ctx = n_ctx_pad; a.kq_scale = 1.0f / sqrtf((float) hd); a.prefill_mode = prefill_mode; }
    void rows(bamd_attn_args & a, int H) { a.scores = (float *) up(nullptr, (size_t) H * n_ctx_pad * 4); a.probs = (float *) up(nullptr, (size_t) H * n_ctx_pad * 4); a.out = (float *) up(nullptr, (size_t) H * hd * 4); }   // single-token paths
    int down(const bamd_attn_args & a, float * out, size_t out_floats, uint16_t * k_ref, uint16_t * v_ref) { return finish(out, a.out, out_floats * 4) || kv_down(k_ref, v_ref); }   // after the launch
    // the first n probabilities of query head 0 (stored in V^T position order)
    int probs_down(const bamd_attn_args & a, int n, float * probs_h0) {
        std::vector<float> pp((size_t) n_ctx_pad);
        HIPC(hipMemcpy(pp.data(), a.probs, (size_t) n_ctx_pad * 4, hipMemcpyDeviceToHost));
        for (int p = 0; p < n; ++p) probs_h0[p] = pp[(size_t) vperm_host(p)];
        return 0;
    }
};

extern "C" __attribute__((visibility("default"))) int bamd_op_attention(const float * q, const float * k, const float * v, uint16_t * k_cache, uint16_t * v_cache_t,
                                 const float * rope_row_h, int H, int Hkv, int hd, int n_ctx, int pos, int prefill_mode, float * out,
                                 float * probs_h0) {
    const bool split_path = (prefill_mode & 2) != 0;   // bit 1: force the three-kernel (long-context) path
    prefill_mode &= 1;
    if (need_device()) return 1;
    if (H <= 0 || Hkv <= 0 || hd <= 0 || hd % 64 || hd > 256 || n_ctx <= 0 || pos < 0 || pos >= n_ctx || n_ctx % 32 || H % Hkv) return fail("bad attention shape");
    AttnFixture f(n_ctx, Hkv, hd); const int Ekv = Hkv * hd;
    std::vector<float> rope((size_t) n_ctx * hd, 0.f);
    memcpy(rope.data() + (size_t) pos * hd, rope_row_h, (size_t) hd * 4);
    bamd_step_state h; memset(&h, 0, sizeof h); h.pos = pos; h.n_ctx = n_ctx; h.n_kv = std::min(n_ctx, std::max(32, (pos + 1 + 31) / 32 * 32));
    bamd_attn_args a; memset(&a, 0, sizeof a);
    a.st = (bamd_step_state *) f.up(&h, sizeof h);
    a.q = (float *) f.up(q, (size_t) H * hd * 4); a.k = (float *) f.up(k, (size_t) Ekv * 4); a.v = (float *) f.up(v, (size_t) Ekv * 4);
    f.kv_up(k_cache, v_cache_t);
    a.rope = (float *) f.up(rope.data(), rope.size() * 4); if (a.rope) a.rope_cur = a.rope + (size_t) pos * hd;
    f.rows(a, H);
    if (!f.ok()) return fail("device alloc/copy failed");
    f.args(a, prefill_mode);
    { const int tiles = std::min(std::max(n_ctx / 64, 1), 64);
      if (bamd_launch_attention(a, H / Hkv, split_path ? -tiles : tiles, nullptr)) return fail("unsupported head configuration"); }
    if (f.down(a, out, (size_t) H * hd, k_cache, v_cache_t)) return 1;
    return probs_h0 && split_path ? f.probs_down(a, h.n_kv, probs_h0) : 0;
}

// the K-shift of one layer as kv_update runs it: the delta -> (cos, sin) table from k_shift_table, then bamd_launch_k_shift over the chain-major cache
extern "C" __attribute__((visibility("default"))) int bamd_op_k_shift(uint16_t * k_cache, int n_ctx, int Hkv, int hd, const int32_t * delta, float freq_base,
                                                                        float freq_scale, const float * freq_factors, float ext_factor, float attn_factor, int n_ctx_orig) {
    if (need_device()) return 1;
    if (Hkv <= 0 || hd <= 0 || hd % 64 || hd > 256 || n_ctx <= 0) return fail("bad K-shift shape");
    AttnFixture f(n_ctx, Hkv, hd);
    std::vector<int32_t> idx;
    std::vector<float> tab;
    k_shift_table(delta, n_ctx, f.n_ctx_pad, hd, freq_base, freq_scale, freq_factors, ext_factor, attn_factor, n_ctx_orig, idx, tab);
    f.kv_up(k_cache, nullptr);
    int32_t * didx = (int32_t *) f.up(idx.data(), idx.size() * 4); float * dtab = (float *) f.up(tab.data(), tab.size() * 4);
    if (!f.ok()) return fail("device alloc/copy failed");
    bamd_launch_k_shift(f.kc, n_ctx, Hkv, hd, didx, dtab, nullptr);
    HIPC(hipGetLastError());
    HIPC(hipDeviceSynchronize());
    return f.kv_down(k_cache, nullptr);
}

// the single-token attention after position edits, as bamd_stage_step sets it up when the cells are tracked: step_begin_kernel derives st->cell / st->n_kv
// from cell_plus1 / n_kv_fixed and leaves the position's (cos, sin) row at rope_cur, the token's cellpos entry is written by a host copy behind the
// upload of the others, and the shifted-cell instances of the three-launch path run with `tiles` score workgroups per KV head (0: the engine's count)
extern "C" __attribute__((visibility("default"))) int bamd_op_attention_cells(const float * q, const float * k, const float * v, uint16_t * k_cache, uint16_t * v_cache_t,
                                                                                const float * rope_row_h, const int32_t * cellpos, int cell, int n_kv, int H, int Hkv, int hd,
                                                                                int n_ctx, int pos, int tiles, float * out, float * probs_h0) {
    if (need_device()) return 1;
    if (H <= 0 || Hkv <= 0 || hd <= 0 || hd % 64 || hd > 256 || n_ctx <= 0 || n_ctx % 32 || H % Hkv || H / Hkv > 8) return fail("bad attention shape");
    if (pos < 0 || pos >= n_ctx || n_kv < 1 || n_kv > n_ctx || cell < 0 || cell >= n_kv || tiles < 0) return fail("bad cell / position / n_kv / tiles");
    AttnFixture f(n_ctx, Hkv, hd); const int Ekv = Hkv * hd;
    std::vector<float> rope((size_t) n_ctx * hd, 0.f);
    memcpy(rope.data() + (size_t) pos * hd, rope_row_h, (size_t) hd * 4);
    std::vector<int32_t> cp((size_t) f.n_ctx_pad, -1);                     // as kv_activate uploads cells.pos
    memcpy(cp.data(), cellpos, (size_t) n_ctx * 4);
    bamd_step_state h; memset(&h, 0, sizeof h);                             // as bamd_stage_step sets it for a tracked cell
    h.pos_base = pos; h.n_ctx = n_ctx; h.cell_plus1 = cell + 1; h.n_kv_fixed = n_kv;
    const float embd[256] = {0.0f}; const int32_t tok0 = 0;
    bamd_attn_args a; memset(&a, 0, sizeof a);
    bamd_step_state * st = (bamd_step_state *) f.up(&h, sizeof h); a.st = st;
    int32_t * dcp = (int32_t *) f.up(cp.data(), cp.size() * 4); a.cellpos = dcp;
    const int32_t * forced = (const int32_t *) f.up(&tok0, 4); int32_t * outt = (int32_t *) f.up(nullptr, 64);
    const void * dembd = f.up(embd, sizeof embd); float * dx = (float *) f.up(nullptr, sizeof embd);
    a.q = (float *) f.up(q, (size_t) H * hd * 4); a.k = (float *) f.up(k, (size_t) Ekv * 4); a.v = (float *) f.up(v, (size_t) Ekv * 4);
    f.kv_up(k_cache, v_cache_t);
    a.rope = (float *) f.up(rope.data(), rope.size() * 4); float * rope_cur = (float *) f.up(nullptr, (size_t) hd * 4); a.rope_cur = rope_cur;
    f.rows(a, H);
    if (!f.ok()) return fail("device alloc/copy failed");
    HIPC(hipMemcpy(dcp + cell, &pos, 4, hipMemcpyHostToDevice));            // bamd_stage_step: cellpos[cell] = cells.pos[cell] (find_slot stored pos there)
    bamd_launch_step_begin(st, forced, 1, outt, dembd, BAMD_F32, 256, 1, dx, 1, nullptr, nullptr, nullptr, a.rope, rope_cur, hd);
    f.args(a, 0);
    if (tiles == 0) tiles = std::min(std::max(n_ctx / 64, 1), 64);         // enqueue_layers' count at the default BAMD_QK_TILES
    if (bamd_launch_attention(a, H / Hkv, -tiles, nullptr)) return fail("unsupported head configuration");
    if (f.down(a, out, (size_t) H * hd, k_cache, v_cache_t)) return 1;
    return probs_h0 ? f.probs_down(a, n_kv, probs_h0) : 0;
}

// batched-prefill attention of T tokens at positions pos0 .. pos0 + T - 1 through the launcher enqueue_prefill_batch calls (KV store, then the matrix-core
// or VALU kernels), with the same argument block: q / k / v packed as one [T][H*hd + 2*Hkv*hd] matrix, batch_pos0p1, lds_ld, scratch block
// scratch_bytes: the budget of the scratch block handed to the slice plan (0 = the engine's rule); *n_slices (optional): attention launches issued behind the KV store
extern "C" __attribute__((visibility("default"))) int bamd_op_attention_batch_ex(const float * q, const float * k, const float * v, uint16_t * k_cache, uint16_t * v_cache_t,
                                                                                   const float * rope, int H, int Hkv, int hd, int n_ctx, int pos0, int T, int impl, int ld,
                                                                                   size_t scratch_bytes, float * out, int * n_slices) {
    if (need_device()) return 1;
    if (H <= 0 || Hkv <= 0 || hd <= 0 || hd % 64 || hd > 256 || n_ctx <= 0 || n_ctx % 32 || H % Hkv || H / Hkv > 8) return fail("bad attention shape");
    if (T < 1 || T > BAMD_PREFILL_CAP || pos0 < 0 || pos0 + T > n_ctx) return fail("bad micro-batch");
    if (impl < 0 || impl > 2) return fail("impl must be 0 (launcher's choice), 1 (VALU) or 2 (matrix cores)");
    AttnFixture f(n_ctx, Hkv, hd);
    const int Ekv = Hkv * hd, E = H * hd, ldq = E + 2 * Ekv, gq = H / Hkv;
    const int ld_min = std::min((pos0 + T + 63) / 64 * 64, f.n_ctx_pad);      // attn_lds_ld of the micro-batch's last position
    if (ld == 0) ld = ld_min;
    if (ld % 64 || ld < ld_min || ld > f.n_ctx_pad) return fail("ld must be a multiple of 64 between the padded sequence length and the padded n_ctx");
    std::vector<float> qkv((size_t) T * ldq);
    for (int i = 0; i < T; ++i) {
        memcpy(&qkv[(size_t) i * ldq], q + (size_t) i * E, (size_t) E * 4);
        memcpy(&qkv[(size_t) i * ldq + E], k + (size_t) i * Ekv, (size_t) Ekv * 4);
        memcpy(&qkv[(size_t) i * ldq + E + Ekv], v + (size_t) i * Ekv, (size_t) Ekv * 4);
    }
    bamd_step_state h; memset(&h, 0, sizeof h);                                 // as enqueue_prefill_batch sets it
    h.pos_base = pos0; h.pos = pos0; h.n_ctx = n_ctx; h.step = T; h.n_kv = std::min(n_ctx, (pos0 + T + 31) / 32 * 32);
    bamd_attn_args a; memset(&a, 0, sizeof a);
    a.st = (bamd_step_state *) f.up(&h, sizeof h);
    float * dqkv = (float *) f.up(qkv.data(), qkv.size() * 4);
    f.kv_up(k_cache, v_cache_t);
    a.rope = (float *) f.up(rope, (size_t) n_ctx * hd * 4); a.out = (float *) f.up(nullptr, (size_t) T * E * 4);
    if (!f.ok()) return fail("device alloc/copy failed");
    a.q = dqkv; a.k = dqkv + E; a.v = dqkv + E + Ekv;
    f.args(a, 1);
    a.batch = 1; a.ld_qkv = ldq; a.ld_out = E; a.lds_ld = ld; a.batch_pos0p1 = pos0 + 1;
    size_t need = 0;
    if (bamd_attention_batch_plan(Hkv, gq, hd, T, ld, impl, scratch_bytes, nullptr, nullptr, &need))
        return fail(impl == 2 && !(hd == 128 && T >= 2 && (gq == 1 || gq == 2 || gq == 4 || gq == 8)) ? "matrix-core kernel: shape not covered" : "batched attention: no slice plan (unsupported shape, or a scratch budget below one token tile)");
    if (need && !(a.batch_scratch = (float *) f.up(nullptr, need))) return fail("device alloc failed (scratch block)");
    int ns = 0;
    if (bamd_launch_attention_batch(a, gq, T, nullptr, impl, need, &ns)) return fail(impl == 2 ? "matrix-core kernel: shape not covered" : "batched attention: unsupported shape");
    if (n_slices) *n_slices = ns;
    return f.down(a, out, (size_t) T * E, k_cache, v_cache_t);
}
extern "C" __attribute__((visibility("default"))) int bamd_op_attention_batch(const float * q, const float * k, const float * v, uint16_t * k_cache, uint16_t * v_cache_t,
                                                                                const float * rope, int H, int Hkv, int hd, int n_ctx, int pos0, int T, int impl, int ld,
                                                                                float * out) {
    return bamd_op_attention_batch_ex(q, k, v, k_cache, v_cache_t, rope, H, Hkv, hd, n_ctx, pos0, T, impl, ld, 0, out, nullptr);
}

// ---- launches with more than one operand role, with the argument blocks of the engine (enqueue_layers, enqueue_prefill_batch) ----

// up to three K-quant matrices of `k` columns on the device as wave streams, with outputs one behind the other from `out` as qkv_segments / seg_of lay them
// out: nrows padded to 8 per segment, nvalid the real rows, segment i's output `rows[0] + .. + rows[i - 1]` floats behind `out`
struct SegFixture {
    bamd_mv_seg seg[3]; int nseg = 0, total = 0;
    uint32_t bf16_range[3] = { BAMD_BF16_RANGE_UNKNOWN, BAMD_BF16_RANGE_UNKNOWN, BAMD_BF16_RANGE_UNKNOWN };      // of the BF16 segments (bamd_bf16_range.h)
    int build(Tmp & t, int n, const int32_t * types, const void * const * w_raw, const int32_t * rows, int k, float * out, bool same_out = false) {
        if (n < 1 || n > 3 || k <= 0 || k % 256) return fail("bad segment count / row length");
        for (int i = 0; i < n; ++i) {
            if (!bamd_has_record(types[i]) || rows[i] <= 0 || !w_raw[i]) return fail("bad segment type / rows");
            const int pad = (rows[i] + 7) / 8 * 8;
            const size_t wb = bamd_row_bytes(types[i], k) * (size_t) rows[i], wbp = bamd_stream_bytes(types[i], k, pad);
            void * raw = t.up(w_raw[i], wb), * str = t.up(nullptr, wbp);
            if (!raw || !str) return fail("device alloc/copy failed");
            HIPC(hipMemset(str, 0, wbp));
            bamd_launch_repack(raw, str, types[i], rows[i], k, nullptr);
            if (types[i] == BAMD_BF16 && bamd_bf16_weight_range(str, wbp, &bf16_range[i], nullptr)) return fail("measuring the exponent range failed");
            seg[i].w = str; seg[i].out = same_out ? out : out + total; seg[i].type = types[i]; seg[i].nrows = pad; seg[i].nvalid = rows[i];
            total += rows[i];
        }
        nseg = n;
        return 0;
    }
};

// the fused QKV launch of a decode step (enqueue_layers, 1.): RMSNorm prologue + store over up to three differently typed segments
extern "C" __attribute__((visibility("default"))) int bamd_op_fused_qkv(int nseg, const int32_t * types, const void * const * w_raw, const int32_t * rows, int k, const float * x,
                                                                          const float * norm_w, float eps, int mode, float * y) {
    if (need_device()) return 1;
    if (nseg < 1 || nseg > 3 || !norm_w) return fail("bad segment count / no norm weight");
    int total = 0; for (int i = 0; i < nseg; ++i) { if (rows[i] <= 0) return fail("bad segment rows"); total += rows[i]; }
    Tmp t;
    float * dy = (float *) t.up(nullptr, (size_t) total * 4 + 64);           // (+ 64: a ragged last segment is padded to 8 rows in the stream, never in the output)
    float * dx = (float *) t.up(x, (size_t) k * 4), * dw = (float *) t.up(norm_w, (size_t) k * 4);
    if (!dy || !dx || !dw) return fail("device alloc/copy failed");
    SegFixture f; if (f.build(t, nseg, types, w_raw, rows, k, dy)) return 1;
    bamd_mv_args a; memset(&a, 0, sizeof a);
    for (int i = 0; i < nseg; ++i) a.seg[i] = f.seg[i];
    a.nseg = nseg; a.x = dx; a.normw = dw; a.eps = eps; a.K = k; a.mode = mode;
    if (bamd_launch_mv(a, BAMD_PRO_NORM, BAMD_EPI_STORE, n_cu0(), nullptr)) return fail("mat-vec: type without a kernel");
    return finish(y, dy, (size_t) total * 4);
}

// one batched prompt mat-mul as enqueue_prefill_batch issues it: up to three segments into one [T][ldo] matrix (STORE: the q | k | v call; ADD: one segment
// + residual; SILU_MUL: gate and up into the same columns), routed by bamd_batch_mm.  impl 0: no side tables (integer-dot kernel); impl 2: a side table for
// every segment whose type has a matrix-core kernel, built as build_prefill_aux builds them — the others stay on the integer-dot kernel.  F32 / F16 segments need
// no table: while BAMD_PREFILL_FLT is on, bamd_batch_mm sends them to their matrix-core kernel (at impl 0 as well, as the engine would); while it is off, and for
// BF16 while BAMD_PREFILL_BF16 is off, impl 2 is refused for the unquantised family
extern "C" __attribute__((visibility("default"))) int bamd_op_mul_mat_batch_seg(int nseg, const int32_t * types, const void * const * w_raw, const int32_t * rows, int k, const float * x,
                                                                                  int T, const float * norm_w, float eps, int ldo, const float * residual, int epi, int impl, float * y) {
    if (need_device()) return 1;
    if (T <= 0 || T > BAMD_PREFILL_CAP || ldo <= 0 || (impl != 0 && impl != 2)) return fail("bad T / ldo / impl");
    if (epi != BAMD_EPI_STORE && epi != BAMD_EPI_ADD && epi != BAMD_EPI_SILU_MUL) return fail("bad epilogue");
    if (nseg < 1 || nseg > 3 || (epi == BAMD_EPI_ADD && (nseg != 1 || !residual)) || (epi == BAMD_EPI_SILU_MUL && (nseg != 2 || rows[0] != rows[1]))) return fail("bad segments for this epilogue");
    int total = 0; for (int i = 0; i < nseg; ++i) { if (rows[i] <= 0) return fail("bad segment rows"); total += rows[i]; }
    if ((epi == BAMD_EPI_SILU_MUL ? rows[0] : total) > ldo) return fail("ldo smaller than the rows of a token");
    Tmp t; const size_t ob = (size_t) T * ldo * 4;
    float * dy = (float *) t.up(y, ob);                                      // the caller's content stays where the launch writes nothing
    float * dx = (float *) t.up(x, (size_t) T * k * 4); float * dw = norm_w ? (float *) t.up(norm_w, (size_t) k * 4) : nullptr;
    float * dres = residual ? (float *) t.up(residual, ob) : nullptr;
    void * blob = t.up(nullptr, (size_t) T * bamd_act_blob_bytes(bamd_act_form_of(types[0]), k)), * blob16 = t.up(nullptr, (size_t) T * bamd_blob16_bytes(k));
    if (!dy || !dx || !blob || !blob16 || (norm_w && !dw) || (residual && !dres)) return fail("device alloc/copy failed");
    SegFixture f; if (f.build(t, nseg, types, w_raw, rows, k, dy, epi == BAMD_EPI_SILU_MUL)) return 1;
    for (int i = 1; i < nseg; ++i) if (bamd_act_form_of(f.seg[i].type) != bamd_act_form_of(f.seg[0].type)) return fail(bamd_is_flt(f.seg[i].type) || bamd_is_flt(f.seg[0].type) ? "batched mat-mul: segments that need different activation forms (Q8_K, Q8_0, Q8_1, F32, BF16)" : bamd_is_q1(f.seg[i].type) || bamd_is_q1(f.seg[0].type) ? "batched mat-mul: segments that need different activation forms (Q8_K, Q8_0, Q8_1)" : "batched mat-mul: segments that need both activation forms (Q8_K and Q8_0)");
    bamd_bf16_ranges bf = { (const uint32_t *) t.up(nullptr, (size_t) T * 4), { f.bf16_range[0], f.bf16_range[1], f.bf16_range[2] } };
    if (!bf.x) return fail("device alloc failed");
    bamd_launch_quantize_batch(dx, dw, eps, k, T, blob, blob16, nullptr, bamd_act_form_of(f.seg[0].type), (uint32_t *) bf.x);
    const void * aux[3] = { nullptr, nullptr, nullptr };
    // (F32 / F16 with BAMD_PREFILL_FLT on have a matrix-core kernel without a side table: bamd_batch_mm routes them by the switch alone)
    if (impl == 2 && bamd_is_flt(f.seg[0].type) && !bamd_prefill_mfma_type_notable(f.seg[0].type)) return fail("MFMA path: unsupported type/shape (F32 / F16 / BF16 have no matrix-core kernel)");
    if (impl == 2) for (int i = 0; i < nseg; ++i) {
        const size_t ab = bamd_prefill_aux_bytes(f.seg[i].type, f.seg[i].nrows, k);
        if (!ab) continue;                                                   // Q2_K / Q3_K with the switch off, or a shape without a matrix-core kernel
        void * ax = t.up(nullptr, ab);
        if (!ax) return fail("device alloc failed");
        bamd_launch_prefill_aux(f.seg[i].w, f.seg[i].type, f.seg[i].nrows, k, ax, nullptr);
        aux[i] = ax;
    }
    bamd_mm_args a; memset(&a, 0, sizeof a);
    for (int i = 0; i < nseg; ++i) a.seg[i] = f.seg[i];
    a.nseg = nseg; a.blob = (const uint8_t *) blob; a.K = k; a.T = T; a.ldo = ldo; a.res = epi == BAMD_EPI_ADD ? dres : nullptr;
    if (bamd_batch_mm(a, epi, blob16, aux, n_cu0(), nullptr, &bf)) return fail("batched mat-mul: unsupported shape");
    return finish(y, dy, ob);
}

// attention and the wo projection of one decode layer in ONE launch (bamd_launch_attn_wo), with the argument blocks of enqueue_layers: the attention block as
// bamd_op_attention fills it plus lds_ld (0: the engine's min(512, padded n_ctx)) and rope_cur, the wo block with a.x = the attention output vector, a.res = the
// residual, mode 0, n_cu from the device.  serial / step / il make the tag of this launch; gran_init (null: zeros) is what the H * hd granules hold before it.
// *declined = 1: the launcher has no co-launch for this shape (nothing ran, no output is written)
extern "C" __attribute__((visibility("default"))) int bamd_op_attention_wo(const float * q, const float * k, const float * v, uint16_t * k_cache, uint16_t * v_cache_t,
                                                                             const float * rope_row_h, int H, int Hkv, int hd, int n_ctx, int pos, int lds_ld, int wo_type,
                                                                             const void * wo_raw, int wo_rows, const float * residual, int serial, int step, int il,
                                                                             int with_cellpos, const uint64_t * gran_init, float * x2, uint64_t * gran_out, uint32_t * gave_up,
                                                                             int32_t * declined, int32_t * n_cu_used) {
    if (need_device()) return 1;
    if (H <= 0 || Hkv <= 0 || hd <= 0 || hd % 64 || hd > 256 || n_ctx <= 0 || pos < 0 || pos >= n_ctx || n_ctx % 32 || H % Hkv) return fail("bad attention shape");
    const int K = H * hd;
    if (!bamd_has_record(wo_type) || K % 256 || wo_rows <= 0 || !residual) return fail("bad wo type/shape, or no residual");
    AttnFixture f(n_ctx, Hkv, hd); const int Ekv = Hkv * hd;
    bamd_step_state h; memset(&h, 0, sizeof h);
    h.pos_base = pos; h.pos = pos; h.n_ctx = n_ctx; h.n_kv = std::min(n_ctx, std::max(32, (pos + 1 + 31) / 32 * 32)); h.serial = serial; h.step = step;
    if (lds_ld == 0) lds_ld = std::min(512, f.n_ctx_pad);                       // enqueue_layers
    if (lds_ld % 64 || lds_ld < (h.n_kv + 63) / 64 * 64 || lds_ld > f.n_ctx_pad) return fail("lds_ld must be a multiple of 64 between the padded sequence length and the padded n_ctx");
    std::vector<float> rope((size_t) n_ctx * hd, 0.f);
    memcpy(rope.data() + (size_t) pos * hd, rope_row_h, (size_t) hd * 4);
    std::vector<uint64_t> g0((size_t) K, 0ull);
    if (gran_init) memcpy(g0.data(), gran_init, (size_t) K * 8);
    std::vector<int32_t> cp((size_t) f.n_ctx_pad, -1);
    for (int i = 0; i <= pos; ++i) cp[(size_t) i] = i;
    const uint32_t zero8[8] = { 0 };
    bamd_attn_args a; memset(&a, 0, sizeof a);
    a.st = (bamd_step_state *) f.up(&h, sizeof h);
    a.q = (float *) f.up(q, (size_t) K * 4); a.k = (float *) f.up(k, (size_t) Ekv * 4); a.v = (float *) f.up(v, (size_t) Ekv * 4);
    f.kv_up(k_cache, v_cache_t);
    a.rope = (float *) f.up(rope.data(), rope.size() * 4); a.rope_cur = (float *) f.up(rope_row_h, (size_t) hd * 4);
    f.rows(a, H);
    unsigned long long * gran = (unsigned long long *) f.up(g0.data(), (size_t) K * 8);
    uint32_t * err = (uint32_t *) f.up(zero8, sizeof zero8);
    if (with_cellpos) a.cellpos = (const int32_t *) f.up(cp.data(), cp.size() * 4);
    const int nrows_pad = (wo_rows + 7) / 8 * 8;
    const size_t wb = bamd_row_bytes(wo_type, K) * (size_t) wo_rows, wbp = bamd_stream_bytes(wo_type, K, nrows_pad);
    void * raw = f.up(wo_raw, wb), * str = f.up(nullptr, wbp);
    float * dres = (float *) f.up(residual, (size_t) wo_rows * 4), * dx2 = (float *) f.up(nullptr, (size_t) nrows_pad * 4);
    if (!f.ok()) return fail("device alloc/copy failed");
    HIPC(hipMemset(str, 0, wbp));
    HIPC(hipMemset(dx2, 0, (size_t) nrows_pad * 4));
    bamd_launch_repack(raw, str, wo_type, wo_rows, K, nullptr);
    f.args(a, 0);
    a.lds_ld = lds_ld;
    if (bamd_attention_split_is_ik_clean(a, H / Hkv)) a.probs = nullptr;        // enqueue_layers: the probability rows in global memory belong to the softmax | P.V pair only
    bamd_mv_args w; memset(&w, 0, sizeof w);
    w.seg[0].w = str; w.seg[0].out = dx2; w.seg[0].type = wo_type; w.seg[0].nrows = nrows_pad; w.seg[0].nvalid = wo_rows; w.nseg = 1;
    w.x = a.out; w.K = K; w.res = dres;
    const int n_cu = n_cu0();
    *n_cu_used = n_cu;
    *declined = bamd_launch_attn_wo(a, H / Hkv, w, n_cu, gran, il & 255, err, nullptr) != 0;
    if (*declined) return 0;
    if (finish(x2, dx2, (size_t) wo_rows * 4) || f.kv_down(k_cache, v_cache_t)) return 1;
    HIPC(hipMemcpy(gran_out, gran, (size_t) K * 8, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(gave_up, err, 4, hipMemcpyDeviceToHost));
    return 0;
}

// ---- launch-selection trace: which kernel, grid, LDS and arguments the launchers choose for a shape, from the recording path of BAMD_LAUNCH (host code only) ----
template <typename T> static T * fake_ptr(int field) { return (T *) (uintptr_t) (0x10000u * (unsigned) (field + 1)); }      // distinct per field, never dereferenced
static int trace_result(const bamd_aql_recording & rec, bamd_launch_trace * out) {
    if (rec.launches.size() != 1) return fail("launch trace: " + std::to_string(rec.launches.size()) + " launches recorded, expected one"), 2;
    const bamd_aql_launch & l = rec.launches[0];
    const char * name = hipKernelNameRefByPtr(l.host_fn, nullptr);
    if (!name || strlen(name) >= sizeof out->kernel) return fail("launch trace: kernel name not resolved"), 2;
    memset(out, 0, sizeof *out);
    strcpy(out->kernel, name);
    for (int i = 0; i < 3; ++i) { out->grid[i] = l.grid[i]; out->block[i] = l.block[i]; }
    out->lds_bytes = l.lds_bytes; out->kernarg_bytes = (uint32_t) l.kernarg.size();
    uint64_t h = 0xcbf29ce484222325ull;
    for (uint8_t b : l.kernarg) h = (h ^ b) * 0x100000001b3ull;
    out->kernarg_hash = h;
    return 0;
}
struct TraceScope {                      // BAMD_LAUNCH records into `rec` while this lives
    bamd_aql_recording rec; bamd_aql_recording * prev;
    TraceScope() : prev(bamd_aql_rec) { bamd_aql_rec = &rec; }
    ~TraceScope() { bamd_aql_rec = prev; }
};
// any: through bamd_launch_mv, what the engine and the ops call (every family of types); else bamd_launch_matvec itself, the K-quant launcher
static int trace_mv(bool any, int nseg, const int32_t * types, const int32_t * rows, int k, int pro, int epi, int mode, int n_cu, bamd_launch_trace * out) {
    if (nseg < 1 || nseg > 3 || k <= 0 || k % 256 || !out) return fail("launch trace: bad segment count / row length"), 2;
    if ((pro != BAMD_PRO_PLAIN && pro != BAMD_PRO_NORM) || epi < BAMD_EPI_STORE || epi > BAMD_EPI_ARGMAX) return fail("launch trace: bad prologue / epilogue"), 2;
    bamd_mv_args a; memset(&a, 0, sizeof a);
    float * y = fake_ptr<float>(8);
    int off = 0;
    for (int i = 0; i < nseg; ++i) {                                          // seg_of / qkv_segments; gate and up write the same output
        if (rows[i] <= 0) return fail("launch trace: bad segment rows"), 2;
        a.seg[i].w = fake_ptr<uint8_t>(i); a.seg[i].out = epi == BAMD_EPI_SILU_MUL ? y : y + off; a.seg[i].type = types[i];
        a.seg[i].nrows = (rows[i] + 7) / 8 * 8; a.seg[i].nvalid = rows[i];
        off += rows[i];
    }
    a.nseg = nseg; a.x = fake_ptr<float>(3); a.K = k; a.mode = mode;
    if (pro == BAMD_PRO_NORM) { a.normw = fake_ptr<float>(4); a.eps = 1e-5f; }
    if (epi == BAMD_EPI_ADD) a.res = fake_ptr<float>(5);
    if (epi == BAMD_EPI_ARGMAX) a.best_key = fake_ptr<unsigned long long>(6);
    TraceScope ts;
    if (any ? bamd_launch_mv(a, pro, epi, n_cu, nullptr) : bamd_launch_matvec(a, pro, epi, n_cu, nullptr)) return 1;
    return trace_result(ts.rec, out);
}
extern "C" __attribute__((visibility("default"))) int bamd_trace_matvec(int nseg, const int32_t * types, const int32_t * rows, int k, int pro, int epi, int mode, int n_cu,
                                                                          bamd_launch_trace * out) {
    return trace_mv(false, nseg, types, rows, k, pro, epi, mode, n_cu, out);
}
extern "C" __attribute__((visibility("default"))) int bamd_trace_mv(int nseg, const int32_t * types, const int32_t * rows, int k, int pro, int epi, int mode, int n_cu,
                                                                      bamd_launch_trace * out) {
    return trace_mv(true, nseg, types, rows, k, pro, epi, mode, n_cu, out);
}
extern "C" __attribute__((visibility("default"))) int bamd_trace_attn_wo(int H, int Hkv, int hd, int n_ctx, int lds_ld, int with_cellpos, int wo_type, int wo_rows, int k,
                                                                           int n_cu, int il, bamd_launch_trace * out) {
    if (H <= 0 || Hkv <= 0 || H % Hkv || hd <= 0 || n_ctx <= 0 || wo_rows <= 0 || k <= 0 || k % 256 || !out) return fail("launch trace: bad attention / wo shape"), 2;
    bamd_attn_args t; memset(&t, 0, sizeof t);                               // enqueue_layers, 2.
    t.st = fake_ptr<bamd_step_state>(16); t.q = fake_ptr<float>(17); t.k = fake_ptr<float>(18); t.v = fake_ptr<float>(19);
    t.kc = fake_ptr<unsigned short>(20); t.vc = fake_ptr<unsigned short>(21); t.rope = fake_ptr<float>(22); t.rope_cur = fake_ptr<float>(23);
    t.scores = fake_ptr<float>(24); t.out = fake_ptr<float>(25);
    t.hd = hd; t.Hkv = Hkv; t.n_ctx = n_ctx; t.kq_scale = 1.0f / sqrtf((float) hd); t.lds_ld = lds_ld;
    if (with_cellpos) t.cellpos = fake_ptr<int32_t>(26);
    bamd_mv_args a; memset(&a, 0, sizeof a);                                 // enqueue_layers, 3.
    a.seg[0].w = fake_ptr<uint8_t>(0); a.seg[0].out = fake_ptr<float>(8); a.seg[0].type = wo_type; a.seg[0].nrows = (wo_rows + 7) / 8 * 8; a.seg[0].nvalid = wo_rows;
    a.nseg = 1; a.x = t.out; a.K = k; a.res = fake_ptr<float>(5);
    TraceScope ts;
    if (bamd_launch_attn_wo(t, H / Hkv, a, n_cu, fake_ptr<unsigned long long>(27), il, fake_ptr<uint32_t>(28), nullptr)) return 1;
    return trace_result(ts.rec, out);
}

// ---- micro-benchmark of one mat-vec launch shape (random resident weights; HIP-event timing of `iters` launches) ----
extern "C" __attribute__((visibility("default"))) int bamd_bench_matvec(int type, int nrows, int k, int pro, int epi, int mode, int iters,
                                                                        float * us_per_launch) {
    if (need_device()) return 1;
    if (!bamd_has_record(type) || k % 256 || nrows % 8) return fail("bad type/shape");
    Tmp t; const size_t wb = bamd_row_bytes(type, k) * (size_t) nrows;
    std::vector<uint8_t> hw(wb);
    uint32_t sd = 12345u; for (size_t i = 0; i < wb; ++i) { sd = sd * 1664525u + 1013904223u; hw[i] = (uint8_t) (sd >> 24); }
    const int bb = bamd_block_bytes(type);
    if (bamd_is_flt(type)) {                                  // finite values around 0.004 of either sign
        for (size_t i = 0; i < wb / (type == BAMD_F32 ? 4 : 2); ++i) {
            if (type == BAMD_F32) { hw[4 * i + 3] = (uint8_t) (0x3b | (hw[4 * i + 3] & 0x80)); hw[4 * i + 2] |= 0x80; }
            else if (type == BAMD_F16) hw[2 * i + 1] = (uint8_t) (0x1c | (hw[2 * i + 1] & 0x83));
            else { hw[2 * i + 1] = (uint8_t) (0x3b | (hw[2 * i + 1] & 0x80)); hw[2 * i] |= 0x80; }
        }
    } else
    for (size_t b = 0; b < wb / bb; ++b) {                    // sane f16 scales (0x1c00 ~ 0.0039)
        uint8_t * p = hw.data() + b * bb;
        if (type == BAMD_Q6_K) { p[208] = 0x00; p[209] = 0x1c; }
        else if (type == BAMD_Q3_K) { p[108] = 0x00; p[109] = 0x1c; }
        else if (type == BAMD_Q2_K) { p[80] = 0; p[81] = 0x1c; p[82] = 0; p[83] = 0x1c; }
        else if (bamd_takes_q8_0(type) || type == BAMD_IQ4_XS) { p[0] = 0; p[1] = 0x1c; }      // (IQ4_XS: d alone, scales_h stays random)
        else if (bamd_is_q1(type)) { p[0] = 0; p[1] = 0x1c; p[2] = 0; p[3] = 0x1c; }
        else { p[0] = 0; p[1] = 0x1c; p[2] = 0; p[3] = 0x1c; }
    }
    std::vector<float> hx((size_t) k); for (int i = 0; i < k; ++i) { sd = sd * 1664525u + 1013904223u; hx[i] = (float) (int) (sd >> 8) / 8388608.0f - 1.0f; }
    std::vector<float> hn((size_t) k, 1.0f);
    const size_t wbs = bamd_stream_bytes(type, k, nrows);
    void * raw = t.up(hw.data(), wb), * strA = t.up(nullptr, wbs), * strB = epi == BAMD_EPI_SILU_MUL ? t.up(nullptr, wbs) : nullptr;
    float * dx = (float *) t.up(hx.data(), (size_t) k * 4), * dw = (float *) t.up(hn.data(), (size_t) k * 4);
    float * dres = (float *) t.up(nullptr, (size_t) nrows * 4), * dy = (float *) t.up(nullptr, (size_t) nrows * 4);
    unsigned long long * key = (unsigned long long *) t.up(nullptr, 8);
    if (!raw || !strA || !dx || !dw || !dres || !dy || !key) return fail("device alloc/copy failed");
    HIPC(hipMemset(dres, 0, (size_t) nrows * 4)); HIPC(hipMemset(key, 0, 8));
    bamd_launch_repack(raw, strA, type, nrows, k, nullptr);
    if (strB) bamd_launch_repack(raw, strB, type, nrows, k, nullptr);
    bamd_mv_args a; memset(&a, 0, sizeof a);
    a.seg[0].w = strA; a.seg[0].out = dy; a.seg[0].type = type; a.seg[0].nrows = nrows; a.nseg = 1;
    if (strB) { a.seg[1] = a.seg[0]; a.seg[1].w = strB; a.nseg = 2; }
    a.x = dx; a.normw = dw; a.eps = 1e-5f; a.K = k; a.res = dres; a.best_key = key; a.mode = mode;
    const int ncu = n_cu0();
    if (iters < 1) return fail("iters < 1");
    OwnedStream os; HIPC(hipStreamCreate(&os.s));
    hipStream_t s = os.s;
    for (int i = 0; i < 3; ++i) if (bamd_launch_mv(a, pro, epi, ncu, s)) return fail("mat-vec: type without a kernel");
    HIPC(hipGetLastError());
    EventPair ev; HIPC(ev.create());
    HIPC(hipEventRecord(ev.a, s));
    for (int i = 0; i < iters; ++i) if (bamd_launch_mv(a, pro, epi, ncu, s)) return fail("mat-vec: type without a kernel");
    HIPC(hipEventRecord(ev.b, s));
    HIPC(hipStreamSynchronize(s));
    float ms = 0.f; HIPC(hipEventElapsedTime(&ms, ev.a, ev.b));
    *us_per_launch = ms * 1000.0f / (float) iters;
    return 0;
}
