// bamd_kernels.h — host-visible launch interface of the kernel files (bamd_matvec*.hip, bamd_attention*.hip, bamd_colaunch.hip, bamd_prefill*.hip, bamd_sampler.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/bamd.h"   // bamd_logit_penalty, bamd_shortlist_head
#include "bamd_formats.h"
#include "bamd_bf16_range.h"

enum { BAMD_PRO_PLAIN = 0, BAMD_PRO_NORM = 1 };
enum { BAMD_EPI_STORE = 0, BAMD_EPI_ADD = 1, BAMD_EPI_SILU_MUL = 2, BAMD_EPI_ARGMAX = 3 };

// device-resident decode state: lets a whole decode step (and a captured hipGraph of it) run without host input
struct bamd_step_state {
    int32_t pos_base;              // position of the token of step 0
    int32_t step;                  // steps begun so far
    int32_t pos, n_kv, token;      // this step: position, padded KV length (llama.cpp:14693-14701), token id
    int32_t n_ctx;
    int32_t n_out;                 // arg-max tokens appended to out_tokens so far
    int32_t cell;                  // KV cell this step's token is stored in: = pos until positions were shifted (bamd_kv_seq_add), then the slot
                                   // llama_kv_cache_find_slot picks (llama.cpp:3028-3127)
    int32_t cell_plus1;            // host: cell of step 0 + 1 (0 = cells follow positions)
    int32_t n_kv_fixed;            // host: padded KV length of this step when cells no longer follow positions (0 = from pos)
    int32_t serial;                // host: 12-bit counter of the host calls that set this state (tag of the co-launch flag words, bamd_colaunch.hip)
    unsigned long long best_key;   // arg-max key of the last lm_head (0 = none)
};

struct bamd_mv_seg { const void * w; float * out; int type; int nrows; int nvalid; };   // nrows: multiple of 8 (stream rows, zero-padded); nvalid: real rows (0 = nrows)
struct bamd_mv_args {
    bamd_mv_seg seg[3]; int nseg;
    const float * x;               // f32 activation [K]
    const float * normw;           // RMSNorm weight (BAMD_PRO_NORM)
    float eps; int K;
    const float * res;             // residual (BAMD_EPI_ADD), indexed like seg[0].out
    unsigned long long * best_key; // BAMD_EPI_ARGMAX
    int mode;                      // 0 auto, 1 force one-wave-per-row-group, 2 force split-K (tests); + 16: force the generic kernels
    int cnt_q, cnt_r;              // fast kernels: row-groups per wave slot (mode A) / per workgroup (mode B), quotient and remainder (set by the launcher)
    unsigned long long * tl;       // phase-stamp block of this launch (BAMD_TIMING builds; null = off)
};

struct bamd_attn_args {
    const bamd_step_state * st;
    const float * q, * k, * v;     // f32 [H*hd], [Hkv*hd], [Hkv*hd] of this token (pre-RoPE)
    unsigned short * kc, * vc;     // f16 caches of this layer, chain-major order (bamd_device.h): K [n_ctx][Hkv*hd], V^T [Hkv*hd][n_ctx]; n_ctx % 64 == 0
    const float * rope;            // [n_ctx][hd] (cos,sin) pairs
    const float * rope_cur;        // [hd]: the row of the CURRENT position, left at this fixed address by step_begin_kernel (the long-sequence score kernel requests it
                                   // without a dependent load of the position in front); null = take the row from `rope` (op-level tests, batched prefill)
    float * scores;                // [H][n_ctx] scratch: scores (long-context path)
    float * probs;                 // [H][n_ctx] scratch: probabilities in V^T position order (long-context path)
    float * out;                   // [H*hd]
    int hd, Hkv, n_ctx;
    float kq_scale;
    int prefill_mode;              // 1: KQ with the T>1 semantics of the reference (q -> f16, ggml_vec_dot_f16)
    int batch, ld_qkv, ld_out;     // batched prefill: q/k/v and out are [T][ld_*] f32, token = blockIdx.y, position st->pos + token
    float * batch_scratch;         // batched prefill, more than 512 positions (BAMD_AM_MAXPOS): score rows of the matrix-core kernel (bamd_attention_batch_mfma_scratch bytes); null: the VALU kernel
    int batch_pos0p1;              // batched prefill: the position of token 0, plus one (= st->pos + 1, known to the host: the matrix-core kernel takes it from here
                                   // and starts its requests without a dependent load of the device state); 0 = read st->pos
    int lds_ld;                    // single-launch / batched kernels: floats per score / probability row in LDS — a multiple of 64 that bounds the padded
                                   // sequence length of this launch (or of every replay of the graph it is captured in); 0 = n_ctx
    unsigned long long * tl;       // phase-stamp block of this launch (BAMD_TIMING builds; null = off)
    const int32_t * cellpos;       // [n_ctx] position held by every KV cell, -1 = free (after a context shift: cells no longer follow positions; the mask
                                   // is the reference's "cell.pos > pos or empty -> -inf", llama.cpp:14152-14200); null = cell i holds position i
};

// batched prefill mat-mul: Y[t][row] = W[row,:] . Q8_K(a_t), T tokens
struct bamd_mm_args {
    bamd_mv_seg seg[3]; int nseg;  // as bamd_mv_args; seg[].out = base of the [T][ldo] output of that segment's rows
    const uint8_t * blob;          // [T][bamd_blob_bytes(K)] quantised activations (bamd_launch_quantize_batch)
    int K, T, ldo;                 // ldo: floats between consecutive tokens in every output / residual matrix
    const float * res;             // BAMD_EPI_ADD: residual, indexed like seg[0].out
};

#define BAMD_TL_WG 512                 /* workgroups recorded per launch (phase stamps, BAMD_TIMING builds) */
#define BAMD_TL_WG_WORDS 24            /* per workgroup: [wave 0: 8 phases][wave 7: 8 phases][exit stamp of each of 8 waves] */
#define BAMD_TL_SLOT_WORDS (BAMD_TL_WG * BAMD_TL_WG_WORDS)
int  bamd_timing_enabled(void);   // 1 when the kernels were compiled with -DBAMD_TIMING
void bamd_launch_repack(const void * raw, void * dst, int type, int nrows, int K, hipStream_t s);
void bamd_launch_quantize_q8k_test(const float * x, const float * nw, float eps, int K, int norm, void * out, hipStream_t s);
[[nodiscard]] int bamd_launch_matvec(const bamd_mv_args & a, int pro, int epi, int n_cu, hipStream_t s);          // 1 = a segment's type has no kernel (nothing launched)
// the same for launches whose segments are all of ONE family of the 32-weight block formats (bamd_matvec_b32.h): Q8_0 / Q4_0 / Q5_0 (Q8_0 activations) or
// Q4_1 / Q5_1 (Q8_1 activations); the family of segment 0 decides, 1 = a segment of the other family; 2 = split-K (mode 2) was asked for Q4_1 / Q5_1, which do not have it.
// IQ4_NL counts to the first family (Q8_0 activations): a launch with such a segment takes a kernel of its own, 2 = split-K was asked for in such a launch
[[nodiscard]] int bamd_launch_matvec_b32(const bamd_mv_args & a, int pro, int epi, int n_cu, hipStream_t s);
[[nodiscard]] int bamd_launch_matvec_b32_q1(const bamd_mv_args & a, int pro, int epi, int n_cu, hipStream_t s);      // its Q4_1 / Q5_1 half (a code object per family: bamd_matvec_b32.h)
// and the launches of the first family with at least one IQ4_NL segment (a third code object, bamd_matvec_b32_nl.hip); 2 = split-K (mode 2) was asked for: IQ4_NL has none
[[nodiscard]] int bamd_launch_matvec_b32_nl(const bamd_mv_args & a, int pro, int epi, int n_cu, hipStream_t s);
// what the engine and the ops call: the family of the first segment picks the launcher, and each launcher refuses a segment of another family (a launch
// quantises its activations once, as Q8_K, as Q8_0 or as Q8_1: bamd_act_form_of).  bamd_launch_matvec itself stays the K-quant launcher that tests/test_launch_selection.py pins, its
// refusal of every other type included
// the unquantised family, F32 / F16 (f32 activations) and BF16 (bf16 activations): bamd_matvec_flt.hip; 1 = a segment of another activation form, or a K the LDS does not hold
[[nodiscard]] int bamd_launch_matvec_flt(const bamd_mv_args & a, int pro, int epi, int n_cu, hipStream_t s);
void bamd_launch_repack_flt(const void * raw, void * dst, int type, int nrows, int K, hipStream_t s);                  // behind bamd_launch_repack
void bamd_launch_act_bf16_test(const float * x, const float * nw, float eps, int K, int norm, void * out, hipStream_t s);
// batched prompt path of that family (bamd_prefill_flt.hip; behind bamd_launch_quantize_batch / bamd_launch_matmul_batch): a token's activations are
// bamd_flt_act_bytes(form, K) bytes, in the order the chains read them
// xrange (bf16 form; null: none): [T] range words of the tokens' stored patterns, for bamd_launch_matmul_mfma_bf16 (bamd_bf16_range.h)
void bamd_launch_act_batch_flt(int form, const float * x, const float * nw, float eps, int K, int T, void * blob, hipStream_t s, uint32_t * xrange = nullptr);
int  bamd_launch_matmul_batch_flt(const bamd_mm_args & a, int epi, int n_cu, hipStream_t s);
[[nodiscard]] static inline int bamd_launch_mv(const bamd_mv_args & a, int pro, int epi, int n_cu, hipStream_t s) {
    if (a.nseg > 0 && bamd_is_flt(a.seg[0].type)) return bamd_launch_matvec_flt(a, pro, epi, n_cu, s);
    return a.nseg > 0 && bamd_is_b32(a.seg[0].type) ? bamd_launch_matvec_b32(a, pro, epi, n_cu, s) : bamd_launch_matvec(a, pro, epi, n_cu, s);
}
void bamd_launch_quantize_q81_test(const float * x, const float * nw, float eps, int K, int norm, void * out, hipStream_t s);
void bamd_launch_quantize_q80_test(const float * x, const float * nw, float eps, int K, int norm, void * out, hipStream_t s);
void bamd_launch_step_begin(bamd_step_state * st, const int32_t * forced, int n_forced, int32_t * out_tokens, const void * embd,
                            int embd_type, int E, int V, float * x, int do_embed, hipStream_t s, const int32_t * slots = nullptr, int32_t * cellpos = nullptr,
                            const float * rope = nullptr, float * rope_cur = nullptr, int hd = 0, const bamd_step_state * inbox = nullptr);
int  bamd_launch_attention(const bamd_attn_args & a, int gq, int max_tiles, hipStream_t s);
int  bamd_attention_split_is_ik_clean(const bamd_attn_args & a, int gq);      // the long-sequence path of this shape keeps the inter-kernel rules (bamd_device.h): own-queue replay allowed
// single-launch attention and the wo projection (+ residual) behind it in ONE launch (bamd_colaunch.hip); gran: [H * hd] zero-initialised 8-byte
// granules of the context (the attention output travels through them), il: layer index (part of the tag), err: give-up counter.
// 1 = this shape has no co-launch kernel: issue the two launches
int  bamd_launch_attn_wo(const bamd_attn_args & t, int gq, const bamd_mv_args & wo, int n_cu, unsigned long long * gran, int il, uint32_t * err, hipStream_t s);
// K-shift (build_k_shift, llama.cpp:8482-8512 -> ggml_compute_forward_rope_f16, ggml.c:14169-14290): every cell's K row re-rotated in place by
// the cos / sin row tab[tab_of_cell[cell]] (row 0 = delta 0); kc chain-major f16 [n_cells][Hkv*hd]
void bamd_launch_k_shift(unsigned short * kc, int n_cells, int Hkv, int hd, const int32_t * tab_of_cell, const float * tab, hipStream_t s);
size_t bamd_blob_bytes(int K);
size_t bamd_blob16_bytes(int K);
// bytes of one token's activations in `form` (any bamd_act_form): what a caller of bamd_launch_quantize_batch allocates per token
static inline size_t bamd_act_blob_bytes(int form, int K) { const size_t f = bamd_flt_act_bytes(form, K); return f ? f : bamd_blob_bytes(K); }
// blob: int8 activations for matmul_batch_kernel (may be null); blob16: f16 copy for the MFMA kernel (may be null)
// form (bamd_act_form_of the consuming mat-mul's weights): BAMD_ACT_Q8_0 for Q8_0 / Q4_0 / Q5_0 weights, BAMD_ACT_Q8_1 for Q4_1 / Q5_1 — blob takes the Q8_0 / Q8_1 form
// of the same size (bamd_prefill_b32.hip); blob16 is written, in the f16 form of bamd_prefill2_b32.hip (544 / 576 bytes of a record, the same per-token stride), only
// while a family that reads this form is on (bamd_prefill_reads_act16, bamd_prefill_family.h; otherwise nothing reads it)
// bf16_range (BAMD_ACT_BF16 only; null: none): [T] words, one per token: the exponent range of its bf16 activations (bamd_bf16_range.h), written for the guard of
// the BF16 matrix-core kernel; the blob is the same with and without
void bamd_launch_quantize_batch(const float * x, const float * nw, float eps, int K, int T, void * blob, void * blob16, hipStream_t s, int form = BAMD_ACT_Q8_K, uint32_t * bf16_range = nullptr);
void bamd_launch_quantize_batch_b32(int form, const float * x, const float * nw, float eps, int K, int T, void * blob, hipStream_t s, void * blob16 = nullptr);
int  bamd_launch_matmul_batch_b32_nl(const bamd_mm_args & a, int epi, int n_cu, hipStream_t s);       // its launches with an IQ4_NL segment (bamd_prefill_b32_nl.hip); callers go through the next
int  bamd_launch_matmul_batch_b32(const bamd_mm_args & a, int epi, int n_cu, hipStream_t s);          // every segment of the family of segment 0 (Q8_0 / Q4_0 / Q5_0, or Q4_1 / Q5_1), a.blob in its form; 1 = shape not supported
// K-quant matrices on the matrix cores, exact (bamd_prefill2.hip): y[t][row] = W[row,:] . Q8_K(a_t); epi BAMD_EPI_STORE: out = y; BAMD_EPI_ADD: out = y + res;
// BAMD_EPI_SILU_MUL: out = silu(res) * y (res = the gate projection, may alias out).  The A fragments are built once per 64-row x 64-token workgroup from the
// wave-stream copy and the matrix's load-time side table (aux: bamd_prefill_aux_bytes bytes, filled by bamd_launch_prefill_aux).  1 = type / shape not supported or no table
// (Q4_K / Q5_K: the sixteen-wave matmul_mfma3_q4k_kernel; Q6_K / Q3_K / Q2_K: the eight-wave matmul_mfma2_kernel, one body with a policy struct per format)
int  bamd_prefill_mfma_supported(void);      // the current device accepts the kernels' LDS size (asked at model load)
// which weight types have such a kernel now, and the switches they are behind (bamd_prefill_mfma_type and its kin): bamd_prefill_family.h
size_t bamd_prefill_aux_bytes(int type, int nrows_pad, int K);
void bamd_launch_prefill_aux(const void * w_stream, int type, int nrows_pad, int K, void * aux, hipStream_t s);
int  bamd_launch_matmul_mfma2(const void * w_stream, const void * aux, int type, int nrows, int nrows_pad, int K, const void * blob16, int T, float * out, const float * res,
                              int epi, int ldo, hipStream_t s);
// the side of the three entry points above for the 32-weight block formats, Q8_0 / Q4_0 / Q5_0 / Q4_1 / Q5_1 and IQ4_NL (the Q4_0 table), one kernel template
// (bamd_prefill2_b32.hip); callers go through those
size_t bamd_prefill_aux_bytes_b32(int type, int nrows_pad, int K);
void bamd_launch_prefill_aux_b32(const void * w_stream, int type, int nrows_pad, int K, void * aux, hipStream_t s);
int  bamd_launch_matmul_mfma_b32(const void * w_stream, const void * aux, int type, int nrows, int nrows_pad, int K, const void * blob16, int T, float * out, const float * res,
                                 int epi, int ldo, hipStream_t s);
// F32 / F16 matrices on the matrix cores, exact (bamd_prefill2_flt.hip): the kernel reads the resident weight stream and the f32 activation rows of
// bamd_launch_act_batch_flt (blob) as they are, there is no side table to build.  BF16: the kernel below.  Epilogues as bamd_launch_matmul_mfma2; 1 = type / shape
// not supported.  bamd_prefill_mfma_count: one more launch of `type` for bamd_prefill_mfma_runs (every matrix-core launcher; the counters live in bamd_prefill2.hip)
int  bamd_launch_matmul_mfma_flt(const void * w_stream, int type, int nrows, int nrows_pad, int K, const void * blob, int T, float * out, const float * res, int epi, int ldo,
                                 hipStream_t s);
void bamd_prefill_mfma_count(int type);
// BF16 matrices on the matrix cores, exact (bamd_prefill2_bf16.hip; BAMD_PREFILL_BF16): the resident weight stream and the bf16 activation rows of
// bamd_launch_act_batch_flt as they are, no side table.  wrange: the range word of the matrix (bamd_bf16_weight_range over its stream: synchronises s, load time
// only), xrange: [T] the tokens' range words, written by the activation pass — a workgroup whose ranges do not prove every product exact in f32 runs the VALU
// step instead and is counted (bamd_bf16_fallback_tiles_all: synchronises every device that launched, sums the counters).  1 = shape not supported
int  bamd_bf16_weight_range(const void * w_stream, size_t bytes, uint32_t * word, hipStream_t s);
int  bamd_launch_matmul_mfma_bf16(const void * w_stream, uint32_t wrange, int nrows, int nrows_pad, int K, const void * blob, const uint32_t * xrange, int T, float * out,
                                  const float * res, int epi, int ldo, hipStream_t s);
unsigned long long bamd_bf16_fallback_tiles_all(void);
int  bamd_launch_matmul_batch(const bamd_mm_args & a, int epi, int n_cu, hipStream_t s);      // 1 = shape not supported
void bamd_launch_embed_batch(const int32_t * tokens, int T, const void * embd, int embd_type, int E, int V, float * x, hipStream_t s);
// impl: 0 = the matrix-core kernel where it covers the shape, else the VALU kernels (the engine); 1 = the VALU kernels only; 2 = the matrix-core
// kernel only (1 when it declines the shape — after the KV store).  Op-level tests select the path; the engine passes the default.
// scratch_bytes: size of a.batch_scratch (0 with a block: the caller sized it by bamd_attention_batch_mfma_scratch, as before the slice plan existed).  While the
// score rows fit the LDS (ld * 8 <= BAMD_ATTN_LDS_MAX) and the block holds the whole micro-batch this is one launch; otherwise the attention is issued in token slices
// that reuse the block (bamd_attention_batch_plan with budget = scratch_bytes), *n_slices (optional) = how many
int  bamd_launch_attention_batch(const bamd_attn_args & a, int gq, int T, hipStream_t s, int impl = 0, size_t scratch_bytes = 0, int * n_slices = nullptr);     // 1 = shape not supported
// the same on the matrix cores (after the KV store); 1 = shape not covered.  t0 / Ts: the slice [t0, t0 + Ts) of the micro-batch's T tokens this launch covers
// (t0 a multiple of the kernel's token tile 16 / gq; Ts 0 = all of them); positions, q rows and out rows stay those of the whole micro-batch
int  bamd_launch_attention_batch_mfma(const bamd_attn_args & a, int gq, int T, hipStream_t s, int t0 = 0, int Ts = 0);
size_t bamd_attention_batch_mfma_scratch(int Hkv, int gq, int T, int ld);                         // bytes of a.batch_scratch it needs for sequences of up to ld positions (0: none)
void bamd_launch_attention_batch_gs(const bamd_attn_args & a, int gq, int t0, int Ts, hipStream_t s);   // the VALU kernel with its rows in a.batch_scratch (beyond the LDS; gq 1..8 checked by the caller)
int  bamd_attention_batch_mfma_on(void);                                                           // 0: switched off (BAMD_ATTN_MFMA=0)
// the slice plan of a micro-batch's attention: bamd_attention_batch_plan (include/bamd.h; defined in bamd_attention.hip, host code only)
void bamd_launch_sampler_shortlist(float * logits, const bamd_logit_penalty * pen, int n_pen, const uint8_t * halve_class, int halve,
                                   const float * cutoff_of, int V, bamd_shortlist_head * head, int32_t * ids, float * vals, int cap, hipStream_t s);
