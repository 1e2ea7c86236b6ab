/* bamd.h — C-ABI of libbooster_amd.so, level 1: the model-runtime calls that Booster's bridge makes.
 *
 * This is the layer the reference's cpp/bridge.cpp and cpp/janus.cpp call through cpp/include/llama.h
 * (SURVEY.md §8b "below the boundary"); every entry point names the llama.h function it replaces.  Plain C
 * types only: pointers are HOST pointers unless the name says `dev`.  All functions return 0 on success or a
 * non-zero error code unless documented otherwise; bamd_last_error() gives the message.  There is NO CPU
 * fallback: without a usable MI355X-class HIP device every compute entry point fails loudly.
 *
 * The nine cgo symbols of cpp/bridge.h are declared in booster_bridge.h and implemented on top of this.
 */
#ifndef BAMD_H
#define BAMD_H
#include <stdint.h>
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct bamd_model   bamd_model;
typedef struct bamd_context bamd_context;

/* ggml tensor type ids, as stored in GGUF (cpp/ggml/include/ggml.h:360-375) */
enum { BAMD_TYPE_F32 = 0, BAMD_TYPE_F16 = 1, BAMD_TYPE_Q2_K = 10, BAMD_TYPE_Q3_K = 11, BAMD_TYPE_Q4_K = 12, BAMD_TYPE_Q5_K = 13, BAMD_TYPE_Q6_K = 14, BAMD_TYPE_IQ4_NL = 20, BAMD_TYPE_IQ4_XS = 23, BAMD_TYPE_BF16 = 30 };

const char * bamd_last_error(void);

/* llama_backend_init (llama.h) / ggml_backend_cuda_get_device_count (ggml-cuda.h:30): number of HIP devices, <0 on error */
int bamd_backend_init(void);
int bamd_device_count(void);

/* llama_load_model_from_file (cpp/src/llama.cpp:16539).  Loads layers [layer_first, layer_last) of a GGUF Llama
 * model onto HIP device `device` (layer_last < 0: all).  with_embd / with_output say whether this stage owns the
 * token-embedding lookup and output_norm + lm_head (layer split: first / last stage — llama.cpp:5932-5969). */
bamd_model * bamd_model_load(const char * gguf_path, int device, int layer_first, int layer_last, int with_embd, int with_output);
void         bamd_model_free(bamd_model * m);                           /* llama_free_model */
int          bamd_model_n_vocab(const bamd_model * m);                  /* llama_n_vocab */
int          bamd_model_n_embd(const bamd_model * m);                   /* llama_n_embd */
int          bamd_model_n_layer(const bamd_model * m);                  /* llama_n_layer (whole model) */
int          bamd_model_n_ctx_train(const bamd_model * m);              /* llama_n_ctx_train */
int64_t      bamd_model_weight_bytes(const bamd_model * m);             /* bytes of matmul weights resident on this stage */
int64_t      bamd_model_prefill_aux_bytes(const bamd_model * m);        /* bytes of the prompt mat-muls' side tables built at load; 0 = none (prompts on the integer-dot kernel) */
/* copy back the GGUF-layout bytes of one resident tensor (testing / oracle cross-checks); returns bytes or <0 */
int64_t      bamd_model_tensor_raw(const bamd_model * m, const char * name, void * dst, int64_t cap);

/* llama_new_context_with_model (llama.cpp:16592): f16 KV cache for n_ctx positions, scratch, RoPE table. */
bamd_context * bamd_context_new(bamd_model * m, int n_ctx);
void           bamd_context_free(bamd_context * c);                     /* llama_free */
int            bamd_n_ctx(const bamd_context * c);                      /* llama_n_ctx */
void           bamd_kv_cache_clear(bamd_context * c);                   /* llama_kv_cache_clear (llama.cpp:3230) */

/* llama_decode(ctx, llama_batch_get_one(tokens, n_tokens, n_past, 0)) (llama.cpp:18517, :14537).
 * Processes the tokens at positions n_past.. with the reference's semantics for a micro-batch of n_tokens
 * (n_tokens > 1: attention scores use the f16-rounded q of the reference's T>1 path) and leaves the logits of
 * the LAST token for bamd_get_logits.  More than 512 tokens are evaluated in micro-batches of 512 (n_ubatch, llama.cpp:14615).
 * Returns 0, or 1 on failure like llama_decode. */
int           bamd_decode(bamd_context * c, const int32_t * tokens, int n_tokens, int n_past);
const float * bamd_get_logits(bamd_context * c);                        /* llama_get_logits: host, n_vocab floats */

/* Position edits of the KV cache, sequence 0 — llama_kv_cache_seq_rm / llama_kv_cache_seq_add (cpp/src/llama.cpp:3150-3217, :3268-3313),
 * the two calls of Booster's context shift (cpp/bridge.cpp:487-503):
 *     bamd_kv_seq_rm (ctx, n_keep, n_keep + n_discard);  bamd_kv_seq_add(ctx, n_keep + n_discard, n_past, -n_discard);  n_past -= n_discard;
 * Cells whose position leaves the sequence are freed and refilled in cell order (llama_kv_cache_find_slot, :3028-3127); the K rows of
 * moved cells are re-rotated by their delta before the next evaluation (K-shift: build_k_shift :8482-8512, ggml.c:14169-14290); the
 * attention then runs over cells and masks by the position each holds — all as the reference does, bit for bit.  While cells and
 * positions differ, tokens are evaluated one per bamd_decode / bamd_stage_step call (multi-token calls return an error) or by the device
 * loop bamd_generate_greedy, which runs find_slot for all its steps ahead on the host (it does not depend on the tokens); an edit that leaves cell i holding position i again (a plain truncation, seq_rm(n, -1)) ends that mode at once.  The calls wait
 * for the device to go idle first (hipDeviceSynchronize): work of this context still in flight on any stream is finished before the cell
 * metadata changes.
 * Negative p0 / p1 mean 0 / infinity as in llama.h.  Layer-split: call on every stage's context.  Return 0 on success. */
int bamd_kv_seq_rm(bamd_context * c, int p0, int p1);
int bamd_kv_seq_add(bamd_context * c, int p0, int p1, int delta);
/* llama_kv_cache_seq_div(ctx, 0, p0, p1, d) (llama.cpp:3315-3350): positions in [p0, p1) divided by d, the difference added to the pending
 * rotation — with bamd_kv_seq_add the three calls of Self-Extend (cpp/bridge.cpp:507-523; ga_n is fixed to 1 there, so Booster never issues them). */
int bamd_kv_seq_div(bamd_context * c, int p0, int p1, int d);

/* Greedy decode entirely on the device: n_steps single-token steps starting at position n_past; step 0 consumes
 * the arg-max of the logits left by the previous bamd_decode/bamd_generate_greedy call.  out_tokens receives
 * n_steps+1 ids: the token fed to each step, then the arg-max after the last step.  No host round trip between
 * steps: the steps are replayed as AQL packets with fence scope NONE from the library's own HSA queue (round 6; csrc/bamd_aql.h) where
 * the step's kernels allow it, else as one hipGraph per step on the context's stream (bamd_set_aql(0) / BAMD_AQL=0 forces that).
 * *elapsed_ms (optional) = time of the n_steps steps (HIP events; host clock from submission to completion on the own queue). */
int bamd_generate_greedy(bamd_context * c, int n_past, int n_steps, int32_t * out_tokens, float * elapsed_ms);
void bamd_set_aql(int on);                 /* process-wide: 1 (default, also env BAMD_AQL) = own AQL queue where possible; 0 = hipGraph replays */
int bamd_aql_runs(const bamd_context * c); /* bamd_generate_greedy calls + single-token bamd_decode steps of this context that ran on the own queue so far */
/* The own queue has no deadline for a run, only a stall limit: a run fails once the queue's read index has not moved for `ms` (default 60 000; ms <= 0
 * restores it; takes effect at the next run).  A queue that stays stuck for one more limit is not used again: every context replays its hipGraphs from then on. */
void bamd_set_aql_stall_ms(int ms);
/* Counters of `device`'s own queue (tests: which path a run took): out[0] packets written so far, out[1] replays that found the ring full at least once before
 * they were written, out[2] extra doorbells rung at the ring's last slot inside a replay, out[3] ring size in packets.  All 0 with BAMD_AQL=0 / no own queue. */
void bamd_aql_stats(int device, uint64_t out[4]);

/* ---- layer-split stage interface (one process per GPU; hidden state moves between stages) ---- */
/* Run this stage's layers on one token.  The token id comes from `token`, or — when token_dev is non-NULL — from that
 * device int32 (no host round trip; used on the first stage).  hidden_in_dev: f32 [n_embd] device pointer (ignored on
 * the first stage, which embeds the token); hidden_out_dev: f32 [n_embd] device pointer (ignored on the last stage,
 * which computes logits + arg-max instead).  Work is enqueued on `hip_stream` (a hipStream_t; NULL = the default
 * stream) and NOT synchronised.  prefill_mode as in bamd_decode (n_tokens > 1).  Returns 0 or an error code. */
int bamd_stage_step(bamd_context * c, int32_t token, const void * token_dev, int pos, const void * hidden_in_dev, void * hidden_out_dev,
                    int want_logits, int prefill_mode, void * hip_stream);
/* Batched counterpart of bamd_stage_step for prompt micro-batches of 2..512 tokens: `tokens` (host) on the stage that owns the
 * embedding, hidden_in_dev [n_tokens][n_embd] f32 on the others; writes hidden_out_dev [n_tokens][n_embd] on every stage but the
 * last, which computes the logits of the LAST token when want_logits (bamd_stage_get_logits).  Returns 2 when this model / context
 * shape has no batched kernels: the caller then falls back to bamd_stage_step per token.  Bit-identical to that path. */
int bamd_stage_prefill(bamd_context * c, const int32_t * tokens, int n_tokens, int n_past, const void * hidden_in_dev, void * hidden_out_dev,
                       int want_logits, void * hip_stream);
/* last stage: write the arg-max of the last bamd_stage_step(want_logits=1) into a device int32 (stream-ordered). */
int bamd_stage_token_to(bamd_context * c, void * token_dev, void * hip_stream);
/* host logits (n_vocab floats) of the last bamd_stage_step(want_logits=1) on the last stage; synchronises `hip_stream`. */
const float * bamd_stage_get_logits(bamd_context * c, void * hip_stream);
int bamd_model_device(const bamd_model * m);
/* arg-max token of the last bamd_stage_step(want_logits=1) on the last stage; synchronises `hip_stream`. */
int bamd_stage_argmax(bamd_context * c, void * hip_stream, int32_t * token);

/* ---- sampler prefilter on the device: the Janus penalties and shortlist where the lm_head left the logits ---- */
/* one distinct penalised token: logit = (float)(logit * pre) when pre != 0 (the EOS boost, janus.cpp:236), then `count` times
 * logit *= f (kind 0: float x float, janus.cpp:263) or logit = (float)(logit * d) (kind 1: float x double, janus.cpp:255) */
typedef struct { int32_t id, count, kind; float f; double d, pre; } bamd_logit_penalty;
typedef struct { unsigned long long top_key; int32_t count, ntop, nan, top_id; float top_logit, cutoff; } bamd_shortlist_head;
#define BAMD_SHORTLIST_CAP 1024
#define BAMD_PENALTY_CAP 512
/* per-vocabulary tables, uploaded once: halve_class[id] != 0 = token of a class the x0.5 pass hits (janus.cpp:269-283);
 * cutoff_of[id] = the shortlist cut-off when `id` is the top token (janus.cpp:303-306) */
int bamd_sampler_tables(bamd_context * c, const uint8_t * halve_class, const float * cutoff_of, int n_vocab);
/* Applies the penalties to the logits of the last decode / stage step IN PLACE on the device, then collects the candidates with
 * !(logit / top < cutoff_of[top]) (unordered) into ids / vals (up to BAMD_SHORTLIST_CAP) and fills *head: count (may exceed the cap),
 * ntop (logits equal to the top), nan, top_id, top_logit, cutoff.  Nothing is collected when top <= 0.  Runs on `hip_stream` —
 * pass bamd_context_stream(c) after bamd_decode, the stage's stream after bamd_stage_step — and synchronises it.  Returns 0 or 1. */
int bamd_logits_shortlist(bamd_context * c, const bamd_logit_penalty * pen, int n_pen, int halve, bamd_shortlist_head * head,
                          int32_t * ids, float * vals, void * hip_stream);
void * bamd_context_stream(bamd_context * c);
/* 0: bamd_decode leaves the logits on the device; bamd_get_logits then copies them on demand (default 1: copied by every decode) */
void bamd_set_logits_readback(bamd_context * c, int on);
/* waits for the context's stream and reports what a bamd_decode without read-back left unchecked (llama_synchronize, llama.cpp:18527-18551): for a caller
 * that evaluates and then does NOT sample (a request stopped during its prompt).  Returns 0 or 1. */
int bamd_synchronize(bamd_context * c);
/* test hook: overwrite the device logits (n_vocab floats) */
int bamd_set_logits_test(bamd_context * c, const float * logits);

/* ---- tokenizer of a GGUF, CPU only: llama_tokenize / llama_token_to_piece / llama_token_is_eog ---- */
typedef struct bamd_vocab bamd_vocab;
bamd_vocab * bamd_vocab_load(const char * gguf_path);                   /* llm_load_vocab, llama.cpp:5250 */
void bamd_vocab_free(bamd_vocab * v);
/* llama_tokenize (llama-vocab.cpp:1243); returns the token count (may exceed cap) */
int bamd_vocab_tokenize(const bamd_vocab * v, const char * text, int text_len, int add_special, int parse_special, int32_t * out, int cap);
/* llama_token_to_piece with special = true (llama-vocab.cpp:1539); returns bytes written, or -needed */
int bamd_vocab_piece(const bamd_vocab * v, int id, char * buf, int cap);
int bamd_vocab_n(const bamd_vocab * v);
int bamd_vocab_is_eog(const bamd_vocab * v, int id);                    /* llama_token_is_eog */
int bamd_vocab_eos(const bamd_vocab * v);
int bamd_vocab_eot(const bamd_vocab * v);

/* Test hook, CPU only: Booster's `gpus:` split (bridge.cpp:745-750 + llm_load_tensors, llama.cpp:5932-5969) — the device of every layer and,
 * at index n_layer, of the output layer, on a box with device_count GPUs.  Returns 1 when the setting is refused (it would need a CPU path). */
int bamd_plan_stages_test(int n_layer, int gpu1, int gpu2, int gpu3, int gpu4, int device_count, int32_t * device_of);

/* CPU only: open a GGUF (or the FIRST shard of a gguf-split model, llama.cpp:3659-3714) with the library's reader and report the tensor
 * count, the total tensor bytes and an FNV-1a digest over (name, type, shape, data) in name order.  Returns 0, or 1 with a message on stderr. */
int bamd_gguf_probe(const char * gguf_path, int64_t * n_tensors, int64_t * n_bytes, uint64_t * digest);

/* Test hook, CPU only: the candidate shortlist of the Janus sampler (janus.cpp:262-300 — full descending sort, cut at the first
 * candidate with logit / top < cutoff) through the linear-time path (fast = 1; falls back by itself when ties or a non-positive top
 * make the order depend on the full sort) or the full-sort path (fast = 0).  Writes up to `cap` ids in order, returns the count. */
int bamd_janus_shortlist_test(const float * logits, int n_vocab, float cutoff, int fast, int32_t * ids, int cap);
/* Test hooks, CPU only: the host Janus sampler on a vocabulary (initJanus, janus.cpp:410-700; sample_janus_token, janus.cpp:191-331;
 * llama_sample_token, llama-sampling.cpp:610-631).  _new builds the per-token type / scale tables; _sample applies the penalties to
 * `logits` (n_vocab floats) in place and draws with std::mt19937(seed); last = the most recent tokens, newest last. */
void * bamd_janus_test_new(const bamd_vocab * v, float scale, float hi, float lo, int depth);
void bamd_janus_test_tables(void * janus, float * types, float * scales);
int bamd_janus_test_sample(void * janus, float * logits, const int32_t * last, int n_last, int prompt_len, int pos, int max, uint32_t seed);
void bamd_janus_test_free(void * janus);
/* Test hook, GPU: one draw of a pod's sampler (ctx = what initContext returned) on scripted logits; device = 1 runs the penalties and
 * the shortlist on the device (bamd_logits_shortlist), 0 the host sampler.  logits_after / counts[2] (device draws, host-path draws)
 * may be NULL.  Returns the token, or -1. */
int bamd_bridge_sample_test(void * ctx, const float * logits, const int32_t * last, int n_last, int prompt_len, int pos, int max, uint32_t seed,
                            int device, float * logits_after, int64_t * counts);

/* Test hook: the stages initContext split a pod into (Booster's gpus: rule, BOOSTER_GPUS, BAMD_VIRTUAL_DEVICES): out[3 s .. 3 s + 2] = {device of the plan,
 * first layer, last layer + 1} for up to cap_stages stages; returns the number of stages. */
int bamd_bridge_stage_layout(void * ctx, int32_t * out, int cap_stages);

/* Prompt evaluation mode, process-wide: 1 (default, also env BAMD_PREFILL_BATCH) = bamd_decode with 2..512 tokens runs the batched
 * prefill kernels (every layer once per micro-batch, like llama_decode with n_tokens > 1); 0 = token by token through the decode
 * kernels.  Bit-identical results.  Micro-batches run batched at every position of the context: while two score rows of the padded sequence length fit the LDS
 * (18 432 positions) as they always did, beyond that with their score rows in the context's scratch block (bamd_set_attn_scratch_mb), in token slices that reuse
 * it.  Only where that block cannot be allocated do the micro-batches beyond 18 432 positions go token by token (bamd_stage_prefill returns 2 there).  After a
 * context shift tokens are evaluated one per call in either mode. */
void bamd_set_prefill_batch(int on);   /* 2 = batched, but the mat-muls on the integer-dot kernel instead of the matrix-core kernels (the path of a model whose
                                        * side tables did not fit: they are built at model load, all matrices or none, BAMD_PREFILL_AUX_RESERVE_GB of the device left free) */
/* Budget of a context's batched-attention scratch block in MiB, process-wide (also env BAMD_ATTN_SCRATCH_MB): the score rows of a prompt micro-batch beyond 512
 * positions live there (H x tokens x padded length x 4 bytes), and a micro-batch whose rows exceed the budget has its attention issued in token slices that reuse
 * the block (bamd_attention_batch_plan).  0 (default) = H x 512 x 18432 x 4 bytes (1.2 GB on the 8B shape): what a 512-token micro-batch at 18 432 positions
 * takes, so up to there a micro-batch is one slice.  A budget too small for one token tile sends micro-batches beyond 18 432 positions token by token.
 * Bit-identical results at every setting. */
void bamd_set_attn_scratch_mb(int mb);
/* The slice plan of a micro-batch's attention, host only (no device): T tokens, score rows of ld floats (a multiple of 64), impl as bamd_op_attention_batch,
 * budget_bytes for the scratch block (0 = the default above).  Slice i covers tokens [i * tokens_per_slice, min(T, (i + 1) * tokens_per_slice)); tokens_per_slice is
 * a whole number of the kernel's token tiles (16 / gq on the matrix cores, 1 on the VALU); scratch_bytes (<= budget) is what one slice needs (0: none).
 * Returns 1 when there is no plan: bad shape, impl 2 where the matrix-core kernel declines, or a budget below one tile. */
int bamd_attention_batch_plan(int Hkv, int gq, int hd, int T, int ld, int impl, size_t budget_bytes, int * tokens_per_slice, int * n_slices, size_t * scratch_bytes);
/* Matrix-core prompt mat-muls for Q3_K / Q2_K weights, process-wide: 0 (default, also env BAMD_PREFILL_LOWBIT) = a model that holds such a matrix builds
 * no side tables and evaluates its prompts on the integer-dot kernel; 1 = these types have side tables and kernels like Q4_K / Q5_K / Q6_K.  A model takes the
 * value at load (its tables exist or not); with the switch off again a model that has tables runs its prompts on the integer-dot kernel.  Bit-identical results. */
void bamd_set_prefill_lowbit(int on);
/* The same switch for Q8_0 / Q4_0 / Q5_0 weights (env BAMD_PREFILL_Q0): 0 (default) = a model that holds such a layer matrix builds no side tables and evaluates
 * its prompts on the integer-dot kernel; 1 = side tables (the rows' block scales as f32, 32 B per row and 256 weights) and a matrix-core kernel of their own.
 * Taken at model load, like bamd_set_prefill_lowbit.  Bit-identical results. */
void bamd_set_prefill_q0(int on);
/* And for Q4_1 / Q5_1 weights (env BAMD_PREFILL_Q1): 0 (default) = as above; 1 = side tables (the rows' block scales and minima as f32, 64 B per row and 256
 * weights) and a matrix-core kernel of their own.  Independent of bamd_set_prefill_q0.  Side tables are all-or-nothing per model: a Q4_0 / Q5_0 file made with
 * an importance matrix holds Q4_1 / Q5_1 ffn_down matrices and gets tables only with both switches on.  Taken at model load.  Bit-identical results. */
void bamd_set_prefill_q1(int on);
/* And for IQ4_NL weights (env BAMD_PREFILL_NL): 0 (default) = a model that holds such a layer matrix builds no side tables and evaluates its prompts on the
 * integer-dot kernel; 1 = side tables (the Q4_0 ones: the rows' block scales as f32, 32 B per row and 256 weights) and a matrix-core kernel of their own, with the
 * two accumulator sets of the type's chain.  Independent of the switches above: a model that also holds a Q8_0 / Q4_0 / Q5_0 or Q4_1 / Q5_1 layer matrix needs that
 * family's switch too (side tables are all-or-nothing per model); llama.cpp's IQ4_NL files hold IQ4_NL and K-quant matrices and need this one alone.  Taken at
 * model load.  Bit-identical results. */
void bamd_set_prefill_nl(int on);
/* Matrix-core prompt mat-muls for F32 / F16 weights (env BAMD_PREFILL_FLT): 0 (default) = such matrices evaluate prompts on the VALU kernel; 1 = on
 * v_mfma_f32_16x16x4_f32, the same fma chains.  UNLIKE the four switches above this one is read at each launch, not at model load: the kernel reads the resident
 * weights and the f32 activation rows as they are, there is no side table (bamd_model_prefill_aux_bytes stays 0 for such a model), so it takes effect for models and
 * contexts that exist already.  BF16 weights have a switch of their own (below).  Bit-identical results. */
void bamd_set_prefill_flt(int on);
/* Matrix-core prompt mat-muls for BF16 weights (env BAMD_PREFILL_BF16): 0 (default) = such matrices evaluate prompts on the VALU kernel; 1 = on
 * v_mfma_f32_16x16x4_f32.  A bf16 x bf16 product is exact in f32 unless it falls below 2^-149 or overflows, and there the reference's multiply-then-add is the
 * fma of the instruction; a workgroup whose exponent ranges (one word per matrix, computed at load; one per token, written by the activation pass) do not prove
 * that runs the two-rounding step on the vector ALUs inside the same launch.  Independent of bamd_set_prefill_flt; read at each launch like it, no side table,
 * and with it on a BF16 matrix no longer keeps a model's other types from their side tables.  Bit-identical results. */
void bamd_set_prefill_bf16(int on);
/* Tests and tools: workgroups of that kernel that took the two-rounding step since the library was loaded.  Waits for every device that launched one. */
unsigned long long bamd_prefill_bf16_fallback_tiles(void);
/* matrix-core prompt mat-mul launches of weight type `type` (GGUF type id: 0 F32, 1 F16, 2 Q4_0, 3 Q4_1, 6 Q5_0, 7 Q5_1, 8 Q8_0, 10 Q2_K .. 14 Q6_K, 20 IQ4_NL, 30 BF16; 23 IQ4_XS has no such kernel and stays 0) since the library was loaded */
long long bamd_prefill_mfma_runs(int type);

/* ---- measurement -------------------------------------------------------------------------------------- */
/* One eager single-token step at position `pos` with a HIP-event pair around every kernel launch.
 * classes: 0 matvec (all weight streaming), 1 attention (qk+softmax+pv), 2 step-begin/other.
 * For each class: launches[], ms[] (sum of durations), bytes[] (algorithmic bytes: weight records streamed /
 * KV bytes read).  Entry 3: ms[3] = what an EMPTY event pair reads on that stream (to subtract per launch).
 * Arrays must hold 4 entries. */
int bamd_profile_step(bamd_context * c, int pos, int * launches, double * ms, double * bytes);
/* the same per launch kind — arrays of 8: [0] fused QKV, [1] attention, [2] other, [3] wo, [4] gate/up, [5] ffn_down, [6] lm_head, [7] an empty event pair */
int bamd_profile_step_kinds(bamd_context * c, int pos, int * launches, double * ms, double * bytes);

/* Micro-benchmark: `iters` back-to-back launches of one mat-vec shape on random resident weights (pro: 0 plain,
 * 1 RMSNorm prologue; epi: 0 store, 1 +residual, 2 silu(gate)*up pair, 3 store+arg-max; mode as below). */
int bamd_bench_matvec(int type, int nrows, int k, int pro, int epi, int mode, int iters, float * us_per_launch);

/* ---- op-level entry points (parity tests call the kernels through these; host pointers in, host out) ---- */
/* quantize_row_q8_K (ggml-quants.c:3593) of norm_w ? rms_norm(x)*norm_w : x ; out = k/256 block_q8_K (292 B each) */
int bamd_op_quantize_q8_K(const float * x, int64_t k, const float * norm_w, float eps, void * out_blocks);
/* the same for the activation form of Q8_0 / Q4_0 / Q5_0 weights: k / 32 block_q8_0 {f16 d, i8 qs[32]}, 34 bytes each (quantize_row_q8_0) */
int bamd_op_quantize_q8_0(const float * x, int64_t k, const float * norm_w, float eps, void * out_blocks);
/* and of Q4_1 / Q5_1 weights: k / 32 block_q8_1 {f16 d, f16 s, i8 qs[32]}, 36 bytes each (quantize_row_q8_1) */
int bamd_op_quantize_q8_1(const float * x, int64_t k, const float * norm_w, float eps, void * out_blocks);
/* and of BF16 weights: k bf16 values, ggml_fp32_to_bf16_row of the (normed) vector.  F32 and F16 weights take the f32 vector as it is: the ops below accept the
   types 0 (F32), 1 (F16) and 30 (BF16) with w_raw row-major as in the GGUF file */
int bamd_op_act_bf16(const float * x, int64_t k, const float * norm_w, float eps, uint16_t * out_u16);
/* y[nrows] = W . Q8_K(act) (+ residual), W = GGUF-layout blocks [nrows][k] of `type`  (ggml_compute_forward_mul_mat, ggml.c:12277) */
int bamd_op_mul_mat_vec(int type, const void * w_raw, int nrows, int k, const float * x, const float * norm_w, float eps,
                        const float * residual, float * y, int mode /* 0 auto, 1 wave-per-row-group, 2 split-K */);
/* the lm_head launch with the greedy arg-max epilogue (BAMD_EPI_ARGMAX): y as bamd_op_mul_mat_vec without residual, *row = the row the
 * epilogue picks, which must be the lowest row of largest y (std::max_element).  mode 0: the launcher's choice; mode 16: the generic kernel */
int bamd_op_mul_mat_vec_argmax(int type, const void * w_raw, int nrows, int k, const float * x, const float * norm_w, float eps, float * y,
                               int mode, int32_t * row);
/* Y[T][nrows] = rows of W . Q8_K(act_t) (+ residual[T][nrows]) for T activation rows x[T][k] through the batched prefill kernels
 * (ggml_compute_forward_mul_mat with ne11 = T): impl 0 = integer-dot kernel (any K-quant), 1 = MFMA kernel (Q4_K, k % 1024 == 0) */
int bamd_op_mul_mat_batch(int type, const void * w_raw, int nrows, int k, const float * x, int T, const float * norm_w, float eps,
                          const float * residual, float * y, int impl);
/* y[nrows] = silu(Wg . a) * (Wu . a)  (llm_build_ffn LLM_FFN_SILU/LLM_FFN_PAR, llama.cpp:7960-8085) */
int bamd_op_ffn_gate_up(int type, const void * wg_raw, const void * wu_raw, int nrows, int k, const float * x, const float * norm_w,
                        float eps, float * y);
/* one row of a GGUF matrix dequantised (ggml_compute_forward_get_rows_q, ggml.c:13186) */
int bamd_op_get_row(int type, const void * w_raw, int nrows, int k, int row, float * y);
/* single-token attention of one layer (llm_build_kv, llama.cpp:8318): ropes q/k with the table row `pos`, stores
 * k/v (f16) into the caches, returns out[H*hd]; caches are host arrays in the reference's layouts and are updated. */
int bamd_op_attention(const float * q, const float * k, const float * v, uint16_t * k_cache, uint16_t * v_cache_t,
                      const float * rope_row, int H, int Hkv, int hd, int n_ctx, int pos, int prefill_mode, float * out,
                      float * probs_h0);
/* attention of a micro-batch of T tokens at positions pos0 .. pos0 + T - 1 (llm_build_kv with n_tokens = T, the reference's T > 1 semantics):
 * q [T][H*hd], k / v [T][Hkv*hd] before RoPE, rope [n_ctx][hd] the (cos,sin) table; the caches (host arrays in the reference's layouts) are updated,
 * out [T][H*hd].  impl: 0 = the launcher's choice (as the engine calls it), 1 = VALU kernels only, 2 = matrix-core kernel only (error where it
 * declines the shape).  ld: floats per LDS score row / scratch column, 0 = the engine's choice, else a multiple of 64 from the padded length of
 * the micro-batch's last position up to the padded n_ctx. */
int bamd_op_attention_batch(const float * q, const float * k, const float * v, uint16_t * k_cache, uint16_t * v_cache_t,
                            const float * rope, int H, int Hkv, int hd, int n_ctx, int pos0, int T, int impl, int ld, float * out);
/* the same with the scratch budget of the slice plan (scratch_bytes, 0 = the default) and, in *n_slices (optional), the number of attention launches issued behind
 * the KV store: a small budget forces several slices at a small shape.  ld may exceed 18 432 here and above: the rows then live in the scratch block. */
int bamd_op_attention_batch_ex(const float * q, const float * k, const float * v, uint16_t * k_cache, uint16_t * v_cache_t,
                               const float * rope, int H, int Hkv, int hd, int n_ctx, int pos0, int T, int impl, int ld, size_t scratch_bytes, float * out,
                               int * n_slices);
/* RoPE (cos,sin) table row as built on the host for position pos (ggml_rope_cache_init, ggml.c:14017) */
int bamd_op_rope_row(int pos, int n_dims, float freq_base, float freq_scale, const float * freq_factors, float * row);
/* the K-shift of one layer (llama_kv_cache_update -> build_k_shift, llama.cpp:15245-15277, :8482-8512) through the engine's own table code and launch:
 * every cell of k_cache [n_ctx][Hkv*hd] (host, reference layout, updated in place) re-rotated by delta[cell], with these rope parameters (beta_fast 32,
 * beta_slow 1, as the context's own table); cells with delta 0 included */
int bamd_op_k_shift(uint16_t * k_cache, int n_ctx, int Hkv, int hd, const int32_t * delta, float freq_base, float freq_scale, const float * freq_factors,
                    float ext_factor, float attn_factor, int n_ctx_orig);
/* single-token attention after position edits (bamd_kv_seq_add / _div): as bamd_op_attention, but the token's k / v go to cell `cell`, cellpos
 * [n_ctx] holds the position of every cell (-1 = free; the token's own entry is set to pos here), a cell is attended when it holds a position <= pos,
 * over the first n_kv cells; always the three-launch path with `tiles` score workgroups per KV head (0 = the engine's count).  probs_h0 (optional):
 * [n_kv] probabilities of query head 0 */
int bamd_op_attention_cells(const float * q, const float * k, const float * v, uint16_t * k_cache, uint16_t * v_cache_t, const float * rope_row,
                            const int32_t * cellpos, int cell, int n_kv, int H, int Hkv, int hd, int n_ctx, int pos, int tiles, float * out,
                            float * probs_h0);
/* the fused QKV launch of a decode step over up to three differently typed segments (types / w_raw / rows [nseg]: GGUF-layout blocks [rows[i]][k]), argument
 * block as the engine's: outputs one behind the other, RMSNorm prologue (norm_w required), store epilogue.  y [rows[0] + .. + rows[nseg - 1]].
 * mode: 0 the launcher's choice, 1 one wave per row-group, 2 split-K, + 16 generic kernels */
int bamd_op_fused_qkv(int nseg, const int32_t * types, const void * const * w_raw, const int32_t * rows, int k, const float * x, const float * norm_w,
                      float eps, int mode, float * y);
/* one batched prompt mat-mul as the engine issues it: T activation rows x [T][k] against up to three segments, into y [T][ldo] (in: what the untouched
 * columns keep; out: the result).  epi 0 (store): segment outputs one behind the other in each row; epi 1 (add): one segment, residual [T][ldo]; epi 2:
 * y = silu(seg 0 . a) * (seg 1 . a), both of rows[0] rows.  impl 0: integer-dot kernel; impl 2: every segment whose type has a matrix-core kernel runs
 * there, with a side table built as at model load, the others (Q2_K, Q3_K) stay on the integer-dot kernel — the routing of the engine's prompt path */
int bamd_op_mul_mat_batch_seg(int nseg, const int32_t * types, const void * const * w_raw, const int32_t * rows, int k, const float * x, int T,
                              const float * norm_w, float eps, int ldo, const float * residual, int epi, int impl, float * y);
/* attention and the wo projection of one decode layer in ONE launch (the co-launch of a decode step below 448 positions): the inputs of bamd_op_attention
 * (decode semantics), lds_ld = floats per LDS score row (0 = the engine's min(512, padded n_ctx)), the wo matrix [wo_rows][H * hd] of wo_type and the residual
 * [wo_rows].  serial, step and il go into the launch's tag (serial << 20 | (step & 0xfff) << 8 | il) as the step state and the layer index; with_cellpos != 0
 * passes a cell-position table (the launcher must decline); gran_init (NULL = zeros) is what the H * hd 8-byte granules {value bits, tag} hold before the
 * launch.  Out: x2 [wo_rows], the updated caches, gran_out [H * hd] as the launch left them, *gave_up = the give-up counter, *n_cu_used = the device's CU
 * count.  *declined = 1: the launcher has no co-launch kernel for the shape; nothing ran and the other outputs are untouched */
int bamd_op_attention_wo(const float * q, const float * k, const float * v, uint16_t * k_cache, uint16_t * v_cache_t, const float * rope_row, int H, int Hkv,
                         int hd, int n_ctx, int pos, int lds_ld, int wo_type, const void * wo_raw, int wo_rows, const float * residual, int serial, int step,
                         int il, int with_cellpos, const uint64_t * gran_init, float * x2, uint64_t * gran_out, uint32_t * gave_up, int32_t * declined,
                         int32_t * n_cu_used);

/* ---- launch-selection trace (host only: needs no device) ----
 * What the mat-vec launchers would launch for a shape, taken from their own recording path (the one the own-queue replay uses): nothing runs, no pointer is
 * dereferenced.  The argument blocks are filled as the engine's decode step fills them (rows padded to 8 per segment, nvalid = the real rows), with fixed
 * made-up addresses, so the hash of the packed kernel arguments pins every field a launcher sets (the row-group counts, the leading arguments, ...).
 * Return: 0 = one launch, described in *out; 1 = refused (a type without a kernel) / declined (no co-launch for the shape): nothing recorded; 2 = error */
typedef struct bamd_launch_trace {
    char kernel[1024];               /* mangled name of the kernel */
    uint32_t grid[3], block[3];
    uint32_t lds_bytes;              /* dynamic LDS */
    uint32_t kernarg_bytes;
    uint64_t kernarg_hash;           /* FNV-1a 64 of the packed explicit arguments */
} bamd_launch_trace;
/* bamd_launch_matvec: nseg (1..3) segments of types[i] / rows[i]; pro 0 plain, 1 RMSNorm; epi 0 store, 1 residual add, 2 silu(gate) * up (two segments, one
 * output), 3 arg-max; mode as bamd_op_fused_qkv */
int bamd_trace_matvec(int nseg, const int32_t * types, const int32_t * rows, int k, int pro, int epi, int mode, int n_cu, bamd_launch_trace * out);
/* the same through the dispatch the engine uses, which serves every family of weight types (the one above is the K-quant launcher alone) */
int bamd_trace_mv(int nseg, const int32_t * types, const int32_t * rows, int k, int pro, int epi, int mode, int n_cu, bamd_launch_trace * out);
/* bamd_launch_attn_wo: the attention block of a decode layer (n_ctx: padded; with_cellpos != 0: a cell-position table is set) and the wo launch behind it
 * (one segment [wo_rows][k], residual add, mode 0) */
int bamd_trace_attn_wo(int H, int Hkv, int hd, int n_ctx, int lds_ld, int with_cellpos, int wo_type, int wo_rows, int k, int n_cu, int il, bamd_launch_trace * out);

#ifdef __cplusplus
}
#endif
#endif
