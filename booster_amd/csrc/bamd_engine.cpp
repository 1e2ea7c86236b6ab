// bamd_engine.cpp — model runtime of libbooster_amd.so: GGUF -> HBM (wave-stream repack), KV cache, the fixed
// Llama decode pipeline as a static launch sequence / hipGraph, and the level-1 C-ABI of include/bamd.h.
//
// Replaces, for general.architecture = "llama" only, what the reference does in cpp/src/llama.cpp
// (llama_load_model_from_file :16539, llm_load_tensors :5899, llama_new_context_with_model :16592,
// llama_kv_cache_init :2926, build_llama :8781, llama_decode_internal :14537) and cpp/ggml/src/ggml-backend.c
// (graph split / scheduling) with one static pipeline: 6 kernels per layer, activations never leave HBM/LDS,
// the step's control state (position, KV length, token) lives on the device.
#include "../../include/bamd.h"
#include "bamd_formats.h"
#include "bamd_gguf.h"
#include "bamd_kernels.h"
#include "bamd_prefill_family.h"
#include "bamd_aql.h"
#include "bamd_engine_internal.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

thread_local std::string g_err;
// BAMD_PREFILL_BATCH=0: evaluate prompts token by token through the decode kernels instead of the batched kernels (same bits)
static int g_prefill_batch = [] { const char * e = getenv("BAMD_PREFILL_BATCH"); return (e && e[0] == '0') ? 0 : 1; }();
// BAMD_PREFILL_MFMA=0: Q4_K mat-muls of the batched prefill on the integer-dot kernel instead of the MFMA kernel (same bits)
static int g_prefill_mfma = [] { const char * e = getenv("BAMD_PREFILL_MFMA"); return (e && e[0] == '0') ? 0 : 1; }();
// The matrix-core kernels need a side table per matrix (bamd_prefill2.hip): built at MODEL LOAD, all matrices or none, against an explicit memory budget — after the
// weights are resident the tables (+ 78 % of the Q4_K / Q5_K bytes, + 63 % of the Q6_K bytes) must leave BAMD_PREFILL_AUX_RESERVE_GB (default 8) GiB of the device free,
// else the model runs its prompts on the integer-dot kernel (token by token where that has no instance).  BAMD_PREFILL_AUX=0 skips them (decode-only deployments).
// Which types have tables and kernels, and the switches of those that are off by default: bamd_prefill_family.h (bamd_prefill_mfma_type); a model takes their values at load.
static const int g_prefill_aux = [] { const char * e = getenv("BAMD_PREFILL_AUX"); return (e && e[0] == '0') ? 0 : 1; }();
// BAMD_STAGE_GRAPH=0: bamd_stage_step enqueues its kernels one by one instead of replaying a captured hipGraph
static const int g_stage_graph = [] { const char * e = getenv("BAMD_STAGE_GRAPH"); return (e && e[0] == '0') ? 0 : 1; }();
static int g_attn_scratch_mb = [] { const char * e = getenv("BAMD_ATTN_SCRATCH_MB"); const int v = e ? atoi(e) : 0; return v > 0 ? v : 0; }();   // budget of a context's batched-attention scratch block in MiB (bamd_set_attn_scratch_mb); 0 = the plan's default
static const bool g_attn_fused = [] { const char * e = getenv("BAMD_ATTN_FUSED"); return !(e && e[0] == '0'); }();   // default: fused single-launch attention (BAMD_ATTN_FUSED=0: three-kernel path)
// BAMD_AQL=0: the device-side greedy loop replays one hipGraph per step on the context's HIP stream (rounds 1-5) instead of AQL packets with fence scope
// NONE on the library's own queue (bamd_aql.h).  Same kernels, same bits; BAMD_AQL_VERBOSE=1 says why when the own queue is not used
static int g_aql = [] { const char * e = getenv("BAMD_AQL"); return (e && e[0] == '0') ? 0 : 1; }();
extern "C" __attribute__((visibility("default"))) void bamd_set_aql(int on) { g_aql = on ? 1 : 0; }
extern "C" __attribute__((visibility("default"))) void bamd_set_aql_stall_ms(int ms) { bamd_aql_set_stall_ms(ms); }
extern "C" __attribute__((visibility("default"))) void bamd_aql_stats(int device, uint64_t out[4]) { bamd_aql_get_stats(device, out); }

extern "C" __attribute__((visibility("default"))) const char * bamd_last_error(void) { return g_err.c_str(); }

// -------------------------------------------------------------------------------------------------------
// RoPE table on the host — ggml_rope_cache_init / rope_yarn / ggml_rope_yarn_corr_dims (ggml.c:13994-14041).
// cos/sin come from the host libm exactly like the reference's CPU path; the device only looks them up.
// -------------------------------------------------------------------------------------------------------
static float rope_yarn_ramp(const float low, const float high, const int i0) {
    const float y = (i0 / 2 - low) / fmaxf(0.001f, high - low);
    return 1 - fminf(1, fmaxf(0, y));
}
static float rope_corr_dim(int n_dims, int n_ctx_orig, float n_rot, float base) {
    return n_dims * logf(n_ctx_orig / (n_rot * 2 * (float) M_PI)) / (2 * logf(base));
}
void rope_row(float * cache, int32_t pos, int n_dims, float freq_base, float freq_scale, const float * freq_factors,
                     float ext_factor, float attn_factor, int n_ctx_orig, float beta_fast, float beta_slow) {
    const float theta_scale = powf(freq_base, -2.0f / n_dims);
    float corr_dims[2];
    {
        const float start = floorf(rope_corr_dim(n_dims, n_ctx_orig, beta_fast, freq_base));
        const float end = ceilf(rope_corr_dim(n_dims, n_ctx_orig, beta_slow, freq_base));
        corr_dims[0] = start > 0 ? start : 0;
        corr_dims[1] = end < n_dims - 1 ? end : n_dims - 1;
    }
    float theta = (float) pos;
    for (int i0 = 0; i0 < n_dims; i0 += 2) {
        const float ff = freq_factors ? freq_factors[i0 / 2] : 1.0f;
        const float theta_extrap = theta / ff;
        const float theta_interp = freq_scale * theta_extrap;
        float th = theta_interp, mscale = attn_factor;
        if (ext_factor != 0.0f) {
            const float ramp_mix = rope_yarn_ramp(corr_dims[0], corr_dims[1], i0) * ext_factor;
            th = theta_interp * (1 - ramp_mix) + theta_extrap * ramp_mix;
            mscale *= 1.0f + 0.1f * logf(1.0f / freq_scale);
        }
        cache[i0 + 0] = cosf(th) * mscale;
        cache[i0 + 1] = sinf(th) * mscale;
        theta *= theta_scale;
    }
}

// -------------------------------------------------------------------------------------------------------
struct DevMat {                      // one quantised matrix resident in HBM
    void * stream = nullptr;         // wave-stream records (matmul operand)
    void * raw = nullptr;            // GGUF layout (kept only for token_embd: row gather)
    int type = 0, nrows = 0, K = 0;  // nrows = rows in the GGUF
    int nrows_pad = 0;               // rows of the stream (next multiple of 8; missing rows are zero records)
    size_t bytes = 0;
    uint32_t bf16_range = BAMD_BF16_RANGE_UNKNOWN;   // BF16: the exponent range of its weights (bamd_bf16_range.h), measured once when the stream is packed
};
struct DevLayer {
    float * attn_norm = nullptr, * ffn_norm = nullptr;
    DevMat wq, wk, wv, wo, wg, wu, wd;
    // prefill side tables (bamd_prefill2.hip), built at model load (build_prefill_aux): one per QKV segment (qkv_segments), wo, gate, up, down
    void * aux_qkv[3] = { nullptr, nullptr, nullptr }, * aux_o = nullptr, * aux_g = nullptr, * aux_u = nullptr, * aux_d = nullptr;
};

struct bamd_model {
    int device = 0;
    int E = 0, H = 0, Hkv = 0, hd = 0, L = 0, F = 0, V = 0, n_ctx_train = 0, n_rot = 0;
    float eps = 1e-5f, rope_theta = 10000.f, rope_freq_scale = 1.f, rope_ext_factor = 0.f, rope_attn_factor = 1.f;
    int rope_n_ctx_orig = 0;
    int layer_first = 0, layer_last = 0;
    bool with_embd = true, with_output = true;
    std::vector<float> rope_freqs;   // host copy (optional)
    std::vector<DevLayer> layers;    // [layer_last - layer_first]
    DevMat tok_embd, output;
    float * out_norm = nullptr;
    int64_t weight_bytes = 0;
    int n_cu = 256;
    std::unique_ptr<GgufFile> file;  // stays mapped (bamd_model_tensor_raw)
    std::vector<void *> allocs;
    bool aux_ok = false, aux_none_needed = false; int64_t aux_bytes = 0; std::string aux_why;      // prefill side tables: all matrices or none (build_prefill_aux)
};

// ---- one cached replay of "the fixed launch sequence of one step", rebuilt when, and only when, the key of the step at hand differs from the one it was built for.
// The key is everything a sequence is recorded with: which attention kernels it holds (attn_path) and, for the stage graphs, the pointers it was captured with
enum AttnPath { ATTN_SPLIT = 0, ATTN_SINGLE = 1, ATTN_CELLS = 2 };   // scores | softmax | P.V;  single-launch kernel;  the split path's shifted-cell kernels (+ slot table)
struct ReplayKey {
    AttnPath path = ATTN_SPLIT;
    const void * token_src = nullptr, * hin = nullptr, * hout = nullptr;        // stage graphs only
    bool operator==(const ReplayKey & o) const { return path == o.path && token_src == o.token_src && hin == o.hin && hout == o.hout; }
};
struct StepReplay {                  // EITHER a hipGraph (capture_graph) OR packets for the library's own queue (record_aql), and the key it was built for
    hipGraphExec_t exec = nullptr; bamd_aql_graph * aql = nullptr; ReplayKey key;
    void reset() { if (exec) hipGraphExecDestroy(exec); if (aql) bamd_aql_free(aql); exec = nullptr; aql = nullptr; }
    void reset_unless(const ReplayKey & k) { if (!(key == k)) reset(); }
};

struct bamd_context {
    bamd_model * m = nullptr;
    int n_ctx = 0;
    std::vector<unsigned short *> kc, vc;
    float * rope = nullptr, * rope_cur = nullptr;   // rope_cur [hd]: the cos / sin row of the current step's position (step_begin_kernel -> attn_qk_kernel)
    float * x = nullptr, * x2 = nullptr, * q = nullptr, * k = nullptr, * v = nullptr, * att = nullptr, * h = nullptr, * scores = nullptr, * probs = nullptr;
    int n_ctx_pad = 0;              // KV row stride: n_ctx rounded up to 64 (V^T rows are stored in 64-position blocks)
    float * logits = nullptr;        // device
    float * logits_host = nullptr;   // pinned
    bool logits_readback = true, logits_host_valid = false;
    bool status_pending = false;     // a bamd_decode without read-back returned before its stream was waited for: the next synchronising call checks the give-up words
    // sampler prefilter (bamd_logits_shortlist): per-vocabulary tables, penalty list and result (device + pinned mirrors)
    uint8_t * samp_cls = nullptr; float * samp_cut = nullptr;
    bamd_logit_penalty * samp_pen = nullptr, * samp_pen_host = nullptr;
    unsigned char * samp_out = nullptr, * samp_out_host = nullptr;
    bamd_step_state * st = nullptr;
    int32_t * forced = nullptr; int forced_cap = 0;
    int32_t * out_tokens = nullptr; int out_cap = 0;
    hipStream_t stream = nullptr;
    // every replay of this context: the greedy loop's step as a hipGraph and as packets for the own queue, bamd_stage_step's single host-fed token on the own queue, its stage graphs [want_logits][prefill_mode]
    StepReplay greedy_graph, greedy_aql, step_aql, stage_graph[2][2];
    bool aql_failed = false;                     // sticky: a recording of this context could not be turned into packets, both own-queue users stay on their hipGraphs
    int aql_runs = 0, aql_steps = 0;             // bamd_generate_greedy calls / single-token steps that ran on the own queue (bamd_aql_runs)
    bamd_step_state * inbox = nullptr;           // pinned host memory: the state of that step, read by step_begin_kernel itself (no copy in front of the step)
    unsigned long long * co_gran = nullptr;   // co-launch granules [H * hd] {value, tag} + give-up counter behind them (bamd_colaunch.hip), zero-initialised
    uint32_t * co_err = nullptr;
    int32_t * slots = nullptr; int slots_cap = 0;   // device-side greedy loop after a context shift: {cell, padded KV length} of every step (bamd_generate_greedy)
    int host_serial = 0;             // host calls that set the device state so far (bamd_step_state.serial)
    // KV cell metadata (llama_kv_cache cells: pos / delta / head / used, llama.cpp:2700-2760) — inactive (cell i holds position i, nothing to
    // track) until the first bamd_kv_seq_rm / bamd_kv_seq_add
    struct Cells { bool active = false, has_shift = false; std::vector<int32_t> pos, delta; int head = 0, used = 0; } cells;
    int n_cached = 0;               // positions evaluated so far (highest n_past + n_tokens seen): what the cells hold when tracking starts
    int32_t * cellpos = nullptr;    // device copy of cells.pos (attention mask of the shifted path)
    int32_t * shift_idx = nullptr; float * shift_tab = nullptr; int shift_tab_cap = 0;
    // phase-stamp blocks (bamd_timeline_step, BAMD_TIMING builds): one block of BAMD_TL_SLOT_WORDS u64 per launch
    unsigned long long * tl_base = nullptr; int tl_slot = 0, tl_cap = 0;
    // batched prefill buffers, [bcap] tokens each (allocated at the first multi-token decode)
    int bcap = 0;
    float * attn_bscr = nullptr; size_t attn_bscr_bytes = 0, attn_bscr_failed = 0;   // score rows of the batched prefill attention: the matrix-core kernel beyond BAMD_AM_MAXPOS = 512 positions, every kernel beyond the LDS (ensure_attn_scratch: grow-only under the budget; absent = the VALU kernels with their rows in LDS, token by token beyond)
    float * bx = nullptr, * bx2 = nullptr, * bqkv = nullptr, * batt = nullptr, * bh = nullptr; unsigned char * bblob = nullptr, * bblob16 = nullptr;
    uint32_t * bbfr = nullptr;      // beside bblob: one range word per token of its bf16 rows (bamd_bf16_range.h)
    std::vector<void *> allocs;
};

static int dev_alloc(std::vector<void *> & keep, void ** p, size_t bytes) {
    HIPC(hipMalloc(p, bytes + 4096));           // + 4 KiB: the sixteen-wave prefill kernel's nibble loads of the two super-blocks behind the end of K run past
                                                // the last record group (bamd_prefill2.hip)
    keep.push_back(*p);
    return 0;
}

extern "C" __attribute__((visibility("default"))) int bamd_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { g_err = "hipGetDeviceCount failed (no HIP device?)"; return -1; }
    return n;
}
extern "C" __attribute__((visibility("default"))) int bamd_backend_init(void) { return bamd_device_count(); }

// upload one matrix: raw bytes -> (optional raw copy) + wave-stream repack on the device
static int upload_mat(bamd_model * m, const GgufTensor * t, DevMat & d, bool keep_raw, bool want_stream, void * staging, hipStream_t s,
                      void * stream_dst = nullptr) {
    if (t->ne.size() != 2) return fail("tensor " + t->name + ": expected 2 dims");
    d.type = t->type; d.K = (int) t->ne[0]; d.nrows = (int) t->ne[1]; d.bytes = t->nbytes;
    if (!bamd_has_record(d.type)) return fail("tensor " + t->name + ": type " + std::to_string(d.type) + " not supported (F32, F16, BF16, Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q2_K, Q3_K, Q4_K, Q5_K, Q6_K, IQ4_NL, IQ4_XS)");
    if (bamd_has_record(d.type) && d.K % 256) return fail("tensor " + t->name + ": row length not a multiple of 256");
    if (want_stream) {
        if (d.K % 256) return fail("tensor " + t->name + ": row length not a multiple of 256");
        // an unquantised matrix keeps its whole activation vector in the LDS of a CU (bamd_matvec_flt.hip): refused here, not at the first launch
        if (bamd_is_flt(d.type) && d.K > bamd_flt_max_k(d.type))
            return fail("tensor " + t->name + ": row length " + std::to_string(d.K) + " is beyond what the F32 / F16 / BF16 mat-vec kernels hold in LDS (" + std::to_string(bamd_flt_max_k(d.type)) + " for this type)");
    }
    d.nrows_pad = (d.nrows + 7) / 8 * 8;
    if (d.nrows_pad != d.nrows && stream_dst) return fail("tensor " + t->name + ": fused QKV needs row counts that are multiples of 8");
    void * rawdev = staging;
    if (keep_raw) { if (dev_alloc(m->allocs, &d.raw, t->nbytes)) return 1; rawdev = d.raw; }
    HIPC(hipMemcpyAsync(rawdev, t->data, t->nbytes, hipMemcpyHostToDevice, s));
    if (want_stream) {
        const size_t stream_bytes = bamd_stream_bytes(d.type, d.K, d.nrows_pad);
        if (stream_bytes >= (size_t) 0x7fffffff) return fail("tensor " + t->name + ": wave-stream copy exceeds 2 GiB (32-bit record offsets)");
        if (stream_dst) d.stream = stream_dst;
        else { if (dev_alloc(m->allocs, &d.stream, stream_bytes)) return 1; if (d.nrows_pad != d.nrows) HIPC(hipMemsetAsync(d.stream, 0, stream_bytes, s)); }
        bamd_launch_repack(rawdev, d.stream, d.type, d.nrows, d.K, s);
        HIPC(hipGetLastError());
        if (d.type == BAMD_BF16 && bamd_bf16_weight_range(d.stream, stream_bytes, &d.bf16_range, s)) return fail("tensor " + t->name + ": measuring the exponent range failed");
        m->weight_bytes += (int64_t) t->nbytes;
    }
    HIPC(hipStreamSynchronize(s));     // staging buffer is reused by the next tensor
    return 0;
}
static int upload_f32(bamd_model * m, const GgufTensor * t, float ** p, int n, hipStream_t s) {
    if (!t) return fail("missing norm tensor");
    if (t->type != BAMD_F32 || (int) t->ne[0] != n) return fail("tensor " + t->name + ": expected f32[" + std::to_string(n) + "]");
    if (dev_alloc(m->allocs, (void **) p, (size_t) n * 4)) return 1;
    HIPC(hipMemcpyAsync(*p, t->data, (size_t) n * 4, hipMemcpyHostToDevice, s));
    return 0;
}

static void build_prefill_aux(bamd_model * m, hipStream_t s);
// The ONE attn_q | attn_k | attn_v whose matrices need two activation forms and that loads: the pair llama.cpp's IQ4_NL recipe writes.  llama_tensor_get_type
// (src/llama.cpp:15544-15546) makes attn_v Q5_K wherever n_gqa >= 4 (Llama-3, Mistral, the 8B shape) while attn_q and attn_k stay IQ4_NL: Q8_0 activations
// for the first two, Q8_K for the third.  The engine runs such a layer's QKV as one launch per form (qkv_groups); every other mix stays refused at load.
// (bamd_is_kquant holds IQ4_XS too, so an IQ4_XS attn_v beside IQ4_NL attn_q / attn_k passes here as well: no recipe writes it and no test covers it; it takes the
// same two launches, the second on the generic Q8_K kernel)
static bool qkv_recipe_mix(int tq, int tk, int tv) { return tq == BAMD_IQ4_NL && tk == BAMD_IQ4_NL && bamd_is_kquant(tv); }
static int model_load_impl(bamd_model * m, const char * path, int device, int lf, int ll, int with_embd, int with_output) {
    // the file is read and its header validated before any device is touched: a bad file is reported as such on any machine
    m->file.reset(new GgufFile());
    std::string err;
    if (!m->file->open(path, err)) return fail(err);
    GgufFile & g = *m->file;
    std::string arch;
    if (!g.get_str("general.architecture", arch) || arch != "llama") return fail("general.architecture must be \"llama\" (got \"" + arch + "\")");
    uint32_t u;
    if (!g.get_u32("llama.embedding_length", u)) return fail("missing llama.embedding_length"); m->E = (int) u;
    if (!g.get_u32("llama.block_count", u)) return fail("missing llama.block_count"); m->L = (int) u;
    if (!g.get_u32("llama.feed_forward_length", u)) return fail("missing llama.feed_forward_length"); m->F = (int) u;
    if (!g.get_u32("llama.attention.head_count", u)) return fail("missing llama.attention.head_count"); m->H = (int) u;
    m->Hkv = m->H; if (g.get_u32("llama.attention.head_count_kv", u)) m->Hkv = (int) u;
    if (!g.get_f32("llama.attention.layer_norm_rms_epsilon", m->eps)) return fail("missing llama.attention.layer_norm_rms_epsilon");
    m->n_ctx_train = 2048; if (g.get_u32("llama.context_length", u)) m->n_ctx_train = (int) u;
    if (m->E <= 0 || m->L <= 0 || m->F <= 0 || m->H <= 0 || m->Hkv <= 0) return fail("embedding_length, block_count, feed_forward_length and head counts must be positive");
    if (m->E % m->H) return fail("llama.embedding_length is not a multiple of llama.attention.head_count");
    m->hd = m->E / m->H;
    m->n_rot = m->hd; if (g.get_u32("llama.rope.dimension_count", u)) m->n_rot = (int) u;
    if (m->n_rot != m->hd) return fail("llama.rope.dimension_count != n_embd/n_head is not supported");
    g.get_f32("llama.rope.freq_base", m->rope_theta);
    {   // RoPE scaling as llm_load_hparams reads it (llama.cpp:4630-4650): the type defaults to "linear" when the key is absent, the
        // factor comes from rope.scaling.factor or the legacy rope.scale_linear, freq_scale = 1 / factor; a "none" type never scales
        // (llama_new_context_with_model, llama.cpp:16682-16684).  YaRN: ext_factor = 1 (:16686-16688), the magnitude factor is
        // rope.scaling.attn_factor for every type (:16690), the correction range comes from rope.scaling.original_context_length
        // (default: the training context; :4630-4631, :16670-16672) with beta_fast 32 / beta_slow 1 (:16441-16442).
        std::string st = "linear"; float factor = 0.f;
        g.get_str("llama.rope.scaling.type", st);
        if (st != "none" && st != "linear" && st != "yarn") return fail("rope scaling type \"" + st + "\" not supported");
        if (!g.get_f32("llama.rope.scaling.factor", factor)) g.get_f32("llama.rope.scale_linear", factor);
        m->rope_freq_scale = (factor == 0.f || st == "none") ? 1.0f : 1.0f / factor;
        m->rope_ext_factor = st == "yarn" ? 1.0f : 0.0f;
        m->rope_attn_factor = 1.0f; g.get_f32("llama.rope.scaling.attn_factor", m->rope_attn_factor);
        m->rope_n_ctx_orig = m->n_ctx_train;
        if (g.get_u32("llama.rope.scaling.original_context_length", u) && u != 0) m->rope_n_ctx_orig = (int) u;
    }
    if (m->H % m->Hkv) return fail("n_head % n_head_kv != 0");
    const int gq = m->H / m->Hkv;
    if (gq < 1 || gq > 8) return fail("GQA ratio (heads per KV head) must be 1 .. 8");
    if (m->hd % 64 || m->hd > 256) return fail("head dim must be 64, 128, 192 or 256");
    if (m->E % 256 || m->F % 256)
        return fail(m->E % 32 || m->F % 32 ? "n_embd and n_ff must be multiples of 256"
                                           : "n_embd and n_ff must be multiples of 256 (n_embd " + std::to_string(m->E) + ", n_ff " + std::to_string(m->F) +
                                             ": a row length that is a multiple of 32 but not of 256 is a valid Q4_0 / Q4_1 / Q5_0 / Q5_1 / Q8_0 tensor (or IQ4_NL one), but a wave-stream record holds 256 weights per row)");
    if (m->E > 32768 || m->F > 131072) return fail("n_embd / n_ff beyond what the kernels' LDS budgets were sized for");
    if (ll < 0 || ll > m->L) ll = m->L;
    if (lf < 0 || lf > ll) return fail("bad layer range");
    m->layer_first = lf; m->layer_last = ll; m->with_embd = with_embd != 0; m->with_output = with_output != 0;

    const GgufTensor * te = g.tensor("token_embd.weight");
    if (!te) return fail("missing token_embd.weight");
    if (te->ne.size() != 2 || (int) te->ne[0] != m->E) return fail("token_embd.weight: row length != llama.embedding_length");
    m->V = (int) te->ne[1];
    if (m->V <= 0) return fail("token_embd.weight: empty vocabulary");
    if (const GgufTensor * rf = g.tensor("rope_freqs.weight")) {
        if (rf->type != BAMD_F32 || (int) rf->ne[0] < m->hd / 2) return fail("bad rope_freqs.weight");
        m->rope_freqs.assign((const float *) rf->data, (const float *) rf->data + m->hd / 2);
    }
    const int ndev = bamd_device_count();
    if (ndev <= 0) return fail("no HIP device available: libbooster_amd has no CPU fallback");
    if (device < 0 || device >= ndev) return fail("bad device index");
    HIPC(hipSetDevice(device));
    m->device = device;
    { hipDeviceProp_t p; HIPC(hipGetDeviceProperties(&p, device)); m->n_cu = p.multiProcessorCount > 0 ? p.multiProcessorCount : 256; }
    hipStream_t s; HIPC(hipStreamCreate(&s));
    size_t stage_bytes = 0;
    for (auto & t : g.tensors) stage_bytes = std::max(stage_bytes, t.nbytes);
    void * staging = nullptr;
    { const hipError_t e = hipMalloc(&staging, stage_bytes ? stage_bytes : 16); if (e != hipSuccess) { hipStreamDestroy(s); return fail(std::string("staging buffer: ") + hipGetErrorString(e)); } }
    int rc = 0;
    do {
        if (m->with_embd) { if ((rc = upload_mat(m, te, m->tok_embd, true, false, staging, s))) break; }
        if (m->with_output) {
            if ((rc = upload_f32(m, g.tensor("output_norm.weight"), &m->out_norm, m->E, s))) break;
            const GgufTensor * to = g.tensor("output.weight");
            if (!to) to = te;                                              // tied embeddings, llama.cpp:6070-6076
            if ((rc = upload_mat(m, to, m->output, false, true, staging, s))) break;
            if (m->output.K != m->E) { rc = fail("output.weight: row length != llama.embedding_length"); break; }
        }
        m->layers.resize((size_t) (ll - lf));
        for (int il = lf; il < ll && !rc; ++il) {
            DevLayer & ly = m->layers[(size_t) (il - lf)];
            const std::string p = "blk." + std::to_string(il) + ".";
            if ((rc = upload_f32(m, g.tensor(p + "attn_norm.weight"), &ly.attn_norm, m->E, s))) break;
            if ((rc = upload_f32(m, g.tensor(p + "ffn_norm.weight"), &ly.ffn_norm, m->E, s))) break;
            struct { const char * n; DevMat * d; } mats[] = { { "attn_q", &ly.wq }, { "attn_k", &ly.wk }, { "attn_v", &ly.wv }, { "attn_output", &ly.wo },
                                                              { "ffn_gate", &ly.wg }, { "ffn_up", &ly.wu }, { "ffn_down", &ly.wd } };
            // wq | wk | wv share one allocation so that equal-typed neighbours form ONE weight stream (fused QKV mat-vec)
            char * qkv_base = nullptr; size_t qkv_off = 0;
            {
                size_t tot = 0;
                for (int j = 0; j < 3; ++j) {
                    const GgufTensor * t = g.tensor(p + mats[j].n + ".weight");
                    if (t && t->ne.size() == 2 && bamd_has_record(t->type)) tot += bamd_stream_bytes(t->type, t->ne[0], ((int64_t) t->ne[1] + 7) / 8 * 8);
                }
                if (dev_alloc(m->allocs, (void **) &qkv_base, tot)) { rc = 1; break; }
            }
            int mi = 0;
            for (auto & mm : mats) {
                const GgufTensor * t = g.tensor(p + mm.n + ".weight");
                if (!t) { rc = fail("missing tensor " + p + mm.n + ".weight"); break; }
                void * dst = nullptr;
                if (mi < 3) { dst = qkv_base + qkv_off; if (t->ne.size() == 2 && bamd_has_record(t->type)) qkv_off += bamd_stream_bytes(t->type, t->ne[0], ((int64_t) t->ne[1] + 7) / 8 * 8); }
                if ((rc = upload_mat(m, t, *mm.d, false, true, staging, s, dst))) break;
                ++mi;
            }
            if (rc) break;
            if (ly.wq.nrows != m->E || ly.wq.K != m->E || ly.wk.nrows != m->Hkv * m->hd || ly.wk.K != m->E || ly.wv.nrows != m->Hkv * m->hd || ly.wv.K != m->E ||
                ly.wo.nrows != m->E || ly.wo.K != m->E || ly.wg.nrows != m->F || ly.wg.K != m->E || ly.wu.nrows != m->F || ly.wu.K != m->E ||
                ly.wd.nrows != m->E || ly.wd.K != m->F) { rc = fail("layer " + std::to_string(il) + ": unexpected tensor shapes"); break; }
            if (ly.wg.type != ly.wu.type) { rc = fail("ffn_gate and ffn_up must share one quantisation type"); break; }
            // the fused QKV launch quantises its activations ONCE: Q8_K for K-quant segments, Q8_0 for Q4_0 / Q5_0 / Q8_0 ones, Q8_1 for Q4_1 / Q5_1 ones
            // (bamd_act_form_of).  No llama.cpp recipe mixes the
            // families inside attn_q | attn_k | attn_v; a file that does is refused here rather than run with the wrong form.  The one exception is the pair
            // qkv_recipe_mix names, which the decode step and the batched prompt path run as one launch per form (qkv_groups).  IQ4_NL beside Q8_0 / Q4_0 / Q5_0
            // (one form, but no recipe writes it either) is refused in the same words: what loads is what a recipe writes
            for (int j = 1; j < 3 && !rc && !qkv_recipe_mix(ly.wq.type, ly.wk.type, ly.wv.type); ++j)
                if (bamd_act_form_of(mats[j].d->type) != bamd_act_form_of(mats[0].d->type) || (mats[j].d->type == BAMD_IQ4_NL) != (mats[0].d->type == BAMD_IQ4_NL))
                    rc = fail(p + mats[0].n + ".weight (type " + std::to_string(mats[0].d->type) + ") and " + p + mats[j].n + ".weight (type " + std::to_string(mats[j].d->type) +
                              ") need different activation formats (" + (bamd_is_flt(mats[0].d->type) || bamd_is_flt(mats[j].d->type) ? "Q8_K / Q8_0 / Q8_1 / F32 / BF16" : bamd_is_q1(mats[0].d->type) || bamd_is_q1(mats[j].d->type) ? "Q8_K / Q8_0 / Q8_1" : "Q8_K / Q8_0") + ") in one fused launch: not supported");
            if (rc) break;
        }
    } while (0);
    hipStreamSynchronize(s);
    hipFree(staging);
    if (!rc) {
        build_prefill_aux(m, s);
        if (!m->aux_ok && !m->aux_none_needed && getenv("BAMD_PREFILL_VERBOSE")) fprintf(stderr, "bamd: prompts run without the matrix-core kernels: %s\n", m->aux_why.c_str());
    }
    hipStreamDestroy(s);
    return rc;
}

extern "C" __attribute__((visibility("default"))) bamd_model * bamd_model_load(const char * path, int device, int layer_first, int layer_last, int with_embd, int with_output) {
    bamd_model * m = new bamd_model();
    int rc = 1;
    try { rc = model_load_impl(m, path, device, layer_first, layer_last, with_embd, with_output); }
    catch (const std::exception & e) { g_err = std::string("model load: ") + e.what(); rc = 1; }     // nothing may unwind through the C boundary
    if (rc) { bamd_model_free(m); return nullptr; }
    return m;
}
extern "C" __attribute__((visibility("default"))) void bamd_model_free(bamd_model * m) {
    if (!m) return;
    hipSetDevice(m->device);
    for (void * p : m->allocs) hipFree(p);
    delete m;
}
extern "C" __attribute__((visibility("default"))) int bamd_model_n_vocab(const bamd_model * m) { return m->V; }
extern "C" __attribute__((visibility("default"))) int64_t bamd_model_prefill_aux_bytes(const bamd_model * m) { return m->aux_ok ? m->aux_bytes : 0; }
extern "C" __attribute__((visibility("default"))) int bamd_model_n_embd(const bamd_model * m) { return m->E; }
extern "C" __attribute__((visibility("default"))) int bamd_model_n_layer(const bamd_model * m) { return m->L; }
extern "C" __attribute__((visibility("default"))) int bamd_model_n_ctx_train(const bamd_model * m) { return m->n_ctx_train; }
extern "C" __attribute__((visibility("default"))) int64_t bamd_model_weight_bytes(const bamd_model * m) { return m->weight_bytes; }
extern "C" __attribute__((visibility("default"))) int64_t bamd_model_tensor_raw(const bamd_model * m, const char * name, void * dst, int64_t cap) {
    const GgufTensor * t = m->file->tensor(name);
    if (!t) { g_err = std::string("no tensor ") + name; return -1; }
    if ((int64_t) t->nbytes > cap) return (int64_t) t->nbytes;
    memcpy(dst, t->data, t->nbytes);
    return (int64_t) t->nbytes;
}

// -------------------------------------------------------------------------------------------------------
static int context_init(bamd_context * c, bamd_model * m, int n_ctx) {
    HIPC(hipSetDevice(m->device));
    c->m = m; c->n_ctx = n_ctx;
    if (n_ctx < 32 || n_ctx % 32) return fail("n_ctx must be a positive multiple of 32");
    // the attention kernels read one layer's K / V^T through 32-bit byte offsets into a 2 GiB - 1 window (ik_rsrc, bamd_device.h): a larger cache would read zeros
    // past the window, silently.  Checked before anything is allocated
    if ((size_t) ((n_ctx + 63) / 64 * 64) * (size_t) (m->Hkv * m->hd) * 2 >= (size_t) 0x7fffffff) {
        char b[256]; snprintf(b, sizeof b, "n_ctx %d x %d KV elements per position x 2 bytes = %.2f GiB per layer cache: one layer's K (or V) cache must stay below 2 GiB (32-bit offsets in the attention kernels); open the context with a smaller n_ctx",
                              n_ctx, m->Hkv * m->hd, (double) ((size_t) ((n_ctx + 63) / 64 * 64) * (size_t) (m->Hkv * m->hd) * 2) / 1073741824.0);
        return fail(b);
    }
    HIPC(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    const int nl = (int) m->layers.size(), Ekv = m->Hkv * m->hd;
    c->kc.resize((size_t) nl); c->vc.resize((size_t) nl);
    c->n_ctx_pad = (n_ctx + 63) / 64 * 64;
    const size_t kvb = (size_t) c->n_ctx_pad * Ekv * 2;
    for (int i = 0; i < nl; ++i) {                                   // llama_kv_cache_init :2926-3026 — zero-initialised
        if (dev_alloc(c->allocs, (void **) &c->kc[(size_t) i], kvb) || dev_alloc(c->allocs, (void **) &c->vc[(size_t) i], kvb)) return 1;
        HIPC(hipMemsetAsync(c->kc[(size_t) i], 0, kvb, c->stream)); HIPC(hipMemsetAsync(c->vc[(size_t) i], 0, kvb, c->stream));
    }
    {   // RoPE table for every position (host libm, like the reference), uploaded once
        std::vector<float> tab((size_t) n_ctx * m->hd);
        for (int p = 0; p < n_ctx; ++p)
            rope_row(tab.data() + (size_t) p * m->hd, p, m->hd, m->rope_theta, m->rope_freq_scale, m->rope_freqs.empty() ? nullptr : m->rope_freqs.data(),
                     m->rope_ext_factor, m->rope_attn_factor, m->rope_n_ctx_orig, 32.0f, 1.0f);
        if (dev_alloc(c->allocs, (void **) &c->rope, tab.size() * 4)) return 1;
        HIPC(hipMemcpy(c->rope, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
        if (dev_alloc(c->allocs, (void **) &c->rope_cur, (size_t) m->hd * 4)) return 1;
        HIPC(hipMemcpy(c->rope_cur, tab.data(), (size_t) m->hd * 4, hipMemcpyHostToDevice));
    }
    if (dev_alloc(c->allocs, (void **) &c->x, (size_t) m->E * 4) || dev_alloc(c->allocs, (void **) &c->x2, (size_t) m->E * 4) ||
        dev_alloc(c->allocs, (void **) &c->q, (size_t) (m->E + 2 * Ekv) * 4) || dev_alloc(c->allocs, (void **) &c->att, (size_t) m->E * 4) ||
        dev_alloc(c->allocs, (void **) &c->h, (size_t) m->F * 4) || dev_alloc(c->allocs, (void **) &c->scores, (size_t) m->H * c->n_ctx_pad * 4) || dev_alloc(c->allocs, (void **) &c->probs, (size_t) m->H * c->n_ctx_pad * 4) ||
        dev_alloc(c->allocs, (void **) &c->logits, (size_t) m->V * 4) || dev_alloc(c->allocs, (void **) &c->st, sizeof(bamd_step_state))) return 1;
    c->k = c->q + m->E; c->v = c->k + Ekv;                           // q | k | v contiguous: rows of the fused QKV mat-vec
    HIPC(hipMemsetAsync(c->st, 0, sizeof(bamd_step_state), c->stream));
    if (dev_alloc(c->allocs, (void **) &c->co_gran, (size_t) m->H * m->hd * 8 + 64)) return 1;
    HIPC(hipMemsetAsync(c->co_gran, 0, (size_t) m->H * m->hd * 8 + 64, c->stream));
    c->co_err = (uint32_t *) (c->co_gran + (size_t) m->H * m->hd);
    HIPC(hipMemsetAsync(c->logits, 0, (size_t) m->V * 4, c->stream));
    HIPC(hipHostMalloc((void **) &c->logits_host, (size_t) m->V * 4 + 64));     // + the give-up words of the co-launch / engine kernels, read back with the logits
    memset(c->logits_host + m->V, 0, 64);
    c->forced_cap = 4096; c->out_cap = n_ctx + 8;
    if (dev_alloc(c->allocs, (void **) &c->forced, (size_t) c->forced_cap * 4) || dev_alloc(c->allocs, (void **) &c->out_tokens, (size_t) c->out_cap * 4)) return 1;
    HIPC(hipStreamSynchronize(c->stream));
    return 0;
}

// every replay of the context is void.  For the rare events that change what a sequence was built with beyond its key (cell tracking on / off, a new slot table), never per token
static void drop_replays(bamd_context * c) {
    c->greedy_graph.reset(); c->greedy_aql.reset(); c->step_aql.reset();
    for (auto & row : c->stage_graph) for (StepReplay & r : row) r.reset();
}
extern "C" __attribute__((visibility("default"))) bamd_context * bamd_context_new(bamd_model * m, int n_ctx) {
    bamd_context * c = new bamd_context();
    if (context_init(c, m, n_ctx)) { bamd_context_free(c); return nullptr; }
    return c;
}
extern "C" __attribute__((visibility("default"))) void bamd_context_free(bamd_context * c) {
    if (!c) return;
    if (c->m) hipSetDevice(c->m->device);
    drop_replays(c);
    if (c->inbox) hipHostFree(c->inbox);
    for (void * p : c->allocs) hipFree(p);
    if (c->logits_host) hipHostFree(c->logits_host);
    if (c->attn_bscr) hipFree(c->attn_bscr);
    if (c->samp_pen_host) hipHostFree(c->samp_pen_host);
    if (c->samp_out_host) hipHostFree(c->samp_out_host);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
}
extern "C" __attribute__((visibility("default"))) int bamd_n_ctx(const bamd_context * c) { return c->n_ctx; }
extern "C" __attribute__((visibility("default"))) void bamd_kv_cache_clear(bamd_context * c) {
    // llama_kv_cache_clear resets the cell metadata; positions are passed per call here, so only the shifted-cell tracking has anything to forget
    c->cells.active = false; c->cells.has_shift = false; c->n_cached = 0;
}

// -------------------------------------------------------------------------------------------------------
// the static per-token pipeline
// -------------------------------------------------------------------------------------------------------
struct StepTimer {                 // optional per-launch HIP-event timing (bamd_profile_step)
    bool on = false;
    std::vector<hipEvent_t> ev; std::vector<int> cls, kind; std::vector<double> bytes;
    // c: 0 mat-vec, 1 attention, 2 other; k: which launch of the layer (0 qkv, 1 attention, 2 other, 3 wo, 4 gate/up, 5 ffn_down, 6 lm_head)
    void begin(hipStream_t s, int c, double b, int k = -1) { if (!on) return; hipEvent_t a; hipEventCreate(&a); hipEventRecord(a, s); ev.push_back(a); cls.push_back(c); kind.push_back(k < 0 ? c : k); bytes.push_back(b); }
    void end(hipStream_t s) { if (!on) return; hipEvent_t b; hipEventCreate(&b); hipEventRecord(b, s); ev.push_back(b); }
    void cancel() { if (!on) return; hipEventDestroy(ev.back()); ev.pop_back(); cls.pop_back(); kind.pop_back(); bytes.pop_back(); }   // the launch behind begin() did not happen
};

static unsigned long long * tl_next(bamd_context * c) {
    if (!c->tl_base || c->tl_slot >= c->tl_cap) return nullptr;
    return c->tl_base + (size_t) (c->tl_slot++) * BAMD_TL_SLOT_WORDS;
}
static void seg_of(bamd_mv_seg & sg, const DevMat & d, float * out) { sg.w = d.stream; sg.out = out; sg.type = d.type; sg.nrows = d.nrows_pad; sg.nvalid = d.nrows; }
// wq | wk | wv share one allocation and their outputs are contiguous (q | k | v from `out`): equal-typed neighbours are ONE segment, one weight stream.  The only place that rule is written down: the decode step,
// the batched prefill and the prefill side tables (DevLayer::aux_qkv) take their segments from here.  nrows / nvalid: as seg_of counts the first matrix + the GGUF rows of each one merged into it; rows_pad: stream rows
// bf16_range: the range word of each segment's weights (the union over the matrices merged into it)
static int qkv_segments(const DevLayer & ly, float * out, bamd_mv_seg sg[3], int rows_pad[3] = nullptr, uint32_t bf16_range[3] = nullptr) {
    const DevMat * mats[3] = { &ly.wq, &ly.wk, &ly.wv };
    int n = 0, off = 0, pad[3]; uint32_t wr[3] = { BAMD_BF16_RANGE_UNKNOWN, BAMD_BF16_RANGE_UNKNOWN, BAMD_BF16_RANGE_UNKNOWN };
    for (int j = 0; j < 3; ++j) {
        const DevMat & d = *mats[j];
        if (j && d.type == mats[j - 1]->type) { sg[n - 1].nrows += d.nrows; sg[n - 1].nvalid += d.nrows; pad[n - 1] += d.nrows_pad; wr[n - 1] = bamd_bf16_range_join(wr[n - 1], d.bf16_range); }
        else { seg_of(sg[n], d, out ? out + off : nullptr); wr[n] = d.bf16_range; pad[n++] = d.nrows_pad; }
        off += d.nrows;
    }
    if (rows_pad) memcpy(rows_pad, pad, sizeof pad);
    if (bf16_range) memcpy(bf16_range, wr, sizeof wr);
    return n;
}

// A launch quantises its activations once, so consecutive QKV segments of one activation form (bamd_act_form_of) are ONE launch: group g is the segments
// [first[g], first[g + 1]).  One group for every model but the one qkv_recipe_mix lets through the load; each launch normalises and quantises x for itself (the
// same deterministic sum, the same bits) and writes its own slice of q | k | v.  The decode step and the batched prompt path both group here
static int qkv_groups(const bamd_mv_seg * sg, int nseg, int first[4]) {
    int n = 0;
    for (int i = 0; i < nseg; ++i) if (!i || bamd_act_form_of(sg[i].type) != bamd_act_form_of(sg[i - 1].type)) first[n++] = i;
    first[n] = nseg;
    return n;
}
static int qkv_launches(const DevLayer & ly) { bamd_mv_seg sg[3]; int first[4]; return qkv_groups(sg, qkv_segments(ly, nullptr, sg), first); }

// enqueue the layers of this stage for the token whose hidden state is in c->x; leaves the result in c->x
// pos_hi: the highest position this enqueue (or every replay of the graph being captured) will see.  The single-launch attention
// kernel (one workgroup per query head, serial over the sequence) wins below ~450 positions (measured crossover, 8B shape: 1.73 vs
// 1.85 ms/token at 240, equal at 440, 2.06 vs 1.88 at 740) at any n_ctx (its LDS score rows are sized by the sequence bound, not by n_ctx); longer sequences take the
// three-kernel path, whose cost is nearly flat up to a few thousand positions.
static bool attn_fused_for(const bamd_context * c, int pos_hi) { return g_attn_fused && pos_hi < 448 && !c->cells.active; }   // shifted cells: three-launch path (attn_qk_kernel<.., SH>)
static AttnPath attn_path(const bamd_context * c, int pos_hi) { return attn_fused_for(c, pos_hi) ? ATTN_SINGLE : c->cells.active ? ATTN_CELLS : ATTN_SPLIT; }
// LDS row length of the single-launch / batched attention kernels for sequences up to position pos_hi: a multiple of 64, independent of n_ctx
static int attn_lds_ld(const bamd_context * c, int pos_hi) { return std::min((pos_hi + 1 + 63) / 64 * 64, c->n_ctx_pad); }
static int enqueue_layers(bamd_context * c, int prefill_mode, hipStream_t s, StepTimer * tm, int pos_hi) {
    bamd_model * m = c->m;
    const int gq = m->H / m->Hkv;
    static const int qk_tiles = [] { const char * e = getenv("BAMD_QK_TILES"); return e ? atoi(e) : 64; }();   // score-kernel workgroups per KV head: 64 = two per CU at Hkv = 8 (16 waves per CU: 2.066 -> 2.038 ms/token at 8000 positions; 128: 2.13)
    const int tiles = std::min(std::max(c->n_ctx / 64, 1), qk_tiles);
    for (size_t il = 0; il < m->layers.size(); ++il) {
        const DevLayer & ly = m->layers[il];
        bamd_mv_args a; memset(&a, 0, sizeof a);
        // 1. q,k,v = W{q,k,v} . Q8_K(rms_norm(x) * attn_norm)          (llama.cpp:8810-8835), one launch per activation form (qkv_groups)
        bamd_mv_seg qs[3]; int gf[4];
        const int ng = qkv_groups(qs, qkv_segments(ly, c->q, qs), gf);
        for (int g = 0; g < ng; ++g) {
            memset(&a, 0, sizeof a);
            double bytes = 0.0;
            for (int i = gf[g]; i < gf[g + 1]; ++i) { a.seg[a.nseg++] = qs[i]; bytes += (double) (bamd_row_bytes(qs[i].type, m->E) * (size_t) qs[i].nvalid); }
            a.x = c->x; a.normw = ly.attn_norm; a.eps = m->eps; a.K = m->E; a.tl = tl_next(c);
            if (tm) tm->begin(s, 0, bytes);
            if (bamd_launch_mv(a, BAMD_PRO_NORM, BAMD_EPI_STORE, m->n_cu, s)) return fail("mat-vec launch: a matrix type without a kernel");
            if (tm) tm->end(s);
        }
        // 2. RoPE, KV store, softmax(QK^T) V                               (llama.cpp:8837-8849, :8318-8353)
        bamd_attn_args t; memset(&t, 0, sizeof t);
        t.st = c->st; t.q = c->q; t.k = c->k; t.v = c->v; t.kc = c->kc[il]; t.vc = c->vc[il]; t.rope = c->rope; t.rope_cur = c->rope_cur; t.scores = c->scores; t.probs = c->probs; t.out = c->att;
        t.hd = m->hd; t.Hkv = m->Hkv; t.n_ctx = c->n_ctx_pad; t.kq_scale = 1.0f / sqrtf((float) m->hd); t.prefill_mode = prefill_mode;
        // the probability rows in global memory are the data path of the softmax | P.V PAIR only (score rows beyond the LDS); the one-launch softmax + P.V keeps them in
        // LDS and wrote them out for the tests' sake — 2 x 31 KB of stores by sixteen of its workgroups, the ones the launch then ended with
        if (bamd_attention_split_is_ik_clean(t, m->H / m->Hkv)) t.probs = nullptr;
        // single-launch kernel below 448 positions, three kernels (scores | softmax | P.V) above (attn_fused_for)
        t.lds_ld = std::min(512, c->n_ctx_pad);               // single-launch kernel only (sequences < 448 positions): constant, so captured graphs stay valid as pos advances
        t.cellpos = c->cells.active ? c->cellpos : nullptr;
        // 3. x2 = x + Wo . Q8_K(att)                                        (llama.cpp:8294-8303, :8864)
        memset(&a, 0, sizeof a);
        seg_of(a.seg[0], ly.wo, c->x2); a.nseg = 1; a.x = c->att; a.K = m->E; a.res = c->x;
        // 2 + 3 in ONE launch when the attention takes its single-launch kernel and the wo shape has a co-launch instance: the wo workgroups
        // fetch their weights on the CUs the attention leaves idle (bamd_colaunch.hip)
        bool co = false;
        if (attn_fused_for(c, pos_hi) && !prefill_mode) {
            unsigned long long * tl = tl_next(c);
            t.tl = tl; a.tl = tl;
            if (tm) tm->begin(s, 1, (double) ly.wo.bytes);
            co = bamd_launch_attn_wo(t, gq, a, m->n_cu, c->co_gran, (int) (il & 255), c->co_err, s) == 0;
            if (tm) { if (co) tm->end(s); else tm->cancel(); }
            if (!co && tl) c->tl_slot--;
        }
        if (!co) {
            if (tm) tm->begin(s, 1, 0.0);
            t.tl = tl_next(c);
            if (bamd_launch_attention(t, gq, attn_fused_for(c, pos_hi) ? tiles : -tiles, s)) return fail("attention launch: unsupported head configuration");
            if (tm) tm->end(s);
            a.tl = tl_next(c);
            if (tm) tm->begin(s, 0, (double) ly.wo.bytes, 3);
            if (bamd_launch_mv(a, BAMD_PRO_PLAIN, BAMD_EPI_ADD, m->n_cu, s)) return fail("mat-vec launch: a matrix type without a kernel");
            if (tm) tm->end(s);
        }
        // 4. h = silu(Wg . a) * (Wu . a),  a = Q8_K(rms_norm(x2) * ffn_norm)  (llama.cpp:8869-8885)
        memset(&a, 0, sizeof a);
        seg_of(a.seg[0], ly.wg, c->h); seg_of(a.seg[1], ly.wu, c->h); a.nseg = 2; a.x = c->x2; a.normw = ly.ffn_norm; a.eps = m->eps; a.K = m->E; a.tl = tl_next(c);
        if (tm) tm->begin(s, 0, (double) (ly.wg.bytes + ly.wu.bytes), 4);
        if (bamd_launch_mv(a, BAMD_PRO_NORM, BAMD_EPI_SILU_MUL, m->n_cu, s)) return fail("mat-vec launch: a matrix type without a kernel");
        if (tm) tm->end(s);
        // 5. x = x2 + Wd . Q8_K(h)                                          (llama.cpp:8885, :8902)
        memset(&a, 0, sizeof a);
        seg_of(a.seg[0], ly.wd, c->x); a.nseg = 1; a.x = c->h; a.K = m->F; a.res = c->x2; a.tl = tl_next(c);
        if (tm) tm->begin(s, 0, (double) ly.wd.bytes, 5);
        if (bamd_launch_mv(a, BAMD_PRO_PLAIN, BAMD_EPI_ADD, m->n_cu, s)) return fail("mat-vec launch: a matrix type without a kernel");
        if (tm) tm->end(s);
    }
    return 0;
}
static int enqueue_lm_head(bamd_context * c, hipStream_t s, StepTimer * tm) {
    bamd_model * m = c->m;
    bamd_mv_args a; memset(&a, 0, sizeof a);
    seg_of(a.seg[0], m->output, c->logits); a.nseg = 1; a.x = c->x; a.normw = m->out_norm; a.eps = m->eps; a.K = m->E; a.best_key = &c->st->best_key; a.tl = tl_next(c);
    if (tm) tm->begin(s, 0, (double) m->output.bytes, 6);
    if (bamd_launch_mv(a, BAMD_PRO_NORM, BAMD_EPI_ARGMAX, m->n_cu, s)) return fail("mat-vec launch: a matrix type without a kernel");
    if (tm) tm->end(s);
    return 0;
}
static void enqueue_begin(bamd_context * c, int n_forced, int do_embed, hipStream_t s, bool with_slots = false) {
    bamd_model * m = c->m;
    bamd_launch_step_begin(c->st, c->forced, n_forced, c->out_tokens, m->tok_embd.raw, m->tok_embd.type, m->E, m->V, c->x, do_embed, s,
                           with_slots ? c->slots : nullptr, with_slots ? c->cellpos : nullptr, c->rope, c->rope_cur, m->hd);
}

static int enqueue_step(bamd_context * c, hipStream_t s, int pos_hi) { if (enqueue_layers(c, 0, s, nullptr, pos_hi)) return 1; return enqueue_lm_head(c, s, nullptr); }   // a whole single-stage step behind its step_begin launch

// The tag of a granule hand-over (bamd_colaunch.hip) is (host serial : 12, device step : 12, layer : 8); a word must never already hold the tag a
// consumer is about to wait for.  The serial runs 1 .. 0xffe (0 is what zero-initialised granules carry, 0xfff is reserved) and every time it wraps ALL granule
// vectors of the context are overwritten with 0xff bytes — tag 0xffffffff, which no launch produces — in stream order ahead of the launch that reuses serial 1
// (with a bare 12-bit counter a stale granule of 4096 host calls ago carried the awaited tag and a gather passed without waiting).
static int next_serial(bamd_context * c, hipStream_t s) {
    if (++c->host_serial > 0xffe) {
        c->host_serial = 1;
        const bamd_model * m = c->m;
        if (c->co_gran) HIPC(hipMemsetAsync(c->co_gran, 0xff, (size_t) m->H * m->hd * 8, s));
    }
    return 0;
}
static int set_state(bamd_context * c, int pos_base, hipStream_t s, bool keep_key) {
    bamd_step_state h; memset(&h, 0, sizeof h);
    if (next_serial(c, s)) return 1;
    h.pos_base = pos_base; h.n_ctx = c->n_ctx; h.serial = c->host_serial;
    if (keep_key) {
        // keep best_key (the arg-max of the previous lm_head): rewrite only the leading fields
        HIPC(hipMemcpyAsync(c->st, &h, offsetof(bamd_step_state, best_key), hipMemcpyHostToDevice, s));
    } else HIPC(hipMemcpyAsync(c->st, &h, sizeof h, hipMemcpyHostToDevice, s));
    return 0;
}

// May a step with this attention path run as AQL packets on the library's own queue (bamd_aql.h)?  Only the launch sequences whose kernels keep the inter-kernel rules of bamd_device.h: the single-launch
// attention path, and the scores | softmax + P.V path of long sequences when its kernels are the clean ones; anything else (shifted cells, score rows beyond the LDS) replays a hipGraph
static bool aql_allowed(const bamd_context * c, AttnPath path) {
    if (!g_aql || c->aql_failed || path == ATTN_CELLS || bamd_aql_gave_up(c->m->device)) return false;     // (gave up: a run found the device's queue stuck, bamd_aql_run)
    if (path == ATTN_SINGLE) return true;
    const bamd_model * m = c->m;
    bamd_attn_args t; memset(&t, 0, sizeof t); t.hd = m->hd; t.Hkv = m->Hkv; t.n_ctx = c->n_ctx_pad;
    return bamd_attention_split_is_ik_clean(t, m->H / m->Hkv) != 0;
}
// enqueue() issues the step's launches while the launchers record instead of launching (BAMD_LAUNCH); the recording becomes packets.  nullptr: this context leaves the own queue alone from here on
template <typename F> static bamd_aql_graph * record_aql(bamd_context * c, F enqueue) {
    bamd_aql_recording rec;
    bamd_aql_rec = &rec;
    const int rc = enqueue();
    bamd_aql_rec = nullptr;
    const char * why = "recording failed";
    bamd_aql_graph * g = rc ? nullptr : bamd_aql_build(c->m->device, rec, &why);
    if (!g) { c->aql_failed = true; if (getenv("BAMD_AQL_VERBOSE")) fprintf(stderr, "bamd: own AQL queue not used: %s\n", why ? why : "?"); }
    return g;
}
// enqueue() issues the launches on `s` under stream capture; the graph is instantiated into *exec.  what: the error texts of a failed capture / instantiation (ending in ": ": + the HIP error string)
struct CaptureTexts { const char * capture, * instantiate; };
static int capture_fail(const char * text, hipError_t e) { return fail(std::string(text) + (text[strlen(text) - 1] == ' ' ? hipGetErrorString(e) : "")); }
template <typename F> static int capture_graph(hipStream_t s, F enqueue, hipGraphExec_t * exec, const CaptureTexts & what) {
    hipGraph_t g = nullptr;
    HIPC(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue();
    hipError_t e = hipStreamEndCapture(s, &g);
    if (rc || e != hipSuccess) { if (g) hipGraphDestroy(g); return rc ? rc : capture_fail(what.capture, e); }
    e = hipGraphInstantiate(exec, g, nullptr, nullptr, 0);
    hipGraphDestroy(g);
    if (e != hipSuccess) { *exec = nullptr; return capture_fail(what.instantiate, e); }
    return 0;
}

// ---- KV cell bookkeeping after position edits (llama_kv_cache_seq_rm / _seq_add / find_slot / update) ------------------------------------
// The reference keeps, per cache cell, the position it holds and a pending rotation delta (llama.cpp:2700-2760).  As long as nobody edits
// positions, cell i holds position i and nothing is tracked here.  Booster's context shift (cpp/bridge.cpp:487-503) is
//     llama_kv_cache_seq_rm (ctx, 0, n_keep, n_keep + n_discard);  llama_kv_cache_seq_add(ctx, 0, n_keep + n_discard, n_past, -n_discard);
// after which cells and positions differ: freed cells are refilled in cell order (find_slot), the attention runs over CELLS (mask by the
// position each holds), and the K rows of the moved cells are re-rotated by their delta before the next evaluation (K-shift).
// the cells are back to "cell i holds position i" with nothing pending (e.g. after a plain truncation, seq_rm(n, -1)): stop tracking, so that
// micro-batches, the device-side greedy loop and the single-launch attention are available again (llama_decode has no such modes to lose)
static void kv_try_deactivate(bamd_context * c) {
    bamd_context::Cells & k = c->cells;
    if (!k.active || k.has_shift) return;
    for (int i = 0; i < c->n_ctx; ++i) if (k.pos[(size_t) i] != (i < k.used ? i : -1)) return;
    if (k.head != (k.used >= c->n_ctx ? 0 : k.used)) return;
    k.active = false;
    c->n_cached = k.used;
    drop_replays(c);
}
static int kv_activate(bamd_context * c) {
    // cell metadata is edited on the host and copied with blocking copies: nothing of this context may be in flight (the caller's stage
    // streams are hipStreamNonBlocking, so the null-stream copies below would not wait for them)
    HIPC(hipDeviceSynchronize());
    if (c->cells.active) return 0;
    bamd_context::Cells & k = c->cells;
    k.pos.assign((size_t) c->n_ctx, -1); k.delta.assign((size_t) c->n_ctx, 0);
    const int n = std::min(c->n_cached, c->n_ctx);
    for (int i = 0; i < n; ++i) k.pos[(size_t) i] = i;
    k.used = n; k.head = n >= c->n_ctx ? 0 : n;          // llama_decode_internal: head += n_tokens, wraps to 0 at size (llama.cpp:14743-14748)
    if (!c->cellpos && dev_alloc(c->allocs, (void **) &c->cellpos, (size_t) c->n_ctx_pad * 4)) return 1;
    std::vector<int32_t> h((size_t) c->n_ctx_pad, -1);
    memcpy(h.data(), k.pos.data(), (size_t) c->n_ctx * 4);
    HIPC(hipMemcpy(c->cellpos, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    k.active = true;
    drop_replays(c);
    return 0;
}
extern "C" __attribute__((visibility("default"))) int bamd_kv_seq_rm(bamd_context * c, int p0, int p1) {     // llama_kv_cache_seq_rm(ctx, 0, p0, p1): llama.cpp:3150-3217
    HIPC(hipSetDevice(c->m->device));
    if (kv_activate(c)) return 1;
    bamd_context::Cells & k = c->cells;
    if (p0 < 0) p0 = 0;
    if (p1 < 0) p1 = 0x7fffffff;
    int new_head = c->n_ctx;
    for (int i = 0; i < c->n_ctx; ++i) {
        if (k.pos[(size_t) i] >= p0 && k.pos[(size_t) i] < p1) {           // one sequence: a cell is empty once it leaves it
            if (k.pos[(size_t) i] >= 0) k.used--;
            k.pos[(size_t) i] = -1;
            if (new_head == c->n_ctx) new_head = i;
        }
    }
    if (new_head != c->n_ctx && new_head < k.head) k.head = new_head;
    HIPC(hipMemcpy(c->cellpos, k.pos.data(), (size_t) c->n_ctx * 4, hipMemcpyHostToDevice));
    kv_try_deactivate(c);
    return 0;
}
extern "C" __attribute__((visibility("default"))) int bamd_kv_seq_add(bamd_context * c, int p0, int p1, int delta) {   // llama_kv_cache_seq_add: llama.cpp:3268-3313
    HIPC(hipSetDevice(c->m->device));
    if (kv_activate(c)) return 1;
    bamd_context::Cells & k = c->cells;
    if (p0 < 0) p0 = 0;
    if (p1 < 0) p1 = 0x7fffffff;
    if (p0 == p1) return 0;
    int new_head = c->n_ctx;
    for (int i = 0; i < c->n_ctx; ++i) {
        if (k.pos[(size_t) i] >= 0 && k.pos[(size_t) i] >= p0 && k.pos[(size_t) i] < p1) {
            k.has_shift = true;
            k.pos[(size_t) i] += delta; k.delta[(size_t) i] += delta;
            if (k.pos[(size_t) i] < 0) { k.used--; k.pos[(size_t) i] = -1; if (new_head == c->n_ctx) new_head = i; }
        }
    }
    k.head = new_head != c->n_ctx ? new_head : 0;
    HIPC(hipMemcpy(c->cellpos, k.pos.data(), (size_t) c->n_ctx * 4, hipMemcpyHostToDevice));
    return 0;
}
extern "C" __attribute__((visibility("default"))) int bamd_kv_seq_div(bamd_context * c, int p0, int p1, int d) {       // llama_kv_cache_seq_div: llama.cpp:3315-3350 (Self-Extend)
    HIPC(hipSetDevice(c->m->device));
    if (d < 1) return fail("bamd_kv_seq_div: divisor < 1");
    if (kv_activate(c)) return 1;
    bamd_context::Cells & k = c->cells;
    if (p0 < 0) p0 = 0;
    if (p1 < 0) p1 = 0x7fffffff;
    if (p0 == p1) return 0;
    for (int i = 0; i < c->n_ctx; ++i) {
        if (k.pos[(size_t) i] >= 0 && k.pos[(size_t) i] >= p0 && k.pos[(size_t) i] < p1) {
            k.has_shift = true;
            const int32_t p_old = k.pos[(size_t) i];
            k.pos[(size_t) i] /= d; k.delta[(size_t) i] += k.pos[(size_t) i] - p_old;
        }
    }
    HIPC(hipMemcpy(c->cellpos, k.pos.data(), (size_t) c->n_ctx * 4, hipMemcpyHostToDevice));
    return 0;
}
// the K-shift's cos / sin table (kv_update, bamd_op_k_shift): row 0 = delta 0 (the reference rotates EVERY cell, most by zero), then the distinct
// non-zero deltas in ascending order (a context shift: one value; Self-Extend: up to one per cell); idx[cell] = the row of the cell's delta for the
// n_cells cells (the rest of idx, up to n_idx, row 0); tab[row][hd] = rope_row of the row's delta with the rope parameters given
void k_shift_table(const int32_t * delta, int n_cells, int n_idx, int hd, float freq_base, float freq_scale, const float * freq_factors,
                          float ext_factor, float attn_factor, int n_ctx_orig, std::vector<int32_t> & idx, std::vector<float> & tab) {
    std::vector<int32_t> vals(1, 0);
    idx.assign((size_t) n_idx, 0);
    std::vector<int32_t> sorted(delta, delta + n_cells);
    std::sort(sorted.begin(), sorted.end());
    sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
    for (int32_t d : sorted) if (d != 0) vals.push_back(d);
    for (int i = 0; i < n_cells; ++i) {
        const int32_t d = delta[i];
        idx[(size_t) i] = d == 0 ? 0 : (int32_t) (std::lower_bound(vals.begin() + 1, vals.end(), d) - vals.begin());
    }
    tab.assign(vals.size() * (size_t) hd, 0.0f);
    for (size_t j = 0; j < vals.size(); ++j)
        rope_row(tab.data() + j * hd, vals[j], hd, freq_base, freq_scale, freq_factors, ext_factor, attn_factor, n_ctx_orig, 32.0f, 1.0f);
}
// llama_kv_cache_update_internal (llama.cpp:15245-15277): apply the pending K-shift to every layer's K cache, clear the deltas
static int kv_update(bamd_context * c, hipStream_t s) {
    bamd_context::Cells & k = c->cells;
    if (!k.has_shift) return 0;
    bamd_model * m = c->m;
    std::vector<int32_t> idx;
    std::vector<float> tab;
    k_shift_table(k.delta.data(), c->n_ctx, c->n_ctx_pad, m->hd, m->rope_theta, m->rope_freq_scale, m->rope_freqs.empty() ? nullptr : m->rope_freqs.data(),
                  m->rope_ext_factor, m->rope_attn_factor, m->rope_n_ctx_orig, idx, tab);   // the parameters of the context's own table (bamd_context_new)
    if (!c->shift_idx && dev_alloc(c->allocs, (void **) &c->shift_idx, (size_t) c->n_ctx_pad * 4)) return 1;
    if (!c->shift_tab) { if (dev_alloc(c->allocs, (void **) &c->shift_tab, (size_t) (c->n_ctx + 1) * m->hd * 4)) return 1; c->shift_tab_cap = c->n_ctx + 1; }
    HIPC(hipMemcpyAsync(c->shift_idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(c->shift_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, s));
    for (size_t il = 0; il < m->layers.size(); ++il) bamd_launch_k_shift(c->kc[il], c->n_ctx, m->Hkv, m->hd, c->shift_idx, c->shift_tab, s);
    HIPC(hipStreamSynchronize(s));                           // (idx / tab are host temporaries)
    k.has_shift = false;
    std::fill(k.delta.begin(), k.delta.end(), 0);
    return 0;
}
// llama_kv_cache_find_slot for one token (llama.cpp:3028-3127) with llama_decode_internal's head handling (:14686-14688, :14743-14748);
// *n_kv = the padded length the attention runs over (:14693-14701)
static int kv_find_slot(bamd_context * c, int pos, int * cell, int * n_kv) {
    bamd_context::Cells & k = c->cells;
    const int size = c->n_ctx;
    if (k.head > k.used + 2) k.head = 0;
    int n_tested = 0;
    for (;;) {
        if (k.head + 1 > size) { n_tested += size - k.head; k.head = 0; continue; }
        if (k.pos[(size_t) k.head] >= 0) { k.head += 1; n_tested += 1; if (n_tested >= size) return fail("KV cache full: no free cell (llama_decode would return 1)"); continue; }
        break;
    }
    *cell = k.head;
    k.pos[(size_t) k.head] = pos; k.used += 1;
    int cell_max = 0;
    for (int i = size; i > 0; --i) if (k.pos[(size_t) (i - 1)] >= 0) { cell_max = i; break; }
    *n_kv = std::min(size, std::max(32, (cell_max + 31) / 32 * 32));
    k.head += 1; if (k.head >= size) k.head = 0;
    return 0;
}

// ---- batched prefill: a micro-batch of T > 1 tokens through the layers at once (llama_decode with n_tokens > 1) -----------
// The scratch block of the batched attention (score rows of the matrix-core kernel beyond 512 positions, of every kernel beyond the LDS: bamd_attention_batch_plan),
// sized by the plan of this micro-batch under the budget and grown while nothing of this context is in flight on `s` (freed with the context).
// true = the attention of the micro-batch has its kernels: the block is there, or its score rows still fit the LDS (2 x padded length floats per head: 18 432
// positions), where the VALU kernels run without one.  false = beyond the LDS without a block: the caller evaluates token by token.
static size_t attn_scratch_budget() { return (size_t) g_attn_scratch_mb << 20; }      // 0 = the plan's default
static bool ensure_attn_scratch(bamd_context * c, int T, int n_past, hipStream_t s) {
    const bamd_model * m = c->m;
    const int gq = m->H / m->Hkv, ld = attn_lds_ld(c, std::max(n_past, 0) + T - 1);      // (a negative n_past is the caller's error to report)
    const bool lds_ok = (size_t) ld * 8 <= 144 * 1024;
    size_t need = 0;
    if (bamd_attention_batch_plan(m->Hkv, gq, m->hd, T, ld, 0, attn_scratch_budget(), nullptr, nullptr, &need)) return false;
    if (need > c->attn_bscr_bytes && !(c->attn_bscr_failed && need >= c->attn_bscr_failed)) {   // (replaced only while nothing of this context is in flight: stream order)
        if (hipStreamSynchronize(s) != hipSuccess) { (void) hipGetLastError(); return false; }
        if (c->attn_bscr) hipFree(c->attn_bscr);
        c->attn_bscr = nullptr; c->attn_bscr_bytes = 0;
        // ~ H * T * ld * 4 bytes up to the budget (0.5 GB at 8 K positions on the 8B shape, 1.2 GB from 18 K on; 2.4 GB on a 70B stage).  If the device cannot spare
        // it the prompt is not lost: without a block the VALU kernels with their rows in LDS run, and beyond the LDS the micro-batch goes token by token
        if (hipMalloc((void **) &c->attn_bscr, need) == hipSuccess) c->attn_bscr_bytes = need;
        else { (void) hipGetLastError(); c->attn_bscr = nullptr; c->attn_bscr_failed = need; }   // not retried for this size or larger (every layer of every micro-batch drained the stream and failed again)
    }
    return need <= c->attn_bscr_bytes || lds_ok;
}
// a micro-batch of T tokens behind n_past cached positions has batched kernels for every operation (and the scratch block its attention needs: allocated here)
static bool prefill_batch_supported(bamd_context * c, int T, int n_past, hipStream_t s) {
    const bamd_model * m = c->m;
    const int gq = m->H / m->Hkv;
    if (!(g_prefill_batch && g_attn_fused && m->hd <= 256 && (m->hd & 63) == 0 && gq >= 1 && gq <= 8)) return false;
    // every mat-mul needs a kernel: the matrix-core kernels take every K-quant at any K when the model has its side tables; the integer-dot kernel
    // takes any K-quant while 4 tokens of Q8_K activations fit the LDS (K <= 35840; tiles of 8 tokens up to K = 17920)
    // (the unquantised family: its VALU kernel takes any K the load accepted)
    auto ok = [&](int type, int K) { return bamd_is_flt(type) || (g_prefill_mfma && m->aux_ok && bamd_prefill_mfma_type(type)) || 4 * bamd_blob_bytes(K) <= 160 * 1024; };
    for (const DevLayer & ly : m->layers)
        if (!ok(ly.wq.type, m->E) || !ok(ly.wk.type, m->E) || !ok(ly.wv.type, m->E) || !ok(ly.wo.type, m->E) || !ok(ly.wg.type, m->E) || !ok(ly.wu.type, m->E) || !ok(ly.wd.type, m->F)) return false;
    return ensure_attn_scratch(c, T, n_past, s);
}
// prefill side tables of every layer matrix (bamd_prefill2.hip), built at model load (round 6; round 5 built them lazily inside the first batched evaluation — a
// multi-gigabyte allocation after the contexts existed, and a partial failure mixed kernel generations: ADVICE r5).  The QKV segments are the ones
// enqueue_prefill_batch launches (qkv_segments).  All or nothing.
static void build_prefill_aux(bamd_model * m, hipStream_t s) {
    if (!g_prefill_aux) { m->aux_why = "switched off (BAMD_PREFILL_AUX=0)"; return; }
    if (!bamd_prefill_mfma_supported()) { m->aux_why = "the device refuses the matrix-core kernels' LDS size"; return; }
    struct Item { const void * w; int type, nrows, K; void ** slot; };
    std::vector<Item> items;
    for (DevLayer & ly : m->layers) {
        bamd_mv_seg seg[3]; int rows[3];
        const int n = qkv_segments(ly, nullptr, seg, rows);
        for (int i = 0; i < n; ++i) items.push_back({ seg[i].w, seg[i].type, rows[i], m->E, &ly.aux_qkv[i] });
        items.push_back({ ly.wo.stream, ly.wo.type, ly.wo.nrows_pad, m->E, &ly.aux_o });
        items.push_back({ ly.wg.stream, ly.wg.type, ly.wg.nrows_pad, m->E, &ly.aux_g });
        items.push_back({ ly.wu.stream, ly.wu.type, ly.wu.nrows_pad, m->E, &ly.aux_u });
        items.push_back({ ly.wd.stream, ly.wd.type, ly.wd.nrows_pad, m->F, &ly.aux_d });
    }
    // F32 / F16 matrices with BAMD_PREFILL_FLT on, BF16 ones with BAMD_PREFILL_BF16 on: their matrix-core kernel has no side table (bamd_batch_mm reads the switch at each launch), so they ask for
    // nothing here; a model of such matrices only has nothing to build and nothing to report
    const size_t n_all = items.size();
    items.erase(std::remove_if(items.begin(), items.end(), [](const Item & it) { return bamd_prefill_mfma_type_notable(it.type); }), items.end());
    if (n_all && items.empty()) { m->aux_none_needed = true; return; }
    size_t need = 0;
    for (const Item & it : items) {
        const size_t b = bamd_prefill_aux_bytes(it.type, it.nrows, it.K);
        if (!b) { m->aux_why = bamd_prefill_reason(it.type); return; }      // (the sentences: bamd_prefill_family.cpp)
        need += b + 4096;
    }
    if (items.empty()) return;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void) hipGetLastError(); m->aux_why = "hipMemGetInfo failed"; return; }
    double reserve_gb = 8.0; if (const char * e = getenv("BAMD_PREFILL_AUX_RESERVE_GB")) reserve_gb = atof(e);
    const size_t reserve = (size_t) (reserve_gb * 1073741824.0);
    if (need + reserve > free_b) {
        char b[256]; snprintf(b, sizeof b, "side tables need %.2f GiB, %.2f GiB free, %.1f GiB must stay free (BAMD_PREFILL_AUX_RESERVE_GB)", need / 1073741824.0, free_b / 1073741824.0, reserve_gb);
        m->aux_why = b; return;
    }
    std::vector<void *> got;
    for (const Item & it : items) {
        void * p = nullptr;
        if (hipMalloc(&p, bamd_prefill_aux_bytes(it.type, it.nrows, it.K)) != hipSuccess) {
            (void) hipGetLastError();
            for (void * q : got) hipFree(q);
            for (const Item & jt : items) *jt.slot = nullptr;
            m->aux_why = "allocation failed"; m->aux_bytes = 0; return;
        }
        got.push_back(p); *it.slot = p; m->aux_bytes += (int64_t) bamd_prefill_aux_bytes(it.type, it.nrows, it.K);
        bamd_launch_prefill_aux(it.w, it.type, it.nrows, it.K, p, s);
    }
    for (void * q : got) m->allocs.push_back(q);
    hipStreamSynchronize(s);
    m->aux_ok = true;
}
static int ensure_batch_buffers(bamd_context * c) {
    if (c->bcap) return 0;
    bamd_model * m = c->m;
    const size_t T = BAMD_PREFILL_CAP, Ekv = (size_t) m->Hkv * m->hd;
    size_t flt_bytes = 0;
    for (const DevLayer & ly : m->layers)
        for (const DevMat * d : { &ly.wq, &ly.wk, &ly.wv, &ly.wo, &ly.wg, &ly.wu, &ly.wd }) flt_bytes = std::max(flt_bytes, bamd_flt_act_bytes(bamd_act_form_of(d->type), d->K));
    if (dev_alloc(c->allocs, (void **) &c->bx, T * m->E * 4) || dev_alloc(c->allocs, (void **) &c->bx2, T * m->E * 4) ||
        dev_alloc(c->allocs, (void **) &c->bqkv, T * (m->E + 2 * Ekv) * 4) || dev_alloc(c->allocs, (void **) &c->batt, T * m->E * 4) ||
        dev_alloc(c->allocs, (void **) &c->bh, T * m->F * 4) ||
        dev_alloc(c->allocs, (void **) &c->bblob, T * std::max(bamd_blob_bytes(std::max(m->E, m->F)), flt_bytes)) ||      // (an unquantised matrix takes its activations as f32 / bf16 rows)
        dev_alloc(c->allocs, (void **) &c->bbfr, T * 4) ||
        dev_alloc(c->allocs, (void **) &c->bblob16, T * bamd_blob16_bytes(std::max(m->E, m->F)))) return 1;     // (one stride for every form: the K-quant record's 608 B hold the 544 B of the Q8_0 form and the 576 B of the Q8_1 form)
    c->bcap = (int) T;
    return 0;
}
// one batched mat-mul: K-quant segments with a side table on the matrix-core kernels, the rest on the integer-dot kernel (identical bits either way).
// aux[i]: side table of segment i (null: none); blob16: the f16 activations of the matrix-core kernel.  The ONE place this routing is written down: the
// prompt path below and the op-level entry point (bamd_op_mul_mat_batch_seg) both come through here
int bamd_batch_mm(bamd_mm_args a, int epi, const void * blob16, const void * const * aux, int n_cu, hipStream_t s, const bamd_bf16_ranges * bf) {
    const int T = a.T;
    // (F32 / F16 with BAMD_PREFILL_FLT on: no side table — the switch is read here, at each launch; their kernel takes the f32 rows of a.blob.  BF16 with
    // BAMD_PREFILL_BF16 on: the same, with the bf16 rows and the range words beside them)
    auto on_mfma = [&](int i) { return g_prefill_mfma && ((bamd_prefill_mfma_type_notable(a.seg[i].type) && (a.seg[i].type != BAMD_BF16 || bf)) || (aux[i] && bamd_prefill_mfma_type(a.seg[i].type))); };
    auto mm_mfma = [&](const bamd_mv_seg & sg, const void * ax, int nv, float * out, const float * res, int e) {
        if (sg.type == BAMD_BF16) return bamd_launch_matmul_mfma_bf16(sg.w, bf->w[&sg - a.seg], nv, sg.nrows, a.K, a.blob, bf->x, T, out, res, e, a.ldo, s);
        if (sg.type == BAMD_F32 || sg.type == BAMD_F16) return bamd_launch_matmul_mfma_flt(sg.w, sg.type, nv, sg.nrows, a.K, a.blob, T, out, res, e, a.ldo, s);
        return bamd_launch_matmul_mfma2(sg.w, ax, sg.type, nv, sg.nrows, a.K, blob16, T, out, res, e, a.ldo, s);
    };
    if (epi == BAMD_EPI_SILU_MUL) {
        if (on_mfma(0) && on_mfma(1) && a.seg[1].type == a.seg[0].type) {
            const int nv = a.seg[0].nvalid > 0 ? a.seg[0].nvalid : a.seg[0].nrows;
            if (mm_mfma(a.seg[0], aux[0], nv, a.seg[0].out, nullptr, BAMD_EPI_STORE)) return 1;   // gate -> h
            // up, with h = silu(gate) * up as its epilogue (every element is read and rewritten by the one lane that owns it)
            if (mm_mfma(a.seg[1], aux[1], nv, a.seg[0].out, a.seg[0].out, BAMD_EPI_SILU_MUL)) return 1;
            return 0;
        }
        return bamd_launch_matmul_batch(a, epi, n_cu, s);
    }
    bamd_mm_args rest = a; rest.nseg = 0;
    for (int i = 0; i < a.nseg; ++i) {
        if (on_mfma(i)) {
            const int nv = a.seg[i].nvalid > 0 ? a.seg[i].nvalid : a.seg[i].nrows;
            const float * res = epi == BAMD_EPI_ADD ? a.res + (a.seg[i].out - a.seg[0].out) : nullptr;
            if (mm_mfma(a.seg[i], aux[i], nv, a.seg[i].out, res, res ? BAMD_EPI_ADD : BAMD_EPI_STORE)) return 1;
        } else rest.seg[rest.nseg++] = a.seg[i];
    }
    if (rest.nseg) {
        if (epi == BAMD_EPI_ADD) rest.res = a.res + (rest.seg[0].out - a.seg[0].out);
        return bamd_launch_matmul_batch(rest, epi, n_cu, s);
    }
    return 0;
}
static int batch_mm(bamd_context * c, const bamd_mm_args & a, int epi, hipStream_t s, const void * const * aux, uint32_t w0 = BAMD_BF16_RANGE_UNKNOWN, uint32_t w1 = BAMD_BF16_RANGE_UNKNOWN,
                    uint32_t w2 = BAMD_BF16_RANGE_UNKNOWN) {
    const bamd_bf16_ranges bf = { c->bbfr, { w0, w1, w2 } };
    return bamd_batch_mm(a, epi, c->bblob16, aux, c->m->n_cu, s, &bf);
}
// first stage: tokens already in c->forced; later stages: hidden_in [T][E] f32 on this device.  Last stage: leaves the hidden state of
// the LAST token in c->x (for lm_head); other stages: writes hidden_out [T][E] (possibly on the next device: peer copy).
static int enqueue_prefill_batch(bamd_context * c, int T, int n_past, hipStream_t s, const void * hidden_in = nullptr, void * hidden_out = nullptr) {
    bamd_model * m = c->m;
    const int E = m->E, F = m->F, Ekv = m->Hkv * m->hd, ldq = E + 2 * Ekv, gq = m->H / m->Hkv;
    bamd_step_state h; memset(&h, 0, sizeof h);
    h.pos_base = n_past; h.pos = n_past; h.n_ctx = c->n_ctx; h.step = T;
    h.n_kv = std::min(c->n_ctx, (n_past + T + 31) / 32 * 32);
    HIPC(hipMemcpyAsync(c->st, &h, sizeof h, hipMemcpyHostToDevice, s));
    if (m->with_embd) bamd_launch_embed_batch(c->forced, T, m->tok_embd.raw, m->tok_embd.type, E, m->V, c->bx, s);
    else HIPC(hipMemcpyAsync(c->bx, hidden_in, (size_t) T * E * 4, hipMemcpyDeviceToDevice, s));
    for (size_t il = 0; il < m->layers.size(); ++il) {
        const DevLayer & ly = m->layers[il];
        bamd_mm_args a; memset(&a, 0, sizeof a);
        // q,k,v                                                            (llama.cpp:8810-8835)
        // (the activation form of each mat-mul follows its weights: Q8_0 blocks for Q4_0 / Q5_0 / Q8_0, Q8_1 blocks for Q4_1 / Q5_1, else Q8_K; the load refused a QKV launch that would need both)
        // (one quantisation and one mat-mul per activation form: qkv_groups)
        bamd_mv_seg qs[3]; int gf[4]; uint32_t qr[3 + 2] = { 0 };
        const int ng = qkv_groups(qs, qkv_segments(ly, c->bqkv, qs, nullptr, qr), gf);
        for (int g = 0; g < ng; ++g) {
            bamd_launch_quantize_batch(c->bx, ly.attn_norm, m->eps, E, T, c->bblob, c->bblob16, s, bamd_act_form_of(qs[gf[g]].type), c->bbfr);
            memset(&a, 0, sizeof a);
            for (int i = gf[g]; i < gf[g + 1]; ++i) a.seg[a.nseg++] = qs[i];
            a.blob = c->bblob; a.K = E; a.T = T; a.ldo = ldq;
            if (batch_mm(c, a, BAMD_EPI_STORE, s, ly.aux_qkv + gf[g], qr[gf[g]], qr[gf[g] + 1], qr[gf[g] + 2])) return fail("batched mat-mul: unsupported shape");
        }
        // RoPE, KV store, attention with the T>1 semantics                  (llama.cpp:8837-8849, :8318-8353)
        bamd_attn_args t; memset(&t, 0, sizeof t);
        t.st = c->st; t.q = c->bqkv; t.k = c->bqkv + E; t.v = c->bqkv + E + Ekv; t.kc = c->kc[il]; t.vc = c->vc[il]; t.rope = c->rope; t.out = c->batt;
        t.hd = m->hd; t.Hkv = m->Hkv; t.n_ctx = c->n_ctx_pad; t.kq_scale = 1.0f / sqrtf((float) m->hd); t.prefill_mode = 1;
        t.batch = 1; t.ld_qkv = ldq; t.ld_out = E; t.lds_ld = attn_lds_ld(c, n_past + T - 1); t.batch_pos0p1 = n_past + 1;
        // the attention of the layer through the slice plan: one launch while the block (ensure_attn_scratch) holds the micro-batch's rows, token slices otherwise
        t.batch_scratch = c->attn_bscr;
        const size_t bud = attn_scratch_budget(), blk = bud && bud < c->attn_bscr_bytes ? bud : c->attn_bscr_bytes;   // (a budget lowered after the block grew still bounds the slices)
        if (bamd_launch_attention_batch(t, gq, T, s, 0, blk)) return fail("batched attention: unsupported head configuration");
        // x2 = x + Wo . att
        bamd_launch_quantize_batch(c->batt, nullptr, 0.f, E, T, c->bblob, c->bblob16, s, bamd_act_form_of(ly.wo.type), c->bbfr);
        memset(&a, 0, sizeof a);
        seg_of(a.seg[0], ly.wo, c->bx2); a.nseg = 1; a.blob = c->bblob; a.K = E; a.T = T; a.ldo = E; a.res = c->bx;
        { const void * ax[3] = { ly.aux_o, nullptr, nullptr }; if (batch_mm(c, a, BAMD_EPI_ADD, s, ax, ly.wo.bf16_range)) return fail("batched mat-mul: unsupported shape"); }
        // h = silu(Wg . a) * (Wu . a)
        bamd_launch_quantize_batch(c->bx2, ly.ffn_norm, m->eps, E, T, c->bblob, c->bblob16, s, bamd_act_form_of(ly.wg.type), c->bbfr);
        memset(&a, 0, sizeof a);
        seg_of(a.seg[0], ly.wg, c->bh); seg_of(a.seg[1], ly.wu, c->bh); a.nseg = 2; a.blob = c->bblob; a.K = E; a.T = T; a.ldo = F;
        { const void * ax[3] = { ly.aux_g, ly.aux_u, nullptr }; if (batch_mm(c, a, BAMD_EPI_SILU_MUL, s, ax, ly.wg.bf16_range, ly.wu.bf16_range)) return fail("batched mat-mul: unsupported shape"); }
        // x = x2 + Wd . h
        bamd_launch_quantize_batch(c->bh, nullptr, 0.f, F, T, c->bblob, c->bblob16, s, bamd_act_form_of(ly.wd.type), c->bbfr);
        memset(&a, 0, sizeof a);
        seg_of(a.seg[0], ly.wd, c->bx); a.nseg = 1; a.blob = c->bblob; a.K = F; a.T = T; a.ldo = E; a.res = c->bx2;
        { const void * ax[3] = { ly.aux_d, nullptr, nullptr }; if (batch_mm(c, a, BAMD_EPI_ADD, s, ax, ly.wd.bf16_range)) return fail("batched mat-mul: unsupported shape"); }
    }
    if (m->with_output) HIPC(hipMemcpyAsync(c->x, c->bx + (size_t) (T - 1) * E, (size_t) E * 4, hipMemcpyDeviceToDevice, s));
    else HIPC(hipMemcpyAsync(hidden_out, c->bx, (size_t) T * E * 4, hipMemcpyDeviceToDevice, s));
    return 0;
}

// a wo workgroup of a co-launch (bamd_colaunch.hip) that never saw the attention role's flags gave up instead of hanging: the results are void
// the give-up words of the kernels that wait inside a launch (attention || wo co-launch: word 0), copied behind
// the host logits by status_readback and checked once the stream has been synchronised.  A give-up invalidates that step only: the words are
// cleared after reporting, so the context stays usable.
static hipError_t status_readback(bamd_context * c, hipStream_t s) { return hipMemcpyAsync(c->logits_host + c->m->V, c->co_err, 32, hipMemcpyDeviceToHost, s); }
static int co_gave_up(bamd_context * c) {
    uint32_t w[8]; memcpy(w, c->logits_host + c->m->V, 32);
    if (!w[0]) return 0;
    hipMemsetAsync(c->co_err, 0, 32, c->stream);
    hipStreamSynchronize(c->stream);
    memset(c->logits_host + c->m->V, 0, 32);
    return fail("co-launched attention + wo: a workgroup gave up waiting for the attention role (results invalid)");
}
// the evaluation in front of this call (a bamd_decode without read-back) was not waited for: now that its stream has been, check what it left
static int settle_pending(bamd_context * c) { const bool was = c->status_pending; c->status_pending = false; return was ? co_gave_up(c) : 0; }
// a launch that the runtime rejected (LDS / grid beyond the device's limits, wrong architecture) leaves no other trace
static int launch_check() { const hipError_t le = hipGetLastError(); return le == hipSuccess ? 0 : fail(std::string("kernel launch failed: ") + hipGetErrorString(le)); }
// logits and give-up words of the evaluation enqueued on `s` to the host, wait for them, check the words
static int logits_to_host(bamd_context * c, hipStream_t s) {
    if (hipMemcpyAsync(c->logits_host, c->logits, (size_t) c->m->V * 4, hipMemcpyDeviceToHost, s) != hipSuccess) return fail("D2H logits");
    if (status_readback(c, s) != hipSuccess) return fail("D2H co-launch status");
    const hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(std::string("decode failed: ") + hipGetErrorString(e));
    return co_gave_up(c);
}
extern "C" __attribute__((visibility("default"))) int bamd_decode(bamd_context * c, const int32_t * tokens, int n_tokens, int n_past) {
    bamd_model * m = c->m;
    if (!m->with_embd || !m->with_output) return fail("bamd_decode needs a stage that owns embedding and output");
    if (!tokens || n_tokens < 1) return fail("n_tokens out of range");
    if (n_past < 0 || n_past > c->n_ctx - n_tokens) return fail("context overflow");
    if (n_tokens > BAMD_PREFILL_CAP && g_prefill_batch) {
        // llama_decode's n_ubatch split (llama.cpp:14615): micro-batches of 512, the logits are those of the last token
        for (int i = 0; i < n_tokens; i += BAMD_PREFILL_CAP)
            if (bamd_decode(c, tokens + i, std::min(BAMD_PREFILL_CAP, n_tokens - i), n_past + i)) return 1;
        return 0;
    }
    if (n_tokens > c->forced_cap) return fail("n_tokens out of range (token by token evaluation takes at most 4096 per call)");
    if (hipSetDevice(m->device) != hipSuccess) return fail("hipSetDevice");
    hipStream_t s = c->stream;
    if (c->cells.active && n_tokens > 1) return fail("after a context shift (bamd_kv_seq_add) tokens are evaluated one per call");
    if (!c->cells.active) c->n_cached = std::max(c->n_cached, n_past + n_tokens);
    if (hipMemcpyAsync(c->forced, tokens, (size_t) n_tokens * 4, hipMemcpyHostToDevice, s) != hipSuccess) return fail("H2D tokens");
    if (n_tokens > 1 && n_tokens <= BAMD_PREFILL_CAP && prefill_batch_supported(c, n_tokens, n_past, s)) {
        // one micro-batch: every layer once for all tokens (each weight record unpacked once per 8 tokens), lm_head for the last
        if (ensure_batch_buffers(c)) return 1;
        if (enqueue_prefill_batch(c, n_tokens, n_past, s)) return 1;
        if (enqueue_lm_head(c, s, nullptr)) return 1;                    // n_outputs = 1: last token only (llama.cpp:14580-14593)
    } else if (n_tokens == 1) {
        // single token: the captured stage-step graph (state and token are two small host copies, then one graph launch)
        if (bamd_stage_step(c, tokens[0], nullptr, n_past, nullptr, nullptr, 1, 0, s)) return 1;
    } else {
        if (set_state(c, n_past, s, false)) return 1;
        const int prefill_mode = n_tokens > 1;
        for (int t = 0; t < n_tokens; ++t) {
            enqueue_begin(c, n_tokens, 1, s);
            if (enqueue_layers(c, prefill_mode, s, nullptr, n_past + n_tokens)) return 1;
            if (t == n_tokens - 1 && enqueue_lm_head(c, s, nullptr)) return 1;
        }
    }
    if (launch_check()) return 1;
    c->logits_host_valid = c->logits_readback;
    if (!c->logits_readback) {
        if (status_readback(c, s) != hipSuccess) return fail("D2H co-launch status");
        // nothing of this evaluation is read on the host yet (bamd_set_logits_readback(c, 0): the sampler prefilter runs where the lm_head left the logits): do not wait
        // here — the caller's next synchronising call (bamd_logits_shortlist, bamd_get_logits) enqueues behind this evaluation, waits ONCE and checks the status words
        // then.  One host round trip per token instead of two (round 5: 2.31 -> 2.27 ms per token through the bridge at 7850 cached positions)
        c->status_pending = true;
        return 0;
    }
    return logits_to_host(c, s);
}
// a micro-batch of 2..512 prompt tokens through ONE layer-split stage (bamd_stage_step's batched counterpart): tokens (host) on the
// stage that owns the embedding, hidden_in_dev [n_tokens][n_embd] f32 elsewhere; hidden_out_dev [n_tokens][n_embd] on every stage but
// the last, which computes the logits of the last token when want_logits.  Returns 2 when the shape has no batched kernels (caller
// falls back to bamd_stage_step per token).
extern "C" __attribute__((visibility("default"))) int bamd_stage_prefill(bamd_context * c, const int32_t * tokens, int n_tokens, int n_past, const void * hidden_in_dev,
                                                                           void * hidden_out_dev, int want_logits, void * hip_stream) {
    bamd_model * m = c->m;
    HIPC(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t) hip_stream;
    if (n_tokens < 2 || n_tokens > BAMD_PREFILL_CAP || !prefill_batch_supported(c, n_tokens, n_past, s)) return 2;
    if (n_past < 0 || n_past + n_tokens > c->n_ctx) return fail("context overflow");
    if (c->cells.active) return fail("after a context shift (bamd_kv_seq_add) tokens are evaluated one per call");
    c->n_cached = std::max(c->n_cached, n_past + n_tokens);
    if (m->with_embd) { if (!tokens) return fail("bamd_stage_prefill: tokens required on the first stage"); HIPC(hipMemcpyAsync(c->forced, tokens, (size_t) n_tokens * 4, hipMemcpyHostToDevice, s)); }
    else if (!hidden_in_dev) return fail("bamd_stage_prefill: hidden_in required");
    if (!m->with_output && !hidden_out_dev) return fail("bamd_stage_prefill: hidden_out required");
    if (ensure_batch_buffers(c)) return 1;
    if (enqueue_prefill_batch(c, n_tokens, n_past, s, hidden_in_dev, hidden_out_dev)) return 1;
    if (m->with_output && want_logits && enqueue_lm_head(c, s, nullptr)) return 1;
    return launch_check();
}
extern "C" __attribute__((visibility("default"))) void bamd_set_prefill_batch(int on) { g_prefill_batch = on ? 1 : 0; g_prefill_mfma = on == 2 ? 0 : 1; }
extern "C" __attribute__((visibility("default"))) void bamd_set_attn_scratch_mb(int mb) { g_attn_scratch_mb = mb > 0 ? mb : 0; }
extern "C" __attribute__((visibility("default"))) const float * bamd_get_logits(bamd_context * c) {
    if (!c->logits_host_valid) {                                          // bamd_set_logits_readback(c, 0): copy on demand
        if (hipSetDevice(c->m->device) != hipSuccess) return nullptr;
        if (hipMemcpyAsync(c->logits_host, c->logits, (size_t) c->m->V * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return nullptr;
        if (hipStreamSynchronize(c->stream) != hipSuccess) return nullptr;
        if (settle_pending(c)) return nullptr;
        c->logits_host_valid = true;
    }
    return c->logits_host;
}
// waits for everything enqueued on the context's stream and reports what a bamd_decode without read-back left pending (the co-launch give-up words): the
// synchronisation point of a caller that evaluated without sampling afterwards (a request that stops during its prompt, or at n_ctx - 4)
extern "C" __attribute__((visibility("default"))) int bamd_synchronize(bamd_context * c) {
    HIPC(hipSetDevice(c->m->device));
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(std::string("bamd_synchronize: ") + hipGetErrorString(e));
    return settle_pending(c);
}
extern "C" __attribute__((visibility("default"))) void bamd_set_logits_readback(bamd_context * c, int on) { c->logits_readback = on != 0; }
extern "C" __attribute__((visibility("default"))) void * bamd_context_stream(bamd_context * c) { return (void *) c->stream; }
extern "C" __attribute__((visibility("default"))) int bamd_set_logits_test(bamd_context * c, const float * logits) {
    if (hipSetDevice(c->m->device) != hipSuccess) return 1;
    HIPC(hipMemcpy(c->logits, logits, (size_t) c->m->V * 4, hipMemcpyHostToDevice));
    c->logits_host_valid = false;
    return 0;
}

// ---- sampler prefilter (kernels in bamd_sampler.hip) --------------------------------------------------------
extern "C" __attribute__((visibility("default"))) int bamd_sampler_tables(bamd_context * c, const uint8_t * halve_class, const float * cutoff_of, int n_vocab) {
    bamd_model * m = c->m;
    if (n_vocab != m->V || !m->with_output) return fail("bamd_sampler_tables: needs the stage that owns the output layer, n_vocab of the model");
    if (hipSetDevice(m->device) != hipSuccess) return fail("hipSetDevice");
    if (!c->samp_cls) {
        const size_t out_bytes = sizeof(bamd_shortlist_head) + (size_t) BAMD_SHORTLIST_CAP * 8;
        if (dev_alloc(c->allocs, (void **) &c->samp_cls, (size_t) m->V) || dev_alloc(c->allocs, (void **) &c->samp_cut, (size_t) m->V * 4) ||
            dev_alloc(c->allocs, (void **) &c->samp_pen, sizeof(bamd_logit_penalty) * BAMD_PENALTY_CAP) || dev_alloc(c->allocs, (void **) &c->samp_out, out_bytes)) return 1;
        HIPC(hipHostMalloc((void **) &c->samp_pen_host, sizeof(bamd_logit_penalty) * BAMD_PENALTY_CAP));
        HIPC(hipHostMalloc((void **) &c->samp_out_host, out_bytes));
    }
    HIPC(hipMemcpy(c->samp_cls, halve_class, (size_t) m->V, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(c->samp_cut, cutoff_of, (size_t) m->V * 4, hipMemcpyHostToDevice));
    return 0;
}
extern "C" __attribute__((visibility("default"))) int bamd_logits_shortlist(bamd_context * c, const bamd_logit_penalty * pen, int n_pen, int halve,
                                                                            bamd_shortlist_head * head, int32_t * ids, float * vals, void * hip_stream) {
    bamd_model * m = c->m;
    if (!c->samp_cls) return fail("bamd_logits_shortlist before bamd_sampler_tables");
    if (n_pen < 0 || n_pen > BAMD_PENALTY_CAP) return fail("bamd_logits_shortlist: too many penalty entries");
    if (hipSetDevice(m->device) != hipSuccess) return fail("hipSetDevice");
    hipStream_t s = (hipStream_t) hip_stream;
    const size_t out_bytes = sizeof(bamd_shortlist_head) + (size_t) BAMD_SHORTLIST_CAP * 8;
    if (n_pen) {
        memcpy(c->samp_pen_host, pen, sizeof(bamd_logit_penalty) * (size_t) n_pen);
        HIPC(hipMemcpyAsync(c->samp_pen, c->samp_pen_host, sizeof(bamd_logit_penalty) * (size_t) n_pen, hipMemcpyHostToDevice, s));
    }
    bamd_shortlist_head * dh = (bamd_shortlist_head *) c->samp_out;
    int32_t * dids = (int32_t *) (c->samp_out + sizeof(bamd_shortlist_head));
    float * dvals = (float *) (c->samp_out + sizeof(bamd_shortlist_head) + (size_t) BAMD_SHORTLIST_CAP * 4);
    bamd_launch_sampler_shortlist(c->logits, c->samp_pen, n_pen, c->samp_cls, halve, c->samp_cut, m->V, dh, dids, dvals, BAMD_SHORTLIST_CAP, s);
    c->logits_host_valid = false;
    HIPC(hipMemcpyAsync(c->samp_out_host, c->samp_out, out_bytes, hipMemcpyDeviceToHost, s));
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(std::string("sampler prefilter failed: ") + hipGetErrorString(e));
    if (settle_pending(c)) return 1;
    memcpy(head, c->samp_out_host, sizeof *head);
    const int n = std::min(std::max(head->count, 0), BAMD_SHORTLIST_CAP);
    memcpy(ids, c->samp_out_host + sizeof(bamd_shortlist_head), (size_t) n * 4);
    memcpy(vals, c->samp_out_host + sizeof(bamd_shortlist_head) + (size_t) BAMD_SHORTLIST_CAP * 4, (size_t) n * 4);
    return 0;
}

extern "C" __attribute__((visibility("default"))) int bamd_generate_greedy(bamd_context * c, int n_past, int n_steps, int32_t * out_tokens, float * elapsed_ms) {
    bamd_model * m = c->m;
    if (!m->with_embd || !m->with_output) return fail("bamd_generate_greedy needs a stage that owns embedding and output");
    if (n_steps < 1 || n_past < 1 || n_past + n_steps > c->n_ctx || n_steps + 1 > c->out_cap) return fail("bad n_past / n_steps");
    HIPC(hipSetDevice(m->device));
    hipStream_t s = c->stream;
    int attn_hi = n_past + n_steps;
    if (c->cells.active) {
        // cells no longer follow positions (context shift / Self-Extend): the reference keeps generating at full speed (cpp/bridge.cpp:487-503).
        // llama_kv_cache_find_slot depends on the cell metadata only, not on the tokens: run it for all n_steps here and hand the device loop
        // the cell and the padded KV length of every step (step_begin_kernel); pending rotations first (llama_kv_cache_update)
        if (kv_update(c, s)) return 1;
        if (c->slots_cap < n_steps) {
            if (dev_alloc(c->allocs, (void **) &c->slots, (size_t) c->out_cap * 8)) return 1;
            c->slots_cap = c->out_cap;
            drop_replays(c);                                              // (captured with the old pointer)
        }
        std::vector<int32_t> hs((size_t) n_steps * 2);
        for (int t = 0; t < n_steps; ++t) {
            int cell = 0, n_kv = 0;
            if (kv_find_slot(c, n_past + t, &cell, &n_kv)) return 1;
            hs[(size_t) 2 * t] = cell; hs[(size_t) 2 * t + 1] = n_kv; attn_hi = std::max(attn_hi, n_kv - 1);
        }
        HIPC(hipMemcpyAsync(c->slots, hs.data(), hs.size() * 4, hipMemcpyHostToDevice, s));
        HIPC(hipStreamSynchronize(s));                                    // (hs is a host temporary)
    } else c->n_cached = std::max(c->n_cached, n_past + n_steps);
    const ReplayKey key = { attn_path(c, attn_hi) };
    auto enqueue = [&] { enqueue_begin(c, 0, 1, s, c->cells.active); return enqueue_step(c, s, attn_hi); };   // state on the device; the slot table when the cells are tracked
    float ms_steps = 0.f;
    EventPair ev; bool timed_by_events = false;
    // AQL packets on the library's own queue where the attention path allows it, else one hipGraph launch per step on the context's stream
    StepReplay & own = c->greedy_aql;
    const bool want_aql = aql_allowed(c, key.path);
    if (want_aql) own.reset_unless(key); else own.reset();
    if (want_aql && !own.aql) { own.aql = record_aql(c, enqueue); own.key = key; }
    if (own.aql) {
        if (set_state(c, n_past, s, true)) return 1;
        HIPC(hipStreamSynchronize(s));                                // the state and everything before it is in memory: the first packet acquires at system scope
        double sec = 0.0; const char * why = nullptr;
        if (bamd_aql_run(own.aql, n_steps, &sec, &why)) return fail(std::string("own AQL queue: ") + (why ? why : "?"));
        ms_steps = (float) (sec * 1e3); c->aql_runs += 1;
    } else {
        StepReplay & g = c->greedy_graph;
        g.reset_unless(key);
        if (!g.exec && capture_graph(s, enqueue, &g.exec, { "hipStreamEndCapture: ", "hipGraphInstantiate: " })) return 1;
        g.key = key;
        if (set_state(c, n_past, s, true)) return 1;
        HIPC(ev.create()); timed_by_events = true;
        HIPC(hipEventRecord(ev.a, s));
        for (int t = 0; t < n_steps; ++t) HIPC(hipGraphLaunch(g.exec, s));
        HIPC(hipEventRecord(ev.b, s));
    }
    enqueue_begin(c, 0, 0, s);                                        // flush the last arg-max into out_tokens
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(out_tokens, c->out_tokens, (size_t) (n_steps + 1) * 4, hipMemcpyDeviceToHost, s));
    if (logits_to_host(c, s)) return 1;
    c->logits_host_valid = true;
    if (timed_by_events) HIPC(hipEventElapsedTime(&ms_steps, ev.a, ev.b));
    if (elapsed_ms) *elapsed_ms = ms_steps;
    return 0;
}
// how many bamd_generate_greedy calls of this context ran on the own AQL queue so far (tests, bench: which path produced the number)
extern "C" __attribute__((visibility("default"))) int bamd_aql_runs(const bamd_context * c) { return c->aql_runs + c->aql_steps; }

// ---- layer-split stage ---------------------------------------------------------------------------------
// Is this bamd_stage_step call the one the own AQL queue (bamd_aql.h) serves: the whole single-stage step — state from a pinned host inbox, layers, lm_head — as
// packets with fence scope NONE, one host wait at its end?  That is the caller that owns embedding and output, feeds host tokens on the context's own stream and
// wants the logits (bamd_decode from the bridge's token loop); layer-split stages, device-side tokens, shifted cells and prefill-mode steps keep the stage graphs
static bool step_from_inbox(const bamd_context * c, const void * token_dev, const void * hidden_in_dev, const void * hidden_out_dev, int want_logits, int prefill_mode, hipStream_t s) {
    const bamd_model * m = c->m;
    return m->with_embd && m->with_output && !token_dev && !hidden_in_dev && !hidden_out_dev && want_logits && !prefill_mode && !c->cells.active && s == c->stream && s != nullptr;
}
static bool have_inbox(bamd_context * c) {                 // the pinned host block that step_begin_kernel reads the state of such a step from (allocated at the first one)
    if (!c->inbox && hipHostMalloc((void **) &c->inbox, sizeof(bamd_step_state)) != hipSuccess) { (void) hipGetLastError(); c->inbox = nullptr; }
    return c->inbox != nullptr;
}
extern "C" __attribute__((visibility("default"))) int bamd_stage_step(bamd_context * c, int32_t token, const void * token_dev, int pos, const void * hidden_in_dev,
                               void * hidden_out_dev, int want_logits, int prefill_mode, void * hip_stream) {
    bamd_model * m = c->m;
    HIPC(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t) hip_stream;            // NULL = the HIP default (null) stream, as for any HIP API
    if (pos < 0 || pos >= c->n_ctx) return fail("position out of range");
    const ReplayKey own_key = { attn_path(c, pos) };
    if (step_from_inbox(c, token_dev, hidden_in_dev, hidden_out_dev, want_logits, prefill_mode, s) && aql_allowed(c, own_key.path) && have_inbox(c)) {
        StepReplay & own = c->step_aql;
        own.reset_unless(own_key);
        if (!own.aql) {
            own.aql = record_aql(c, [&] {
                bamd_launch_step_begin(c->st, c->forced, 1, c->out_tokens, m->tok_embd.raw, m->tok_embd.type, m->E, m->V, c->x, 1, s, nullptr, nullptr, c->rope, c->rope_cur, m->hd, c->inbox);
                return enqueue_step(c, s, pos);
            });
            own.key = own_key;
        }
        if (own.aql) {
            if (next_serial(c, s)) return 1;
            c->n_cached = std::max(c->n_cached, pos + 1);
            HIPC(hipStreamSynchronize(s));                               // whatever this context enqueued before (a prompt micro-batch nobody waited for) is done
            bamd_step_state * in = c->inbox;
            memset(in, 0, sizeof *in);
            in->pos_base = pos; in->n_ctx = c->n_ctx; in->serial = c->host_serial; in->token = token;
            const char * why = nullptr;
            if (bamd_aql_run(own.aql, 1, nullptr, &why)) return fail(std::string("own AQL queue: ") + (why ? why : "?"));
            c->aql_steps += 1;
            return 0;
        }
    }
    // state for exactly this token: pos_base = pos, step = 0, one forced token (from the host, or from a device int32)
    if (next_serial(c, s)) return 1;
    bamd_step_state h; memset(&h, 0, sizeof h); h.pos_base = pos; h.n_ctx = c->n_ctx; h.serial = c->host_serial;
    int attn_hi = pos;                                   // what decides single-launch vs three-launch attention
    if (c->cells.active) {
        if (prefill_mode) return fail("after a context shift (bamd_kv_seq_add) tokens are evaluated one per call");
        int cell = 0, n_kv = 0;
        if (kv_update(c, s) || kv_find_slot(c, pos, &cell, &n_kv)) return 1;
        h.cell_plus1 = cell + 1; h.n_kv_fixed = n_kv; attn_hi = n_kv - 1;
        HIPC(hipMemcpyAsync(c->cellpos + cell, &c->cells.pos[(size_t) cell], 4, hipMemcpyHostToDevice, s));
    } else c->n_cached = std::max(c->n_cached, pos + 1);
    HIPC(hipMemcpyAsync(c->st, &h, sizeof h, hipMemcpyHostToDevice, s));
    const int32_t * forced = c->forced;
    if (token_dev) forced = (const int32_t *) token_dev;
    else HIPC(hipMemcpyAsync(c->forced, &token, 4, hipMemcpyHostToDevice, s));
    // everything after the two small host copies is a fixed launch sequence for given pointers: replay it as one hipGraph
    // (a stage of 4 layers is ~22 launches at ~8 us of host time each; the layer-split pipeline is host-bound without this)
    auto enqueue = [&]() -> int {
        if (m->with_embd) bamd_launch_step_begin(c->st, forced, 1, c->out_tokens, m->tok_embd.raw, m->tok_embd.type, m->E, m->V, c->x, 1, s, nullptr, nullptr, c->rope, c->rope_cur, m->hd);
        else {
            // no embedding on this stage: still advance the device state (pos, n_kv), then take the hidden state
            bamd_launch_step_begin(c->st, c->forced, 0, c->out_tokens, nullptr, BAMD_F32, 0, m->V, c->x, 1, s, nullptr, nullptr, c->rope, c->rope_cur, m->hd);
            HIPC(hipMemcpyAsync(c->x, hidden_in_dev, (size_t) m->E * 4, hipMemcpyDeviceToDevice, s));
        }
        if (enqueue_layers(c, prefill_mode, s, nullptr, attn_hi)) return 1;
        if (m->with_output) { if (want_logits && enqueue_lm_head(c, s, nullptr)) return 1; }
        else HIPC(hipMemcpyAsync(hidden_out_dev, c->x, (size_t) m->E * 4, hipMemcpyDeviceToDevice, s));
        return 0;
    };
    if (!g_stage_graph || s == nullptr) return enqueue() ? 1 : launch_check();   // the legacy default stream cannot be captured
    StepReplay & sg = c->stage_graph[want_logits ? 1 : 0][prefill_mode ? 1 : 0];
    const ReplayKey key = { attn_path(c, attn_hi), forced, hidden_in_dev, hidden_out_dev };
    sg.reset_unless(key);
    if (!sg.exec && capture_graph(s, enqueue, &sg.exec, { "stage graph capture: ", "stage graph instantiate: " })) return 1;
    sg.key = key;
    HIPC(hipGraphLaunch(sg.exec, s));
    return 0;
}
// write the arg-max token of the last lm_head of this (last) stage into a device int32 — no host round trip
extern "C" __attribute__((visibility("default"))) int bamd_stage_token_to(bamd_context * c, void * token_dev, void * hip_stream) {
    hipStream_t s = (hipStream_t) hip_stream;
    bamd_model * m = c->m;
    HIPC(hipSetDevice(m->device));
    // flush-only step_begin: decodes best_key into out_tokens[n_out]; n_out was reset to 0 by bamd_stage_step
    bamd_launch_step_begin(c->st, c->forced, 0, c->out_tokens, nullptr, BAMD_F32, 0, m->V, c->x, 0, s);
    HIPC(hipMemcpyAsync(token_dev, c->out_tokens, 4, hipMemcpyDeviceToDevice, s));
    return 0;
}
extern "C" __attribute__((visibility("default"))) int bamd_stage_argmax(bamd_context * c, void * hip_stream, int32_t * token) {
    hipStream_t s = (hipStream_t) hip_stream;
    HIPC(hipSetDevice(c->m->device));
    bamd_step_state h;
    HIPC(hipMemcpyAsync(&h, c->st, sizeof h, hipMemcpyDeviceToHost, s));
    HIPC(status_readback(c, s));
    HIPC(hipStreamSynchronize(s));
    if (co_gave_up(c)) return 1;                                      // the stage graphs take the co-launch / engine paths as well
    *token = (int32_t) (0xffffffffu - (uint32_t) (h.best_key & 0xffffffffull));
    return 0;
}

// host logits of the last bamd_stage_step(want_logits=1) on the last stage; synchronises `hip_stream`
extern "C" __attribute__((visibility("default"))) const float * bamd_stage_get_logits(bamd_context * c, void * hip_stream) {
    hipStream_t s = (hipStream_t) hip_stream;
    if (hipSetDevice(c->m->device) != hipSuccess) return nullptr;
    return logits_to_host(c, s) ? nullptr : c->logits_host;
}
// raw GGUF access for the tokenizer side of the bridge
const GgufFile * bamd_model_gguf(const bamd_model * m) { return m->file.get(); }
extern "C" __attribute__((visibility("default"))) int bamd_model_device(const bamd_model * m) { return m->device; }

// ---- measurement -----------------------------------------------------------------------------------------
// one eager step at position pos with a HIP event pair around every launch; per launch kind (StepTimer::begin) the launch count, the summed
// event time and the summed algorithmic bytes; entry 7 = what an EMPTY event pair reads on this stream (median of 9)
extern "C" __attribute__((visibility("default"))) int bamd_profile_step_kinds(bamd_context * c, int pos, int * launches, double * ms, double * bytes) {
    bamd_model * m = c->m;
    if (!m->with_embd || !m->with_output) return fail("profile needs a full single-stage model");
    HIPC(hipSetDevice(m->device));
    hipStream_t s = c->stream;
    int32_t tok = 1;
    HIPC(hipMemcpyAsync(c->forced, &tok, 4, hipMemcpyHostToDevice, s));
    if (set_state(c, pos, s, false)) return 1;
    StepTimer tm; tm.on = true;
    tm.begin(s, 2, 0.0); enqueue_begin(c, 1, 1, s); tm.end(s);
    if (enqueue_layers(c, 0, s, &tm, pos)) return 1;
    if (enqueue_lm_head(c, s, &tm)) return 1;
    HIPC(hipStreamSynchronize(s));
    for (int i = 0; i < 8; ++i) { launches[i] = 0; ms[i] = 0; bytes[i] = 0; }
    const int n_kv = std::min(c->n_ctx, (pos + 1 + 31) / 32 * 32);
    for (size_t i = 0; i < tm.cls.size(); ++i) {
        float t = 0.f; hipEventElapsedTime(&t, tm.ev[2 * i], tm.ev[2 * i + 1]);
        const int k = tm.kind[i];
        launches[k] += 1; ms[k] += t;
        bytes[k] += tm.cls[i] == 1 ? (double) n_kv * m->Hkv * m->hd * 2 * 2 : tm.bytes[i];
    }
    for (auto e : tm.ev) hipEventDestroy(e);
    {
        std::vector<float> ov;
        for (int i = 0; i < 9; ++i) {
            EventPair e; e.create();
            hipEventRecord(e.a, s); hipEventRecord(e.b, s); hipStreamSynchronize(s);
            float t = 0.f; hipEventElapsedTime(&t, e.a, e.b); ov.push_back(t);
        }
        std::sort(ov.begin(), ov.end());
        launches[7] = 9; ms[7] = ov[4]; bytes[7] = 0;
    }
    return 0;
}
// the same folded into three classes: [0] all mat-vec launches, [1] attention, [2] other, [3] the empty event pair
extern "C" __attribute__((visibility("default"))) int bamd_profile_step(bamd_context * c, int pos, int * launches, double * ms, double * bytes) {
    int l[8]; double t[8], b[8];
    if (bamd_profile_step_kinds(c, pos, l, t, b)) return 1;
    for (int i = 0; i < 4; ++i) { launches[i] = 0; ms[i] = 0; bytes[i] = 0; }
    const int cls_of[7] = { 0, 1, 2, 0, 0, 0, 0 };
    for (int k = 0; k < 7; ++k) { launches[cls_of[k]] += l[k]; ms[cls_of[k]] += t[k]; bytes[cls_of[k]] += b[k]; }
    launches[3] = l[7]; ms[3] = t[7]; bytes[3] = 0;
    return 0;
}

// Phase stamps of one decode step at position `pos` (BAMD_TIMING builds only): the step is captured into a hipGraph whose launches
// carry their stamp blocks, replayed `replays` times back to back (each replay overwrites the stamps: the last one is read), and the
// blocks are copied to `out` ([n_launches][BAMD_TL_SLOT_WORDS] u64, launch order: per layer qkv (one launch per activation form: two in a layer whose
// QKV mixes them, qkv_recipe_mix), attention, wo, gate/up, down; then lm_head).  100 MHz device wall clock.  *n_launches receives the number of stamped launches.
extern "C" __attribute__((visibility("default"))) int bamd_timeline_step(bamd_context * c, int pos, int replays, unsigned long long * out, int cap_launches, int * n_launches) {
    bamd_model * m = c->m;
    if (!bamd_timing_enabled()) return fail("bamd_timeline_step: library built without -DBAMD_TIMING (use booster_amd/lib/libbooster_amd_timing.so)");
    if (!m->with_embd || !m->with_output) return fail("timeline needs a full single-stage model");
    HIPC(hipSetDevice(m->device));
    hipStream_t s = c->stream;
    int cap = 1;
    for (const DevLayer & ly : m->layers) cap += 4 + qkv_launches(ly);
    if (cap > cap_launches) return fail("bamd_timeline_step: output buffer too small");
    const size_t bytes = (size_t) cap * BAMD_TL_SLOT_WORDS * 8;
    OwnedDevMem mem;
    HIPC(hipMalloc(&mem.p, bytes));
    unsigned long long * buf = (unsigned long long *) mem.p;
    HIPC(hipMemsetAsync(buf, 0, bytes, s));
    int32_t tok = 1;
    HIPC(hipMemcpyAsync(c->forced, &tok, 4, hipMemcpyHostToDevice, s));
    c->tl_base = buf; c->tl_slot = 0; c->tl_cap = cap;
    OwnedGraphExec ge;
    const int rc = capture_graph(s, [&] { enqueue_begin(c, 1, 1, s); return enqueue_step(c, s, pos); }, &ge.g, { "timeline capture failed", "timeline graph instantiate failed" });
    *n_launches = c->tl_slot;
    c->tl_base = nullptr; c->tl_slot = 0; c->tl_cap = 0;             // on every exit: the stamps belong to this call's buffer
    if (rc) return rc;
    for (int r = 0; r < replays; ++r) {
        if (set_state(c, pos, s, false)) return 1;
        HIPC(hipGraphLaunch(ge.g, s));
    }
    HIPC(hipStreamSynchronize(s));
    HIPC(hipMemcpy(out, buf, (size_t) *n_launches * BAMD_TL_SLOT_WORDS * 8, hipMemcpyDeviceToHost));
    return 0;
}
