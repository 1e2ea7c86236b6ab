"""booster_amd — Python host side above the C-ABI of libbooster_amd.so (include/bamd.h, include/booster_bridge.h).

The reference's host language is Go (pkg/server, cgo); Go is not in this image, so this thin ctypes layer plays
the host role for tests, bench and multi-process layer split.  It contains NO compute: every number comes out
of the HIP library, and loading fails loudly if that library is missing.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BAMD_LIB") or os.path.join(_HERE, "lib", "libbooster_amd.so")   # BAMD_LIB: experiment builds (tools/)
_lib = None

F32, F16, Q4_K, Q5_K, Q6_K = 0, 1, 12, 13, 14
Q2_K, Q3_K = 10, 11
IQ4_NL = 20
IQ4_XS = 23


class BamdError(RuntimeError):
    pass


class LogitPenalty(C.Structure):
    """bamd_logit_penalty (include/bamd.h): one distinct penalised token of the sampler prefilter"""
    _fields_ = [("id", C.c_int32), ("count", C.c_int32), ("kind", C.c_int32), ("f", C.c_float), ("d", C.c_double), ("pre", C.c_double)]


class ShortlistHead(C.Structure):
    """bamd_shortlist_head (include/bamd.h)"""
    _fields_ = [("top_key", C.c_ulonglong), ("count", C.c_int32), ("ntop", C.c_int32), ("nan", C.c_int32), ("top_id", C.c_int32),
                ("top_logit", C.c_float), ("cutoff", C.c_float)]


PENALTY_DTYPE = np.dtype(LogitPenalty)         # numpy view of a penalty list: fields id, count, kind, f, d, pre
SHORTLIST_CAP = 1024                           # BAMD_SHORTLIST_CAP
PENALTY_CAP = 512                              # BAMD_PENALTY_CAP
SHORTLIST_SENTINEL_ID = -1                     # what Context.logits_shortlist leaves in the ids / vals the library did not write
SHORTLIST_SENTINEL_BITS = 0x7FC5A5A5


def lib():
    """The HIP library.  No fallback: a missing .so is an error (run `python -m booster_amd.build`)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BamdError("libbooster_amd.so is not built (python -m booster_amd.build); there is no CPU fallback")
        # PyTorch bundles its own libamdhip64.so.7; two HIP runtimes in one process cannot both own the GPU, and the
        # first one loaded wins the SONAME.  Import torch first so that both sides share torch's runtime.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        vp, ci, cf, i64 = C.c_void_p, C.c_int, C.c_float, C.c_int64
        L.bamd_last_error.restype = C.c_char_p
        L.bamd_model_load.restype = vp; L.bamd_model_load.argtypes = [C.c_char_p, ci, ci, ci, ci, ci]
        L.bamd_model_free.argtypes = [vp]
        for n in ("bamd_model_n_vocab", "bamd_model_n_embd", "bamd_model_n_layer", "bamd_model_n_ctx_train"):
            getattr(L, n).argtypes = [vp]
        L.bamd_model_weight_bytes.restype = i64; L.bamd_model_weight_bytes.argtypes = [vp]
        L.bamd_model_tensor_raw.restype = i64; L.bamd_model_tensor_raw.argtypes = [vp, C.c_char_p, vp, i64]
        L.bamd_context_new.restype = vp; L.bamd_context_new.argtypes = [vp, ci]
        L.bamd_context_free.argtypes = [vp]
        L.bamd_n_ctx.argtypes = [vp]
        L.bamd_kv_cache_clear.argtypes = [vp]
        L.bamd_decode.argtypes = [vp, vp, ci, ci]
        L.bamd_get_logits.restype = C.POINTER(C.c_float); L.bamd_get_logits.argtypes = [vp]
        L.bamd_generate_greedy.argtypes = [vp, ci, ci, vp, C.POINTER(C.c_float)]
        L.bamd_kv_seq_rm.argtypes = [vp, ci, ci]; L.bamd_kv_seq_add.argtypes = [vp, ci, ci, ci]; L.bamd_kv_seq_div.argtypes = [vp, ci, ci, ci]
        L.bamd_stage_step.argtypes = [vp, C.c_int32, vp, ci, vp, vp, ci, ci, vp]
        L.bamd_stage_token_to.argtypes = [vp, vp, vp]
        L.bamd_stage_prefill.argtypes = [vp, vp, ci, ci, vp, vp, ci, vp]
        L.bamd_stage_argmax.argtypes = [vp, vp, C.POINTER(C.c_int32)]
        L.bamd_profile_step.argtypes = [vp, ci, vp, vp, vp]; L.bamd_profile_step_kinds.argtypes = [vp, ci, vp, vp, vp]
        L.bamd_timeline_step.argtypes = [vp, ci, ci, vp, ci, C.POINTER(ci)]
        L.bamd_set_prefill_batch.argtypes = [ci]; L.bamd_set_prefill_batch.restype = None
        for n in ("lowbit", "q0", "q1", "nl", "flt", "bf16"):                 # the switches of csrc/bamd_prefill_family.h
            getattr(L, "bamd_set_prefill_" + n).argtypes = [ci]; getattr(L, "bamd_set_prefill_" + n).restype = None
        L.bamd_set_attn_scratch_mb.argtypes = [ci]; L.bamd_set_attn_scratch_mb.restype = None
        L.bamd_attention_batch_plan.argtypes = [ci, ci, ci, ci, ci, ci, C.c_size_t, C.POINTER(ci), C.POINTER(ci), C.POINTER(C.c_size_t)]
        L.bamd_prefill_mfma_runs.argtypes = [ci]; L.bamd_prefill_mfma_runs.restype = C.c_longlong
        L.bamd_prefill_bf16_fallback_tiles.argtypes = []; L.bamd_prefill_bf16_fallback_tiles.restype = C.c_ulonglong
        L.bamd_model_prefill_aux_bytes.argtypes = [vp]; L.bamd_model_prefill_aux_bytes.restype = i64
        L.bamd_bench_matvec.argtypes = [ci, ci, ci, ci, ci, ci, ci, C.POINTER(C.c_float)]
        L.bamd_op_quantize_q8_K.argtypes = [vp, i64, vp, cf, vp]
        L.bamd_op_quantize_q8_0.argtypes = [vp, i64, vp, cf, vp]
        L.bamd_op_quantize_q8_1.argtypes = [vp, i64, vp, cf, vp]
        L.bamd_op_act_bf16.argtypes = [vp, i64, vp, cf, vp]
        L.bamd_op_mul_mat_vec.argtypes = [ci, vp, ci, ci, vp, vp, cf, vp, vp, ci]
        L.bamd_op_mul_mat_vec_argmax.argtypes = [ci, vp, ci, ci, vp, vp, cf, vp, ci, C.POINTER(C.c_int32)]
        L.bamd_op_ffn_gate_up.argtypes = [ci, vp, vp, ci, ci, vp, vp, cf, vp]
        L.bamd_op_mul_mat_batch.argtypes = [ci, vp, ci, ci, vp, ci, vp, cf, vp, vp, ci]
        L.bamd_op_get_row.argtypes = [ci, vp, ci, ci, ci, vp]
        L.bamd_op_attention.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp]
        L.bamd_op_attention_batch.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp]
        L.bamd_op_attention_batch_ex.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, C.c_size_t, vp, C.POINTER(ci)]
        L.bamd_op_rope_row.argtypes = [ci, ci, cf, cf, vp, vp]
        L.bamd_op_k_shift.argtypes = [vp, ci, ci, ci, vp, cf, cf, vp, cf, cf, ci]
        L.bamd_op_attention_cells.argtypes = [vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp]
        L.bamd_op_fused_qkv.argtypes = [ci, vp, vp, vp, ci, vp, vp, cf, ci, vp]
        L.bamd_op_mul_mat_batch_seg.argtypes = [ci, vp, vp, vp, ci, vp, ci, vp, cf, ci, vp, ci, ci, vp]
        L.bamd_op_attention_wo.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, ci, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp]
        L.bamd_trace_matvec.argtypes = [ci, vp, vp, ci, ci, ci, ci, ci, vp]
        L.bamd_trace_mv.argtypes = [ci, vp, vp, ci, ci, ci, ci, ci, vp]
        L.bamd_trace_attn_wo.argtypes = [ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, vp]
        L.bamd_set_aql.argtypes = [ci]; L.bamd_set_aql.restype = None
        L.bamd_aql_runs.argtypes = [vp]
        L.bamd_set_aql_stall_ms.argtypes = [ci]; L.bamd_set_aql_stall_ms.restype = None
        L.bamd_aql_stats.argtypes = [ci, C.POINTER(C.c_uint64)]; L.bamd_aql_stats.restype = None
        L.bamd_context_stream.restype = vp; L.bamd_context_stream.argtypes = [vp]
        L.bamd_set_logits_readback.argtypes = [vp, ci]; L.bamd_set_logits_readback.restype = None
        L.bamd_set_logits_test.argtypes = [vp, vp]
        L.bamd_sampler_tables.argtypes = [vp, vp, vp, ci]
        L.bamd_logits_shortlist.argtypes = [vp, vp, ci, ci, C.POINTER(ShortlistHead), vp, vp, vp]
        _lib = L
    return _lib


def _chk(rc):
    if rc != 0:
        raise BamdError(lib().bamd_last_error().decode())


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def set_prefill_batch(on):
    """True (default): prompts of 2..512 tokens go through the batched prefill kernels; False: token by token (same bits)."""
    lib().bamd_set_prefill_batch(int(on))      # 2: batched without the MFMA kernel


def set_prefill_lowbit(on):
    """True: models loaded from now on build side tables for their Q3_K / Q2_K matrices and evaluate prompts on the matrix-core kernels; False (default, also
    env BAMD_PREFILL_LOWBIT): a model that holds such a matrix evaluates prompts on the integer-dot kernel.  Same bits either way."""
    lib().bamd_set_prefill_lowbit(int(bool(on)))


def set_prefill_q0(on):
    """True: models loaded from now on build side tables for their Q8_0 / Q4_0 / Q5_0 layer matrices and evaluate prompts on the matrix-core kernel of these types;
    False (default, also env BAMD_PREFILL_Q0): such a model evaluates prompts on the integer-dot kernel.  Same bits either way."""
    lib().bamd_set_prefill_q0(int(bool(on)))


def set_prefill_q1(on):
    """True: models loaded from now on build side tables for their Q4_1 / Q5_1 layer matrices and evaluate prompts on the matrix-core kernel of these types;
    False (default, also env BAMD_PREFILL_Q1): such a model evaluates prompts on the integer-dot kernel.  Independent of set_prefill_q0: a Q4_0 / Q5_0 file made
    with an importance matrix holds Q4_1 / Q5_1 ffn_down matrices and needs both switches on to get tables.  Same bits either way."""
    lib().bamd_set_prefill_q1(int(bool(on)))


def set_prefill_nl(on):
    """True: models loaded from now on build side tables for their IQ4_NL layer matrices and evaluate prompts on the matrix-core kernel of the type; False
    (default, also env BAMD_PREFILL_NL): such a model evaluates prompts on the integer-dot kernel.  Independent of the other switches: a model that also holds
    a Q8_0 / Q4_0 / Q5_0 or Q4_1 / Q5_1 layer matrix needs that family's switch as well to get tables.  Same bits either way."""
    lib().bamd_set_prefill_nl(int(bool(on)))


def set_prefill_flt(on):
    """True: F32 / F16 matrices evaluate prompts on the f32 matrix-core kernel; False (default, also env BAMD_PREFILL_FLT): on the VALU kernel.  Read at each
    launch, not at model load (the kernel needs no side tables), so it also applies to models loaded before.  BF16 matrices: set_prefill_bf16.  Same bits
    either way."""
    lib().bamd_set_prefill_flt(int(bool(on)))


def set_prefill_bf16(on):
    """True: BF16 matrices evaluate prompts on the f32 matrix-core kernel (fma chains where the exponent ranges of the matrix and of the tokens prove every
    product exact in f32, the two-rounding VALU step per workgroup otherwise); False (default, also env BAMD_PREFILL_BF16): on the VALU kernel.  Independent of
    set_prefill_flt and read at each launch like it.  Same bits either way."""
    lib().bamd_set_prefill_bf16(int(bool(on)))


def prefill_bf16_fallback_tiles():
    """tests and tools: workgroups of the BF16 matrix-core kernel that took the two-rounding VALU step since the library was loaded (waits for the device)"""
    return int(lib().bamd_prefill_bf16_fallback_tiles())


def set_attn_scratch_mb(mb):
    """budget in MiB of a context's batched-attention scratch block (also env BAMD_ATTN_SCRATCH_MB); 0 = the default, H x 512 x 18432 x 4 bytes.  A micro-batch whose
    score rows exceed it is attended in token slices that reuse the block.  Same bits at every setting."""
    lib().bamd_set_attn_scratch_mb(int(mb))


def attention_batch_plan(Hkv, gq, hd, T, ld, impl=0, budget_bytes=0):
    """the slice plan of a micro-batch's attention (host only): (tokens per slice, slices, scratch bytes), or None where there is no plan"""
    tps, ns, sb = C.c_int(0), C.c_int(0), C.c_size_t(0)
    if lib().bamd_attention_batch_plan(Hkv, gq, hd, T, ld, impl, budget_bytes, C.byref(tps), C.byref(ns), C.byref(sb)) != 0:
        return None
    return tps.value, ns.value, sb.value


def prefill_mfma_runs(t):
    """matrix-core prompt mat-mul launches of weight type t (GGUF type id) since the library was loaded"""
    return int(lib().bamd_prefill_mfma_runs(int(t)))


def set_aql(on):
    """True (default): Context.generate_greedy replays the step as AQL packets with fence scope NONE on the library's own HSA queue (csrc/bamd_aql.h) where it
    can; False: one hipGraph per step on the context's HIP stream.  Same kernels, same bits.  Takes effect at the next generate_greedy call."""
    lib().bamd_set_aql(int(bool(on)))


def set_aql_stall_ms(ms):
    """the own queue's stall limit in ms: a run fails once the queue's read index has not moved for that long, however long the run itself takes.  ms <= 0 restores
    the default, 60 000.  Takes effect at the next run.  A test hook."""
    lib().bamd_set_aql_stall_ms(int(ms))


def aql_stats(device=0):
    """counters of the device's own queue since the library was loaded: packets written, room_waits (replays that found the ring full at least once before they
    were written), wrap_doorbells (extra doorbells at the ring's last slot inside a replay) and the ring size; all 0 where the own queue is off or unavailable"""
    out = (C.c_uint64 * 4)()
    lib().bamd_aql_stats(int(device), out)
    return {"packets": int(out[0]), "room_waits": int(out[1]), "wrap_doorbells": int(out[2]), "ring": int(out[3])}


def device_count():
    return lib().bamd_device_count()


class Model:
    """llama_model analogue: one layer-split stage of a GGUF Llama model resident on one GPU."""

    def __init__(self, path, device=0, layer_first=0, layer_last=-1, with_embd=True, with_output=True):
        self.h = lib().bamd_model_load(os.fsencode(path), device, layer_first, layer_last, int(with_embd), int(with_output))
        if not self.h:
            raise BamdError(lib().bamd_last_error().decode())
        self.n_vocab = lib().bamd_model_n_vocab(self.h)
        self.n_embd = lib().bamd_model_n_embd(self.h)
        self.n_layer = lib().bamd_model_n_layer(self.h)
        self.weight_bytes = lib().bamd_model_weight_bytes(self.h)

    def tensor_raw(self, name):
        """the GGUF bytes of a tensor as the loader sees them (bamd_model_tensor_raw): uint8 array"""
        n = lib().bamd_model_tensor_raw(self.h, name.encode(), None, 0)
        if n < 0:
            raise BamdError(lib().bamd_last_error().decode())
        out = np.zeros(n, np.uint8)
        if lib().bamd_model_tensor_raw(self.h, name.encode(), _p(out), n) != n:
            raise BamdError("bamd_model_tensor_raw: size changed")
        return out

    def prefill_aux_bytes(self):
        """bytes of the prompt mat-muls' side tables this model built at load; 0: none, its prompts run on the integer-dot kernel"""
        return int(lib().bamd_model_prefill_aux_bytes(self.h))

    def close(self):
        if self.h:
            lib().bamd_model_free(self.h)
            self.h = None


class Context:
    """llama_context analogue (KV cache + scratch + device-side step state)."""

    def __init__(self, model, n_ctx):
        self.model = model
        self.h = lib().bamd_context_new(model.h, n_ctx)
        if not self.h:
            raise BamdError(lib().bamd_last_error().decode())
        self.n_ctx = n_ctx

    def close(self):
        if self.h:
            lib().bamd_context_free(self.h)
            self.h = None

    def decode(self, tokens, n_past):
        """llama_decode(llama_batch_get_one(tokens, n, n_past, 0)); returns the last token's logits."""
        t = np.ascontiguousarray(tokens, np.int32)
        if lib().bamd_decode(self.h, _p(t), t.size, n_past) != 0:
            raise BamdError(lib().bamd_last_error().decode())
        return np.ctypeslib.as_array(lib().bamd_get_logits(self.h), shape=(self.model.n_vocab,)).copy()

    def generate_greedy(self, n_past, n_steps):
        out = np.zeros(n_steps + 1, np.int32)
        ms = C.c_float(0)
        _chk(lib().bamd_generate_greedy(self.h, n_past, n_steps, _p(out), C.byref(ms)))
        return out, float(ms.value)

    def aql_runs(self):
        """generate_greedy calls of this context that ran on the own AQL queue so far"""
        return int(lib().bamd_aql_runs(self.h))

    def last_logits(self):
        ptr = lib().bamd_get_logits(self.h)
        if not ptr:
            raise BamdError("bamd_get_logits failed: " + lib().bamd_last_error().decode())
        return np.ctypeslib.as_array(ptr, shape=(self.model.n_vocab,)).copy()

    def set_logits_readback(self, on):
        """False: decode leaves the logits on the device and last_logits copies them on demand (bamd_set_logits_readback)"""
        lib().bamd_set_logits_readback(self.h, int(bool(on)))

    def set_logits(self, logits):
        """test hook: overwrite the device logits (n_vocab floats, bamd_set_logits_test)"""
        lg = np.ascontiguousarray(logits, np.float32)
        if lg.shape != (self.model.n_vocab,):
            raise BamdError("set_logits: needs n_vocab floats")
        _chk(lib().bamd_set_logits_test(self.h, _p(lg)))

    def sampler_tables(self, halve_class, cutoff_of):
        """the per-vocabulary tables of the sampler prefilter (bamd_sampler_tables): halve_class [n_vocab] uint8, cutoff_of [n_vocab] f32"""
        cls = np.ascontiguousarray(halve_class, np.uint8); cut = np.ascontiguousarray(cutoff_of, np.float32)
        if cls.shape != cut.shape or cls.ndim != 1:
            raise BamdError("sampler_tables: needs two vectors of one length")
        _chk(lib().bamd_sampler_tables(self.h, _p(cls), _p(cut), cls.size))

    def logits_shortlist(self, pen, halve):
        """the sampler prefilter on the context's stream (bamd_logits_shortlist): pen = penalty entries (PENALTY_DTYPE array, or tuples (id, count, kind, f, d,
        pre)), applied to the device logits in place.  Returns (head, ids, vals): head = dict of count, ntop, nan, top_id, top_logit, cutoff (the floats as
        np.float32); ids / vals have SHORTLIST_CAP entries, the first min(count, SHORTLIST_CAP) written by the library, in no particular order, the others left
        at SHORTLIST_SENTINEL_ID / SHORTLIST_SENTINEL_BITS."""
        p = np.ascontiguousarray(pen, PENALTY_DTYPE).reshape(-1)
        head = ShortlistHead()
        ids = np.full(SHORTLIST_CAP, SHORTLIST_SENTINEL_ID, np.int32)
        vals = np.full(SHORTLIST_CAP, SHORTLIST_SENTINEL_BITS, np.uint32).view(np.float32)
        _chk(lib().bamd_logits_shortlist(self.h, _p(p) if p.size else None, p.size, int(bool(halve)), C.byref(head), _p(ids), _p(vals),
                                         lib().bamd_context_stream(self.h)))
        return (dict(count=int(head.count), ntop=int(head.ntop), nan=int(head.nan), top_id=int(head.top_id), top_logit=np.float32(head.top_logit),
                     cutoff=np.float32(head.cutoff)), ids, vals)

    def kv_seq_rm(self, p0, p1):
        """llama_kv_cache_seq_rm(ctx, 0, p0, p1)"""
        _chk(lib().bamd_kv_seq_rm(self.h, int(p0), int(p1)))

    def kv_seq_add(self, p0, p1, delta):
        """llama_kv_cache_seq_add(ctx, 0, p0, p1, delta)"""
        _chk(lib().bamd_kv_seq_add(self.h, int(p0), int(p1), int(delta)))

    def kv_seq_div(self, p0, p1, d):
        """llama_kv_cache_seq_div(ctx, 0, p0, p1, d)"""
        _chk(lib().bamd_kv_seq_div(self.h, int(p0), int(p1), int(d)))

    def context_shift(self, n_keep, n_past):
        """Booster's context shift (cpp/bridge.cpp:487-503); returns the new n_past"""
        n_discard = (n_past - n_keep) // 2
        self.kv_seq_rm(n_keep, n_keep + n_discard)
        self.kv_seq_add(n_keep + n_discard, n_past, -n_discard)
        return n_past - n_discard

    def profile_step_kinds(self, pos):
        """per launch kind: [qkv, attention, other, wo, gate/up, ffn_down, lm_head, empty event pair] -> (launches, ms, bytes)"""
        launches = np.zeros(8, np.int32); ms = np.zeros(8, np.float64); nbytes = np.zeros(8, np.float64)
        _chk(lib().bamd_profile_step_kinds(self.h, pos, _p(launches), _p(ms), _p(nbytes)))
        return launches, ms, nbytes

    def profile_step(self, pos):
        launches = np.zeros(4, np.int32); ms = np.zeros(4, np.float64); nbytes = np.zeros(4, np.float64)
        _chk(lib().bamd_profile_step(self.h, pos, _p(launches), _p(ms), _p(nbytes)))
        return launches, ms, nbytes

    def timeline_step(self, pos, replays=3):
        """phase stamps of one decode step (BAMD_LIB=.../libbooster_amd_timing.so): u64 [launches][512 workgroups][24], 100 MHz;
        per workgroup: 8 phases of wave 0, 8 phases of wave 7, the exit stamp of each of the 8 waves"""
        cap = 6 * self.model.n_layer + 1        # (five launches per layer, six where the QKV needs two activation forms: the IQ4_NL recipe)
        out = np.zeros((cap, 512, 24), np.uint64)
        n = C.c_int(0)
        _chk(lib().bamd_timeline_step(self.h, pos, replays, _p(out), cap, C.byref(n)))
        return out[:n.value]

    def stage_step(self, token, pos, hidden_in_ptr, hidden_out_ptr, want_logits, prefill_mode, stream_ptr, token_dev_ptr=None):
        _chk(lib().bamd_stage_step(self.h, int(token), token_dev_ptr, int(pos), hidden_in_ptr, hidden_out_ptr, int(want_logits),
                                   int(prefill_mode), stream_ptr))

    def stage_prefill(self, tokens, n_tokens, n_past, hidden_in_ptr, hidden_out_ptr, want_logits, stream_ptr):
        """batched prompt micro-batch through this stage (tokens: host ids on the first stage, else None);
        returns False when the shape has no batched kernels (fall back to stage_step per token)"""
        t = None if tokens is None else np.ascontiguousarray(tokens, np.int32)
        rc = lib().bamd_stage_prefill(self.h, _p(t), int(n_tokens), int(n_past), hidden_in_ptr, hidden_out_ptr, 1 if want_logits else 0, stream_ptr)
        if rc == 2:
            return False
        _chk(rc)
        return True

    def stage_token_to(self, token_dev_ptr, stream_ptr):
        _chk(lib().bamd_stage_token_to(self.h, token_dev_ptr, stream_ptr))

    def stage_logits(self, stream_ptr):
        """host logits of the last stage_step(want_logits=True) on the last stage (synchronises the stream)"""
        lib().bamd_stage_get_logits.restype = C.POINTER(C.c_float); lib().bamd_stage_get_logits.argtypes = [C.c_void_p, C.c_void_p]
        ptr = lib().bamd_stage_get_logits(self.h, stream_ptr)
        if not ptr:
            raise BamdError("bamd_stage_get_logits failed")
        return np.ctypeslib.as_array(ptr, shape=(self.model.n_vocab,)).copy()

    def stage_argmax(self, stream_ptr):
        t = C.c_int32(0)
        _chk(lib().bamd_stage_argmax(self.h, stream_ptr, C.byref(t)))
        return int(t.value)


def bench_matvec(ttype, nrows, k, pro=0, epi=0, mode=0, iters=200):
    us = C.c_float(0)
    _chk(lib().bamd_bench_matvec(ttype, nrows, k, pro, epi, mode, iters, C.byref(us)))
    return float(us.value)


# ---- op-level wrappers (parity tests) ------------------------------------------------------------------------
def op_quantize_q8_K(x, norm_w=None, eps=0.0):
    x = np.ascontiguousarray(x, np.float32)
    w = None if norm_w is None else np.ascontiguousarray(norm_w, np.float32)
    out = np.zeros(x.size // 256 * 292, np.uint8)
    _chk(lib().bamd_op_quantize_q8_K(_p(x), x.size, _p(w), eps, _p(out)))
    return out


def op_quantize_q8_0(x, norm_w=None, eps=0.0):
    """the mat-vec prologue of the Q8_0 / Q4_0 / Q5_0 kernels as standard block_q8_0 bytes {f16 d, i8 qs[32]}"""
    x = np.ascontiguousarray(x, np.float32)
    w = None if norm_w is None else np.ascontiguousarray(norm_w, np.float32)
    out = np.zeros(x.size // 32 * 34, np.uint8)
    _chk(lib().bamd_op_quantize_q8_0(_p(x), x.size, _p(w), eps, _p(out)))
    return out


def op_quantize_q8_1(x, norm_w=None, eps=0.0):
    """the mat-vec prologue of the Q4_1 / Q5_1 kernels as standard block_q8_1 bytes {f16 d, f16 s, i8 qs[32]}"""
    x = np.ascontiguousarray(x, np.float32)
    w = None if norm_w is None else np.ascontiguousarray(norm_w, np.float32)
    out = np.zeros(x.size // 32 * 36, np.uint8)
    _chk(lib().bamd_op_quantize_q8_1(_p(x), x.size, _p(w), eps, _p(out)))
    return out


def op_act_bf16(x, norm_w=None, eps=0.0):
    """the mat-vec prologue of the BF16 kernels: the (normed) vector as bf16 bits (uint16), ggml_fp32_to_bf16_row.  F32 / F16 weights take the f32 vector as it
    is; the mat-vec / mat-mul ops accept the types 0 (F32), 1 (F16) and 30 (BF16) with w_raw = the row-major bytes of the matrix"""
    x = np.ascontiguousarray(x, np.float32)
    w = None if norm_w is None else np.ascontiguousarray(norm_w, np.float32)
    out = np.zeros(x.size, np.uint16)
    _chk(lib().bamd_op_act_bf16(_p(x), x.size, _p(w), eps, _p(out)))
    return out


def op_mul_mat_vec(ttype, w_raw, nrows, k, x, norm_w=None, eps=0.0, residual=None, mode=0):
    w_raw = np.ascontiguousarray(w_raw, np.uint8)
    x = np.ascontiguousarray(x, np.float32)
    nw = None if norm_w is None else np.ascontiguousarray(norm_w, np.float32)
    res = None if residual is None else np.ascontiguousarray(residual, np.float32)
    y = np.zeros(nrows, np.float32)
    _chk(lib().bamd_op_mul_mat_vec(ttype, _p(w_raw), nrows, k, _p(x), _p(nw), eps, _p(res), _p(y), mode))
    return y


def op_mul_mat_vec_argmax(ttype, w_raw, nrows, k, x, norm_w=None, eps=0.0, mode=0):
    """the lm_head launch with the greedy arg-max epilogue: (y, the row the epilogue picks); mode 16 forces the generic kernel"""
    w_raw = np.ascontiguousarray(w_raw, np.uint8)
    x = np.ascontiguousarray(x, np.float32)
    nw = None if norm_w is None else np.ascontiguousarray(norm_w, np.float32)
    y = np.zeros(nrows, np.float32)
    row = C.c_int32(-1)
    _chk(lib().bamd_op_mul_mat_vec_argmax(ttype, _p(w_raw), nrows, k, _p(x), _p(nw), eps, _p(y), mode, C.byref(row)))
    return y, int(row.value)


def op_mul_mat_batch(ttype, w_raw, nrows, k, x, norm_w=None, eps=0.0, residual=None, impl=0):
    """Y[t] = W . Q8_K(x[t]) for T rows at once through the prefill kernels: impl 0 = integer-dot kernel, 1 = round-2 MFMA kernel, 2 = round-5 MFMA kernel (3: its eight-wave Q4_K / Q5_K layout)."""
    w_raw = np.ascontiguousarray(w_raw, np.uint8); x = np.ascontiguousarray(x, np.float32)
    T = x.shape[0]
    nw = None if norm_w is None else np.ascontiguousarray(norm_w, np.float32)
    res = None if residual is None else np.ascontiguousarray(residual, np.float32)
    y = np.zeros((T, nrows), np.float32)
    _chk(lib().bamd_op_mul_mat_batch(ttype, _p(w_raw), nrows, k, _p(x), T, _p(nw), eps, _p(res), _p(y), impl))
    return y


def op_ffn_gate_up(ttype, wg_raw, wu_raw, nrows, k, x, norm_w=None, eps=0.0):
    wg_raw = np.ascontiguousarray(wg_raw, np.uint8); wu_raw = np.ascontiguousarray(wu_raw, np.uint8)
    x = np.ascontiguousarray(x, np.float32)
    nw = None if norm_w is None else np.ascontiguousarray(norm_w, np.float32)
    y = np.zeros(nrows, np.float32)
    _chk(lib().bamd_op_ffn_gate_up(ttype, _p(wg_raw), _p(wu_raw), nrows, k, _p(x), _p(nw), eps, _p(y)))
    return y


def op_get_row(ttype, w_raw, nrows, k, row):
    w_raw = np.ascontiguousarray(w_raw, np.uint8)
    y = np.zeros(k, np.float32)
    _chk(lib().bamd_op_get_row(ttype, _p(w_raw), nrows, k, row, _p(y)))
    return y


def op_rope_row(pos, n_dims, freq_base, freq_scale=1.0, freq_factors=None):
    row = np.zeros(n_dims, np.float32)
    ff = None if freq_factors is None else np.ascontiguousarray(freq_factors, np.float32)
    _chk(lib().bamd_op_rope_row(pos, n_dims, freq_base, freq_scale, _p(ff), _p(row)))
    return row


def op_attention(q, k, v, k_cache, v_cache_t, rope_row, H, Hkv, hd, n_ctx, pos, prefill_mode=False, want_probs=False, long_path=False):
    q = np.ascontiguousarray(q, np.float32); k = np.ascontiguousarray(k, np.float32); v = np.ascontiguousarray(v, np.float32)
    rope_row = np.ascontiguousarray(rope_row, np.float32)
    assert k_cache.dtype == np.uint16 and v_cache_t.dtype == np.uint16 and k_cache.flags.c_contiguous and v_cache_t.flags.c_contiguous
    out = np.zeros(H * hd, np.float32)
    probs = np.zeros(n_ctx, np.float32) if want_probs else None
    _chk(lib().bamd_op_attention(_p(q), _p(k), _p(v), _p(k_cache), _p(v_cache_t), _p(rope_row), H, Hkv, hd, n_ctx, pos, int(prefill_mode) | (2 if (long_path or want_probs) else 0),
                                 _p(out), _p(probs)))
    return (out, probs) if want_probs else out


def op_k_shift(k_cache, n_ctx, Hkv, hd, delta, freq_base, freq_scale=1.0, freq_factors=None, ext_factor=0.0, attn_factor=1.0, n_ctx_orig=8192):
    """the K-shift of one layer through the engine's table code and kernel: a COPY of k_cache [n_ctx*Hkv*hd] (uint16, reference layout) with every
    cell re-rotated by delta[cell]"""
    kc = np.array(k_cache, np.uint16).reshape(-1)
    assert kc.size == n_ctx * Hkv * hd
    d = np.ascontiguousarray(delta, np.int32).reshape(n_ctx)
    ff = None if freq_factors is None else np.ascontiguousarray(freq_factors, np.float32)
    _chk(lib().bamd_op_k_shift(_p(kc), n_ctx, Hkv, hd, _p(d), freq_base, freq_scale, _p(ff), ext_factor, attn_factor, n_ctx_orig))
    return kc


def op_attention_cells(q, k, v, k_cache, v_cache_t, rope_row, cellpos, H, Hkv, hd, n_ctx, pos, cell, n_kv, tiles=0):
    """single-token attention after position edits (shifted-cell score kernel): the token goes to `cell`, cells masked by the position each holds
    (cellpos [n_ctx], -1 = free), over n_kv cells.  The caches (uint16, reference layouts) are updated in place; returns (out [H*hd], head 0's
    probabilities [n_kv])"""
    q = np.ascontiguousarray(q, np.float32); k = np.ascontiguousarray(k, np.float32); v = np.ascontiguousarray(v, np.float32)
    rope_row = np.ascontiguousarray(rope_row, np.float32)
    cp = np.ascontiguousarray(cellpos, np.int32).reshape(n_ctx)
    assert k_cache.dtype == np.uint16 and v_cache_t.dtype == np.uint16 and k_cache.flags.c_contiguous and v_cache_t.flags.c_contiguous
    assert k_cache.size == n_ctx * Hkv * hd and v_cache_t.size == n_ctx * Hkv * hd
    out = np.zeros(H * hd, np.float32); probs = np.zeros(n_kv, np.float32)
    _chk(lib().bamd_op_attention_cells(_p(q), _p(k), _p(v), _p(k_cache), _p(v_cache_t), _p(rope_row), _p(cp), cell, n_kv, H, Hkv, hd, n_ctx, pos, tiles,
                                       _p(out), _p(probs)))
    return out, probs


def op_attention_batch(q, k, v, k_cache, v_cache_t, rope, H, Hkv, hd, n_ctx, pos0, impl=0, ld=0):
    """batched-prefill attention of T = len(q) tokens at positions pos0 ..: q [T][H*hd], k / v [T][Hkv*hd] before RoPE, rope [n_ctx][hd];
    the caches (uint16, reference layouts) are updated in place; returns out [T][H*hd].  impl 0 = launcher's choice, 1 = VALU, 2 = matrix cores"""
    q = np.ascontiguousarray(q, np.float32).reshape(-1, H * hd)
    T = q.shape[0]
    k = np.ascontiguousarray(k, np.float32).reshape(T, Hkv * hd); v = np.ascontiguousarray(v, np.float32).reshape(T, Hkv * hd)
    rope = np.ascontiguousarray(rope, np.float32).reshape(n_ctx, hd)
    assert k_cache.dtype == np.uint16 and v_cache_t.dtype == np.uint16 and k_cache.flags.c_contiguous and v_cache_t.flags.c_contiguous
    assert k_cache.size == n_ctx * Hkv * hd and v_cache_t.size == n_ctx * Hkv * hd
    out = np.zeros((T, H * hd), np.float32)
    _chk(lib().bamd_op_attention_batch(_p(q), _p(k), _p(v), _p(k_cache), _p(v_cache_t), _p(rope), H, Hkv, hd, n_ctx, pos0, T, impl, ld, _p(out)))
    return out


def op_attention_batch_ex(q, k, v, k_cache, v_cache_t, rope, H, Hkv, hd, n_ctx, pos0, impl=0, ld=0, scratch_bytes=0):
    """op_attention_batch with the scratch budget of the slice plan (0 = the default); returns (out [T][H*hd], attention launches issued)"""
    q = np.ascontiguousarray(q, np.float32).reshape(-1, H * hd)
    T = q.shape[0]
    k = np.ascontiguousarray(k, np.float32).reshape(T, Hkv * hd); v = np.ascontiguousarray(v, np.float32).reshape(T, Hkv * hd)
    rope = np.ascontiguousarray(rope, np.float32).reshape(n_ctx, hd)
    assert k_cache.dtype == np.uint16 and v_cache_t.dtype == np.uint16 and k_cache.flags.c_contiguous and v_cache_t.flags.c_contiguous
    assert k_cache.size == n_ctx * Hkv * hd and v_cache_t.size == n_ctx * Hkv * hd
    out = np.zeros((T, H * hd), np.float32); ns = C.c_int(0)
    _chk(lib().bamd_op_attention_batch_ex(_p(q), _p(k), _p(v), _p(k_cache), _p(v_cache_t), _p(rope), H, Hkv, hd, n_ctx, pos0, T, impl, ld, scratch_bytes, _p(out),
                                          C.byref(ns)))
    return out, ns.value


def _segments(segs):
    """[(type, raw blocks, rows), ...] -> what the segment ops take: (n, types, pointer array, rows, the arrays kept alive)"""
    keep = [np.ascontiguousarray(w, np.uint8) for _, w, _ in segs]
    types = np.array([t for t, _, _ in segs], np.int32); rows = np.array([r for _, _, r in segs], np.int32)
    ptrs = (C.c_void_p * len(segs))(*[w.ctypes.data for w in keep])
    return len(segs), types, ptrs, rows, keep


def op_fused_qkv(segs, k, x, norm_w, eps=1e-5, mode=0):
    """the fused QKV launch of a decode step over up to three differently typed segments [(type, raw blocks, rows), ...]: the segments' outputs, concatenated"""
    n, types, ptrs, rows, keep = _segments(segs)
    x = np.ascontiguousarray(x, np.float32); nw = np.ascontiguousarray(norm_w, np.float32)
    y = np.zeros(int(rows.sum()), np.float32)
    _chk(lib().bamd_op_fused_qkv(n, _p(types), ptrs, _p(rows), k, _p(x), _p(nw), eps, mode, _p(y)))
    return y


def op_mul_mat_batch_seg(segs, k, x, ldo, epi=0, residual=None, norm_w=None, eps=0.0, impl=0, fill=0.0):
    """one batched prompt mat-mul as the engine issues it: x [T][k] against the segments [(type, raw blocks, rows), ...] into [T][ldo] (columns the call does
    not write keep `fill`).  epi 0 store, 1 add (one segment, residual [T][ldo]), 2 silu(segment 0) * segment 1; impl 0 integer-dot, 2 matrix cores where
    the type has them"""
    n, types, ptrs, rows, keep = _segments(segs)
    x = np.ascontiguousarray(x, np.float32)
    T = x.shape[0]
    nw = None if norm_w is None else np.ascontiguousarray(norm_w, np.float32)
    res = None if residual is None else np.ascontiguousarray(residual, np.float32).reshape(T, ldo)
    y = np.full((T, ldo), fill, np.float32)
    _chk(lib().bamd_op_mul_mat_batch_seg(n, _p(types), ptrs, _p(rows), k, _p(x), T, _p(nw), eps, ldo, _p(res), epi, impl, _p(y)))
    return y


def op_attention_wo(q, k, v, k_cache, v_cache_t, rope_row, H, Hkv, hd, n_ctx, pos, wo_type, wo_raw, wo_rows, residual, lds_ld=0, serial=1, step=1, il=0,
                    gran_init=None, with_cellpos=False):
    """attention and the wo projection of one decode layer in one launch.  The caches (uint16, reference layouts) are updated in place.  Returns a dict:
    declined (the launcher has no co-launch for the shape: nothing else is valid), n_cu, x2 [wo_rows], gran [H*hd] uint64 {value bits | tag << 32} as the
    launch left them, gave_up (the give-up counter)"""
    q = np.ascontiguousarray(q, np.float32); k = np.ascontiguousarray(k, np.float32); v = np.ascontiguousarray(v, np.float32)
    rope_row = np.ascontiguousarray(rope_row, np.float32)
    assert k_cache.dtype == np.uint16 and v_cache_t.dtype == np.uint16 and k_cache.flags.c_contiguous and v_cache_t.flags.c_contiguous
    assert k_cache.size == n_ctx * Hkv * hd and v_cache_t.size == n_ctx * Hkv * hd and q.size == H * hd
    wo_raw = np.ascontiguousarray(wo_raw, np.uint8); res = np.ascontiguousarray(residual, np.float32)
    assert res.size == wo_rows
    g0 = None if gran_init is None else np.ascontiguousarray(gran_init, np.uint64)
    assert g0 is None or g0.size == H * hd
    x2 = np.zeros(wo_rows, np.float32); gran = np.zeros(H * hd, np.uint64)
    gave_up = C.c_uint32(0); declined = C.c_int32(0); n_cu = C.c_int32(0)
    _chk(lib().bamd_op_attention_wo(_p(q), _p(k), _p(v), _p(k_cache), _p(v_cache_t), _p(rope_row), H, Hkv, hd, n_ctx, pos, lds_ld, wo_type, _p(wo_raw), wo_rows,
                                    _p(res), serial, step, il, int(bool(with_cellpos)), _p(g0), _p(x2), _p(gran), C.byref(gave_up), C.byref(declined), C.byref(n_cu)))
    return dict(declined=bool(declined.value), n_cu=int(n_cu.value), x2=x2, gran=gran, gave_up=int(gave_up.value))


class _LaunchTrace(C.Structure):
    _fields_ = [("kernel", C.c_char * 1024), ("grid", C.c_uint32 * 3), ("block", C.c_uint32 * 3), ("lds_bytes", C.c_uint32), ("kernarg_bytes", C.c_uint32),
                ("kernarg_hash", C.c_uint64)]


def _trace(rc, t):
    if rc == 1:
        return None
    _chk(rc)
    return dict(kernel=t.kernel.decode(), grid=list(t.grid), block=list(t.block), lds=int(t.lds_bytes), kernarg_bytes=int(t.kernarg_bytes),
                kernarg_hash=int(t.kernarg_hash))


def trace_matvec(segs, k, pro, epi, mode=0, n_cu=256):
    """what bamd_launch_matvec would launch for the segments [(type, rows), ...] (host only, no device needed): a dict {kernel (mangled name), grid, block, lds,
    kernarg_bytes, kernarg_hash}, or None when a segment's type has no kernel"""
    types = np.array([t for t, _ in segs], np.int32); rows = np.array([r for _, r in segs], np.int32)
    t = _LaunchTrace()
    return _trace(lib().bamd_trace_matvec(len(segs), _p(types), _p(rows), k, pro, epi, mode, n_cu, C.byref(t)), t)


def trace_mv(segs, k, pro, epi, mode=0, n_cu=256):
    """as trace_matvec, through the dispatch the engine uses (bamd_launch_mv): every family of weight types, not the K-quants alone"""
    types = np.array([t for t, _ in segs], np.int32); rows = np.array([r for _, r in segs], np.int32)
    t = _LaunchTrace()
    return _trace(lib().bamd_trace_mv(len(segs), _p(types), _p(rows), k, pro, epi, mode, n_cu, C.byref(t)), t)


def trace_attn_wo(H, Hkv, hd, n_ctx, lds_ld, wo_type, wo_rows, k, n_cu=256, il=0, with_cellpos=False):
    """what bamd_launch_attn_wo would launch (as trace_matvec), or None when it declines the shape"""
    t = _LaunchTrace()
    return _trace(lib().bamd_trace_attn_wo(H, Hkv, hd, n_ctx, lds_ld, int(bool(with_cellpos)), wo_type, wo_rows, k, n_cu, il, C.byref(t)), t)
