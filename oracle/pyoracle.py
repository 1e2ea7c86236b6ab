"""ctypes glue for the CPU oracle (oracle/liboracle.so).  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module.
"""
import ctypes as C
import os
import subprocess
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

F32, F16, Q4_K, Q5_K, Q6_K, Q8_K = 0, 1, 12, 13, 14, 15
BLOCK_BYTES = {Q4_K: 144, Q5_K: 176, Q6_K: 210, Q8_K: 292}


class BoLayer(C.Structure):
    _fields_ = [("attn_norm", C.c_void_p), ("wq", C.c_void_p), ("wk", C.c_void_p), ("wv", C.c_void_p), ("wo", C.c_void_p),
                ("tq", C.c_int), ("tk", C.c_int), ("tv", C.c_int), ("to", C.c_int),
                ("ffn_norm", C.c_void_p), ("wg", C.c_void_p), ("wu", C.c_void_p), ("wd", C.c_void_p),
                ("tg", C.c_int), ("tu", C.c_int), ("td", C.c_int)]


class BoModel(C.Structure):
    _fields_ = [("E", C.c_int), ("H", C.c_int), ("Hkv", C.c_int), ("hd", C.c_int), ("L", C.c_int), ("F", C.c_int), ("V", C.c_int),
                ("eps", C.c_float), ("rope_theta", C.c_float), ("rope_freq_scale", C.c_float),
                ("n_ctx_orig", C.c_int),
                ("rope_freqs", C.c_void_p),
                ("tok_embd", C.c_void_p), ("t_embd", C.c_int),
                ("out_norm", C.c_void_p),
                ("output", C.c_void_p), ("t_out", C.c_int),
                ("layers", C.POINTER(BoLayer))]


TAP_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_float), C.c_int64)


def build():
    subprocess.check_call(["make", "-s", "-C", _HERE, "oracle"])


def lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(_HERE, "liboracle.so")
        src = os.path.join(_HERE, "booster_oracle.c")
        if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(src):
            build()
        L = C.CDLL(path)
        L.bo_fp16_to_fp32.restype = C.c_float; L.bo_fp16_to_fp32.argtypes = [C.c_uint16]
        L.bo_fp32_to_fp16.restype = C.c_uint16; L.bo_fp32_to_fp16.argtypes = [C.c_float]
        L.bo_row_size.restype = C.c_size_t; L.bo_row_size.argtypes = [C.c_int, C.c_int64]
        L.bo_quantize_row_q8_K.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.bo_dequantize_row.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int64]
        for n in ("bo_vec_dot_q4_K_q8_K", "bo_vec_dot_q5_K_q8_K", "bo_vec_dot_q6_K_q8_K"):
            getattr(L, n).restype = C.c_float; getattr(L, n).argtypes = [C.c_int, C.c_void_p, C.c_void_p]
        L.bo_mul_mat_q.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int]
        L.bo_rms_norm.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_float]
        L.bo_v_expf.restype = C.c_float; L.bo_v_expf.argtypes = [C.c_float]
        L.bo_v_silu.restype = C.c_float; L.bo_v_silu.argtypes = [C.c_float]
        L.bo_vec_silu.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.bo_soft_max.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int]
        L.bo_rope_cache.argtypes = [C.c_void_p, C.c_int32, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_float, C.c_float,
                                    C.c_int, C.c_float, C.c_float]
        L.bo_rope_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.bo_dot_f16_f32_tinyblas.restype = C.c_float; L.bo_dot_f16_f32_tinyblas.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.bo_vec_dot_f16.restype = C.c_float; L.bo_vec_dot_f16.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
        L.bo_attention.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
        L.bo_attention_cells.restype = C.c_int
        L.bo_attention_cells.argtypes = [C.c_void_p] * 7 + [C.c_int] * 7 +[C.c_void_p, C.c_void_p, C.c_int]
        L.bo_k_shift.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_float, C.c_float,
                                 C.c_int, C.c_float, C.c_float]
        L.bo_ctx_new.restype = C.c_void_p; L.bo_ctx_new.argtypes = [C.POINTER(BoModel), C.c_int, C.c_int]
        L.bo_ctx_free.argtypes = [C.c_void_p]
        L.bo_ctx_set_tap.argtypes = [C.c_void_p, TAP_FN, C.c_void_p]
        L.bo_kv_clear.argtypes = [C.c_void_p]
        L.bo_kv_seq_rm.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.bo_kv_seq_add.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.bo_kv_seq_div.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.bo_decode.restype = C.c_int; L.bo_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.bo_get_logits.restype = C.POINTER(C.c_float); L.bo_get_logits.argtypes = [C.c_void_p]
        L.bo_kv_k.restype = C.POINTER(C.c_uint16); L.bo_kv_k.argtypes = [C.c_void_p, C.c_int]
        L.bo_kv_v.restype = C.POINTER(C.c_uint16); L.bo_kv_v.argtypes = [C.c_void_p, C.c_int]
        _LIB = L
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- array-level helpers -----------------------------------------------------------------------------------
def quantize_q8_K(x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros(x.size // 256 * 292, np.uint8)
    lib().bo_quantize_row_q8_K(_p(x), _p(out), x.size)
    return out


def dequantize(ttype, raw, k):
    raw = np.ascontiguousarray(raw, np.uint8)
    y = np.zeros(k, np.float32)
    lib().bo_dequantize_row(ttype, _p(raw), _p(y), k)
    return y


def mul_mat_q(ttype, W, nrows, K, x, nthreads=1):
    W = np.ascontiguousarray(W, np.uint8)
    x = np.ascontiguousarray(x, np.float32).reshape(-1, K)
    T = x.shape[0]
    y = np.zeros((T, nrows), np.float32)
    lib().bo_mul_mat_q(ttype, _p(W), nrows, K, _p(x), T, _p(y), nthreads)
    return y


def rms_norm(x, eps):
    x = np.ascontiguousarray(x, np.float32)
    y = np.empty_like(x)
    lib().bo_rms_norm(_p(x), _p(y), x.size, eps)
    return y


def silu(x):
    """ggml_v_silu (one AVX2 lane) of every element: what ggml_silu computes for rows whose length is a multiple of 8 (the reference
    takes the last n % 8 elements of a row through scalar ggml_silu_f32, i.e. libm expf; the decode path's rows are n_ff long)"""
    x = np.ascontiguousarray(x, np.float32)
    y = np.empty_like(x)
    lib().bo_vec_silu(_p(x), _p(y), x.size)
    return y


def soft_max(s, mask, scale):
    s = np.ascontiguousarray(s, np.float32)
    p = np.empty_like(s)
    m = None if mask is None else np.ascontiguousarray(mask, np.float32)
    lib().bo_soft_max(_p(s), None if m is None else _p(m), scale, _p(p), s.size)
    return p


def rope_cache(pos, n_dims, freq_base, freq_scale=1.0, freq_factors=None, ext_factor=0.0, attn_factor=1.0, n_ctx_orig=8192,
               beta_fast=32.0, beta_slow=1.0):
    c = np.zeros(n_dims, np.float32)
    ff = None if freq_factors is None else np.ascontiguousarray(freq_factors, np.float32)
    lib().bo_rope_cache(_p(c), pos, n_dims, freq_base, freq_scale, None if ff is None else _p(ff), ext_factor, attn_factor,
                        n_ctx_orig, beta_fast, beta_slow)
    return c


def attention(q, k, v, k_cache, v_cache_t, rope, H, Hkv, hd, n_ctx, n_past, f16_scores, nthreads=None):
    """llm_build_kv of one layer for the T = len(q) tokens at positions n_past ..: q [T][H*hd], k / v [T][Hkv*hd] f32 before RoPE, rope = the
    (cos, sin) table [>= n_past + T][hd] or its rows [T][hd] of those positions.  k_cache [n_ctx*Hkv*hd] / v_cache_t [Hkv*hd*n_ctx] (uint16,
    the reference's layouts) are updated in place.  Returns out [T][H*hd]."""
    q = np.array(q, np.float32).reshape(-1, H * hd)                      # copies: bo_attention ropes q / k in place
    T = q.shape[0]
    k = np.array(k, np.float32).reshape(T, Hkv * hd); v = np.ascontiguousarray(v, np.float32).reshape(T, Hkv * hd)
    rope = np.asarray(rope, np.float32).reshape(-1, hd)
    rows = np.ascontiguousarray(rope if rope.shape[0] == T else rope[n_past:n_past + T])
    assert rows.shape[0] == T and n_past + T <= n_ctx
    assert k_cache.dtype == np.uint16 and v_cache_t.dtype == np.uint16 and k_cache.flags.c_contiguous and v_cache_t.flags.c_contiguous
    assert k_cache.size == n_ctx * Hkv * hd and v_cache_t.size == n_ctx * Hkv * hd
    out = np.zeros((T, H * hd), np.float32)
    lib().bo_attention(_p(q), _p(k), _p(v), _p(rows), _p(k_cache), _p(v_cache_t), H, Hkv, hd, n_ctx, n_past, T, int(bool(f16_scores)),
                       _p(out), nthreads or min(16, os.cpu_count() or 1))
    return out


def attention_cells(q, k, v, k_cache, v_cache_t, rope_row, cellpos, H, Hkv, hd, n_ctx, pos, cell, n_kv, nthreads=None):
    """bo_attention_cells: ONE token at position pos stored in `cell`, attention over the first n_kv cells masked by the position each holds
    (cellpos [n_ctx], -1 = free; the token's own entry is set to pos here, as find_slot does).  The caches (uint16, reference layouts) are
    updated in place.  Returns (out [H*hd], query head 0's probabilities [n_kv])."""
    q = np.array(q, np.float32).reshape(H * hd); k = np.array(k, np.float32).reshape(Hkv * hd)
    v = np.ascontiguousarray(v, np.float32).reshape(Hkv * hd); rope_row = np.ascontiguousarray(rope_row, np.float32).reshape(hd)
    cp = np.array(cellpos, np.int32).reshape(n_ctx)
    cp[cell] = pos
    assert k_cache.dtype == np.uint16 and v_cache_t.dtype == np.uint16 and k_cache.flags.c_contiguous and v_cache_t.flags.c_contiguous
    assert k_cache.size == n_ctx * Hkv * hd and v_cache_t.size == n_ctx * Hkv * hd
    out = np.zeros(H * hd, np.float32); probs = np.zeros(n_kv, np.float32)
    rc = lib().bo_attention_cells(_p(q), _p(k), _p(v), _p(rope_row), _p(k_cache), _p(v_cache_t), _p(cp), H, Hkv, hd, n_ctx, pos, cell, n_kv,
                                  _p(out), _p(probs), nthreads or min(16, os.cpu_count() or 1))
    assert rc == 0, "bo_attention_cells: bad cell / n_kv"
    return out, probs


def k_shift(k_cache, n_ctx, Hkv, hd, delta, freq_base, freq_scale=1.0, freq_factors=None, ext_factor=0.0, attn_factor=1.0, n_ctx_orig=8192,
            beta_fast=32.0, beta_slow=1.0):
    """bo_k_shift: a COPY of the f16 K cache [n_ctx*Hkv*hd] (uint16, reference layout) with every cell re-rotated by delta[cell]"""
    kc = np.array(k_cache, np.uint16).reshape(-1)
    assert kc.size == n_ctx * Hkv * hd
    d = np.ascontiguousarray(delta, np.int32).reshape(n_ctx)
    ff = None if freq_factors is None else np.ascontiguousarray(freq_factors, np.float32)
    lib().bo_k_shift(_p(kc), n_ctx, Hkv, hd, _p(d), freq_base, freq_scale, None if ff is None else _p(ff), ext_factor, attn_factor, n_ctx_orig,
                     beta_fast, beta_slow)
    return kc


# ---- whole model -----------------------------------------------------------------------------------------
class OracleModel:
    """Builds a bo_model from a booster_amd.gguf.GGUFReader (tensor bytes stay mapped)."""

    def __init__(self, reader, n_layers=None):
        kv, T = reader.kv, reader.tensors
        self.reader = reader
        self._keep = []
        E = int(kv["llama.embedding_length"]); H = int(kv["llama.attention.head_count"])
        Hkv = int(kv.get("llama.attention.head_count_kv", H)); L = int(kv["llama.block_count"])
        if n_layers is not None:
            L = min(L, n_layers)
        Fd = int(kv["llama.feed_forward_length"])
        V = int(T["token_embd.weight"]["shape"][1])
        self.E, self.H, self.Hkv, self.L, self.F, self.V = E, H, Hkv, L, Fd, V
        self.hd = E // H

        def ptr(name):
            a = np.ascontiguousarray(T[name]["data"])
            self._keep.append(a)
            return a.ctypes.data

        layers = (BoLayer * L)()
        for il in range(L):
            p = "blk.%d." % il
            ly = layers[il]
            ly.attn_norm = ptr(p + "attn_norm.weight"); ly.ffn_norm = ptr(p + "ffn_norm.weight")
            for f, t, nm in (("wq", "tq", "attn_q"), ("wk", "tk", "attn_k"), ("wv", "tv", "attn_v"), ("wo", "to", "attn_output"),
                             ("wg", "tg", "ffn_gate"), ("wu", "tu", "ffn_up"), ("wd", "td", "ffn_down")):
                setattr(ly, f, ptr(p + nm + ".weight")); setattr(ly, t, T[p + nm + ".weight"]["type"])
        m = BoModel()
        m.E, m.H, m.Hkv, m.hd, m.L, m.F, m.V = E, H, Hkv, E // H, L, Fd, V
        m.eps = float(kv["llama.attention.layer_norm_rms_epsilon"])
        m.rope_theta = float(kv.get("llama.rope.freq_base", 10000.0))
        m.rope_freq_scale = 1.0
        m.n_ctx_orig = int(kv.get("llama.context_length", 8192))
        m.rope_freqs = ptr("rope_freqs.weight") if "rope_freqs.weight" in T else None
        m.tok_embd = ptr("token_embd.weight"); m.t_embd = T["token_embd.weight"]["type"]
        m.out_norm = ptr("output_norm.weight")
        oname = "output.weight" if "output.weight" in T else "token_embd.weight"     # tied embeddings, llama.cpp:6070-6076
        m.output = ptr(oname); m.t_out = T[oname]["type"]
        m.layers = layers
        self._layers = layers
        self.m = m


class OracleContext:
    def __init__(self, model, n_ctx, nthreads=1):
        self.model = model
        self.n_ctx = n_ctx
        self.c = lib().bo_ctx_new(C.byref(model.m), n_ctx, nthreads)
        self._tap = None
        self.taps = {}

    def close(self):
        if self.c:
            lib().bo_ctx_free(self.c)
            self.c = None

    def enable_taps(self):
        def fn(ud, name, il, data, n):
            key = name.decode() + ("-%d" % il if il >= 0 else "")
            self.taps[key] = np.ctypeslib.as_array(data, shape=(n,)).copy()
        self._tap = TAP_FN(fn)
        lib().bo_ctx_set_tap(self.c, self._tap, None)

    def decode(self, tokens, n_past):
        t = np.ascontiguousarray(tokens, np.int32)
        self.taps = {}
        rc = lib().bo_decode(self.c, _p(t), t.size, n_past)
        assert rc == 0, "bo_decode failed"
        return np.ctypeslib.as_array(lib().bo_get_logits(self.c), shape=(self.model.V,)).copy()

    def kv_seq_rm(self, p0, p1):
        """llama_kv_cache_seq_rm(ctx, 0, p0, p1)"""
        lib().bo_kv_seq_rm(self.c, int(p0), int(p1))

    def kv_seq_add(self, p0, p1, delta):
        """llama_kv_cache_seq_add(ctx, 0, p0, p1, delta)"""
        lib().bo_kv_seq_add(self.c, int(p0), int(p1), int(delta))

    def kv_seq_div(self, p0, p1, d):
        """llama_kv_cache_seq_div(ctx, 0, p0, p1, d)"""
        assert d >= 1
        lib().bo_kv_seq_div(self.c, int(p0), int(p1), int(d))

    def context_shift(self, n_keep, n_past):
        """Booster's context shift (cpp/bridge.cpp:487-503); returns the new n_past"""
        n_discard = (n_past - n_keep) // 2
        self.kv_seq_rm(n_keep, n_keep + n_discard)
        self.kv_seq_add(n_keep + n_discard, n_past, -n_discard)
        return n_past - n_discard

    def kv_k(self, il):
        n = self.n_ctx * self.model.Hkv * self.model.hd
        return np.ctypeslib.as_array(lib().bo_kv_k(self.c, il), shape=(n,)).copy()

    def kv_v(self, il):
        n = self.n_ctx * self.model.Hkv * self.model.hd
        return np.ctypeslib.as_array(lib().bo_kv_v(self.c, il), shape=(n,)).copy()
