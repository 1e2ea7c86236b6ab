"""F32 / F16 / BF16 (unquantised weights): seeded inputs of the float tests and a numpy restatement of what the kernels compute.

The reference build defines GGML_USE_LLAMAFILE, which decides the chain of each type:

  F32 / F16   ggml_compute_forward_mul_mat (ggml.c:12318-12343) hands the mat-mul to llamafile_sgemm -> tinyBLAS<8, __m256, ...>::gemm (sgemm.cpp:408-432): per
              output ONE 8-lane accumulator, lane j:  acc = fmaf(w[8i + j], x[8i + j], acc), i = 0 .. K/8 - 1, from 0 (_mm256_fmadd_ps: one rounding per step);
              F16 weights are widened exactly, THE ACTIVATIONS STAY f32; then hsum(__m256) (sgemm.cpp:163-183): t[m] = c[m] + c[m + 4], (t0 + t2) + (t1 + t3).
              Not ggml_vec_dot_f16 (32 lanes, f16 activations).  The chain of an output does not depend on the number of tokens.
  BF16        no llamafile_sgemm case: the activations are rounded to bf16 (ggml_compute_fp32_to_bf16, ggml-impl.h:88-101: integer round-to-nearest-even, NaN
              quieted, subnormals kept), then ggml_vec_dot_bf16's AVX2 branch (ggml.c:2007-2026): four 8-lane accumulators, lane j of c_a takes
              k = 32i + 8(a - 1) + j with add(mul(w, x), c); (c1 + c3) + (c2 + c4), then the same 8 -> 1 tree.  A bf16 x bf16 product is exact in f32 unless it
              falls below 2^-126; there mul-then-add and fma differ, and what the compiled reference does is recorded: BF16_FUSED below.

The restatement is held to the genuine reference's outputs stored in tests/golden/float_kats.npz (tests/golden/gen_float_kats.py, tests/test_float_ref.py).
The exact f32 fma is lowbit_ref.fma32 (f64 product, TwoSum, round to odd, cast)."""
import ctypes as C
import hashlib
import os

import numpy as np

from lowbit_ref import fma32

F32, F16, BF16 = 0, 1, 30
TYPES = (F32, F16, BF16)
NAME = {F32: "f32", F16: "f16", BF16: "bf16"}
ESIZE = {F32: 4, F16: 2, BF16: 2}
SGEMM_TYPES = (F32, F16)
KS = [256, 512, 1024, 4096]
SCALES = (1e-3, 1.0, 50.0)
ROWS = 32
EDGE_K = 1024
EDGE_WKINDS = ("random", "f16_subnormal", "zero", "f16_max", "tiny", "unit")
EDGE_AKINDS = ("random", "ties", "subnormal", "tiny", "cancel", "zero")
EDGE_NVEC = 6
DEQ_ROWS = (0, 15, 31)
SGEMM_COLS = lambda n: [(2 * j + 1) % n for j in range(5)]      # which vectors form the five columns of the n = 5 llamafile_sgemm call
REF = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "libggml_ref.so")
# the compiled reference's add(mul(w, x), c) of ggml_vec_dot_bf16 is NOT contracted into an fma: the edge vectors hold products below 2^-126, where the two
# differ, and the stored answers are those of the separate multiply and add (tests/test_float_ref.py holds both statements)
BF16_FUSED = False


# ---- number formats -------------------------------------------------------------------------------------------------------------------------
def bf16_bits(x):
    """ggml_compute_fp32_to_bf16 (ggml-impl.h:88-101): uint16 bits of an f32 array"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7fff + ((u >> 16) & 1)) >> 16
    return np.where((u & 0x7fffffff) > 0x7f800000, (u >> 16) | 64, r).astype(np.uint16)


def bf16_to_f32(b):
    return (np.ascontiguousarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


def encode(t, v):
    """raw bytes of the f32 values v in type t (F16 / BF16: rounded to nearest even)"""
    v = np.ascontiguousarray(v, np.float32)
    with np.errstate(all="ignore"):
        return (v if t == F32 else v.astype(np.float16) if t == F16 else bf16_bits(v)).view(np.uint8).reshape(-1)


def to_f32(t, raw):
    """what to_float of the type gives: the weights as f32, exactly"""
    raw = np.ascontiguousarray(raw, np.uint8)
    if t == F32:
        return raw.view(np.float32).copy()
    if t == F16:
        return raw.view(np.float16).astype(np.float32)
    return bf16_to_f32(raw.view(np.uint16))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def _digest(raw, xs):
    h = hashlib.sha256(np.ascontiguousarray(raw).tobytes())
    for x in xs:
        h.update(np.ascontiguousarray(x, np.float32).tobytes())
    return h.hexdigest()


def rand_case(t, K):
    from booster_amd.gguf import random_float_tensor
    rng = np.random.default_rng(7001 * (t + 1) + K)
    raw = random_float_tensor(t, K, ROWS, rng, amp=4.0)
    xs = [(rng.standard_normal(K) * s).astype(np.float32) for s in SCALES]
    return raw, xs, _digest(raw, xs)


def _cycle(kinds, n, rng):
    tags = np.array([kinds[i % len(kinds)] for i in range(n)], dtype=object)
    rng.shuffle(tags)
    return tags


def _pow2(e):
    return np.float32(2.0) ** np.float32(e)


# whole rows / whole vectors of one regime beside the mixed ones: where EVERY term of a dot product is tiny, the products below 2^-126 and the subnormal partial
# sums are the result itself instead of vanishing under a large term
EDGE_ROW_KINDS = (EDGE_WKINDS,) * 16 + (("tiny",),) * 4 + (("f16_subnormal",),) * 4 + (("unit",),) * 4 + (("tiny", "f16_subnormal", "zero", "unit"),) * 4
EDGE_VEC_KINDS = (EDGE_AKINDS, EDGE_AKINDS, ("tiny",), ("subnormal",), ("cancel",), ("tiny", "subnormal", "cancel", "zero"))


def edge_weights(t, K, rows, rng):
    """one kind per 32 weights, drawn from the row's kinds (EDGE_ROW_KINDS): subnormal f16 values (m * 2^-24), +-0, the largest finite f16, tiny values (2^-65
    and below: with tiny or subnormal activations the products fall below 2^-126), and +1 / -1 alternating along every lane's chain (so that `cancel`
    activations leave a subnormal partial sum)"""
    nb = K // 32
    tags = np.concatenate([_cycle(EDGE_ROW_KINDS[r % len(EDGE_ROW_KINDS)], nb, rng) for r in range(rows)])
    w = np.zeros((rows * nb, 32), np.float32)
    for b, k in enumerate(tags):
        sgn = np.where(rng.random(32) < 0.5, -1.0, 1.0).astype(np.float32)
        if k == "random":
            v = (rng.standard_normal(32) * 0.1).astype(np.float32)
        elif k == "f16_subnormal":
            v = sgn * rng.integers(1, 1024, 32).astype(np.float32) * _pow2(-24)
        elif k == "zero":
            v = sgn * np.float32(0.0)
        elif k == "f16_max":
            v = sgn * np.float32(65504.0)
        elif k == "tiny":
            v = sgn * rng.integers(128, 256, 32).astype(np.float32) * _pow2(int(rng.integers(-82, -72)))
        elif k == "unit":
            v = np.tile(np.repeat(np.array([1.0, -1.0], np.float32), 8), 2)       # chain step i of every lane: +1, -1, +1, -1
        else:
            raise ValueError(k)
        w[b] = v
    return encode(t, w.reshape(rows, K)), tags.reshape(rows, nb)


def edge_activations(K, rng, kind_of):
    """one kind per 32 values: f32 values that tie at the bf16 rounding boundary (low half 0x8000) with even and odd upper halves, f32 subnormals, tiny normal
    values, pairs a, a * (1 + 2^-7) around 2^-120 along every chain (with +1 / -1 weights the partial sum is a subnormal), +-0"""
    x = np.zeros(K, np.float32)
    for b, k in enumerate(kind_of):
        sgn = np.where(rng.random(32) < 0.5, -1.0, 1.0).astype(np.float32)
        if k == "random":
            v = (rng.standard_normal(32) * 10.0 ** rng.uniform(-2, 2)).astype(np.float32)
        elif k == "ties":
            hi = (rng.integers(0x3c00, 0x4200, 32).astype(np.uint32) & ~np.uint32(1)) | (np.arange(32, dtype=np.uint32) & 1)     # both parities
            v = ((hi << 16) | np.uint32(0x8000) | (np.where(rng.random(32) < 0.5, 0x80000000, 0).astype(np.uint32))).view(np.float32)
        elif k == "subnormal":
            v = (rng.integers(1, 0x800000, 32).astype(np.uint32) | np.where(rng.random(32) < 0.5, 0x80000000, 0).astype(np.uint32)).view(np.float32)
        elif k == "tiny":
            v = sgn * rng.integers(128, 256, 32).astype(np.float32) * _pow2(int(rng.integers(-75, -62)))
        elif k == "cancel":
            a = rng.integers(128, 256, 8).astype(np.float32) * _pow2(-127)
            v = np.concatenate([a, a * np.float32(1.0 + 2.0 ** -7), a, a * np.float32(1.0 + 2.0 ** -7)]).astype(np.float32)
        elif k == "zero":
            v = sgn * np.float32(0.0)
        else:
            raise ValueError(k)
        x[32 * b:32 * b + 32] = v
    return x


def edge_case(t):
    rng = np.random.default_rng(170003 + t)
    raw, wtags = edge_weights(t, EDGE_K, ROWS, rng)
    nb = EDGE_K // 32
    xt = np.stack([_cycle(EDGE_VEC_KINDS[i], nb, rng) for i in range(EDGE_NVEC)])
    xs = [edge_activations(EDGE_K, rng, xt[i]) for i in range(EDGE_NVEC)]
    return raw, xs, _digest(raw, xs), wtags, xt


def all_cases(t):
    """(key, raw weight bytes, activation vectors, inputs digest) of every stored case of type t"""
    for K in KS:
        raw, xs, digest = rand_case(t, K)
        yield "%s_K%d" % (NAME[t], K), raw, xs, digest
    raw, xs, digest, _, _ = edge_case(t)
    yield "%s_edge" % NAME[t], raw, xs, digest


# ---- the chains -----------------------------------------------------------------------------------------------------------------------------
def _hsum8(c):
    """hsum(__m256) of [..., 8] (sgemm.cpp:163-183; the tail of ggml_vec_dot_bf16 is the same tree)"""
    with np.errstate(all="ignore"):
        t = c[..., 0:4] + c[..., 4:8]
        u = t[..., 0:2] + t[..., 2:4]
        return (u[..., 0] + u[..., 1]).astype(np.float32)


def sgemm_rows(w, x):
    """tinyBLAS<8>: w f32 [rows][K] (F16 weights already widened), x f32 [K] -> f32 [rows]"""
    rows, K = w.shape
    acc = np.zeros((rows, 8), np.float32)
    x = np.ascontiguousarray(x, np.float32)
    for i in range(K // 8):
        acc = fma32(w[:, 8 * i:8 * i + 8], x[None, 8 * i:8 * i + 8], acc)
    return _hsum8(acc)


def vec_dot_bf16_rows(w, xb, fused=None):
    """ggml_vec_dot_bf16, AVX2 branch: w f32 [rows][K] (bf16 values), xb uint16 [K] -> f32 [rows]"""
    fused = BF16_FUSED if fused is None else fused
    rows, K = w.shape
    x = bf16_to_f32(xb)
    acc = np.zeros((rows, 4, 8), np.float32)
    with np.errstate(all="ignore"):
        for i in range(K // 32):
            wv = w[:, 32 * i:32 * i + 32].reshape(rows, 4, 8); xv = x[32 * i:32 * i + 32].reshape(1, 4, 8)
            acc = fma32(wv, xv, acc) if fused else ((wv * xv).astype(np.float32) + acc).astype(np.float32)
        c = (acc[:, 0] + acc[:, 2]) + (acc[:, 1] + acc[:, 3])
    return _hsum8(c)


def mul_mat(t, raw, rows, K, x, chunk=2048):
    """y = W . x as the reference computes it for weights of type t (x: the f32 activation vector; BF16 rounds it first)"""
    w = to_f32(t, np.asarray(raw, np.uint8)[:rows * K * ESIZE[t]]).reshape(rows, K)
    x = np.ascontiguousarray(x, np.float32)
    if t == BF16:
        xb = bf16_bits(x)
        return np.concatenate([vec_dot_bf16_rows(w[r:r + chunk], xb) for r in range(0, rows, chunk)])
    return np.concatenate([sgemm_rows(w[r:r + chunk], x) for r in range(0, rows, chunk)])


# ---- the genuine reference, where it is built (oracle/_ref/libggml_ref.so: `make -C oracle ref`) ---------------------------------------------------
class _Traits(C.Structure):
    _fields_ = [("type_name", C.c_char_p), ("blck_size", C.c_int64), ("blck_size_interleave", C.c_int64), ("type_size", C.c_size_t), ("is_quantized", C.c_bool),
                ("to_float", C.c_void_p), ("from_float", C.c_void_p), ("from_float_ref", C.c_void_p), ("from_float_to_mat", C.c_void_p), ("vec_dot", C.c_void_p),
                ("vec_dot_type", C.c_int), ("nrows", C.c_int64), ("ncols", C.c_int64), ("gemv", C.c_void_p), ("gemm", C.c_void_p)]


def load_ref():
    """the reference library, or None where it is not built"""
    if not os.path.exists(REF):
        return None
    L = C.CDLL(REF)
    class _InitParams(C.Structure):
        _fields_ = [("mem_size", C.c_size_t), ("mem_buffer", C.c_void_p), ("no_alloc", C.c_bool)]
    L.ggml_init.restype = C.c_void_p                            # ggml_init fills the f16 -> f32 table that GGML_FP16_TO_FP32 reads on x86
    L.ggml_init.argtypes = [_InitParams]
    L.ggml_init(_InitParams(1 << 20, None, False))
    L.ggml_internal_get_type_traits.restype = _Traits
    L.ggml_internal_get_type_traits.argtypes = [C.c_int]
    L.ggml_fp32_to_bf16_row.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.llamafile_sgemm.restype = C.c_bool
    L.llamafile_sgemm.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    return L


def reference_outputs(L, t, raw, xs):
    """the live reference for one case: dict of
      to_float  f32 [ROWS][K]            the type's to_float of every row (F32: the rows themselves)
      F32 / F16:  sgemm1 f32 [vectors][ROWS] (llamafile_sgemm at n = 1), sgemm5 f32 [5][ROWS] (n = 5, columns = vectors SGEMM_COLS)
      BF16:       act u16 [vectors][K] (ggml_fp32_to_bf16_row), dots f32 [vectors][ROWS] (the vec_dot of the type traits over those)"""
    K = xs[0].size
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    raw = np.ascontiguousarray(raw, np.uint8)
    rb = K * ESIZE[t]
    out = {}
    tr = L.ggml_internal_get_type_traits(t)
    if t == F32:
        out["to_float"] = raw.view(np.float32).reshape(ROWS, K).copy()
    else:
        to_float = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int64)(tr.to_float)
        deq = np.zeros((ROWS, K), np.float32)
        for r in range(ROWS):
            to_float(C.c_void_p(raw.ctypes.data + r * rb), p(deq[r]), K)
        out["to_float"] = deq
    if t in SGEMM_TYPES:
        X = np.ascontiguousarray(np.stack(xs), np.float32)
        sg1 = np.zeros((len(xs), ROWS), np.float32); sg5 = np.zeros((5, ROWS), np.float32)
        for i in range(len(xs)):
            assert L.llamafile_sgemm(ROWS, 1, K, p(raw), K, p(X[i]), K, p(sg1[i]), ROWS, 0, 1, t, F32, 0)
        X5 = np.ascontiguousarray(X[SGEMM_COLS(len(xs))])
        assert L.llamafile_sgemm(ROWS, 5, K, p(raw), K, p(X5), K, p(sg5), ROWS, 0, 1, t, F32, 0)
        out["sgemm1"] = sg1; out["sgemm5"] = sg5
    else:
        assert not L.llamafile_sgemm(ROWS, 1, K, p(raw), K, p(np.zeros(K, np.float32)), K, p(np.zeros(ROWS, np.float32)), ROWS, 0, 1, t, F32, 0), "llamafile_sgemm took BF16"
        vec_dot = C.CFUNCTYPE(None, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int)(tr.vec_dot)
        assert tr.vec_dot_type == BF16
        act = np.zeros((len(xs), K), np.uint16); dots = np.zeros((len(xs), ROWS), np.float32)
        for i, x in enumerate(xs):
            L.ggml_fp32_to_bf16_row(p(np.ascontiguousarray(x, np.float32)), p(act[i]), K)
            for r in range(ROWS):
                s = C.c_float(0)
                vec_dot(K, C.byref(s), 0, C.c_void_p(raw.ctypes.data + r * rb), 0, p(act[i]), 0, 1)
                dots[i, r] = s.value
        out["act"] = act; out["dots"] = dots
    return out
