"""Q8_0 / Q4_0 / Q5_0: seeded inputs of the legacy-quant tests and a numpy restatement of what the kernels compute — the reference's AVX2
quantize_row_q8_0 (ggml-quants.c:936-994), tinyBLAS_Q0_AVX::gemm (sgemm.cpp:711-759: Q8_0 and Q4_0 weights), ggml_vec_dot_q5_0_q8_0 (ggml-quants.c:4644-4666;
_q4_0_q8_0 :3900-3923 and _q8_0_q8_0 :5227- have the same shape) and dequantize_row_q4_0 / q5_0 / q8_0 (:1515, :1556, :1609).

The restatement is held to the genuine reference's outputs stored in tests/golden/legacy_kats.npz (tests/golden/gen_legacy_kats.py, tests/test_legacy_ref.py).

One dot product = eight SIMD lanes e, each ONE sequential f32 fma chain over the 32-blocks l = 0 .. K/32 - 1, closed by the hsum tree:
    acc_e = fma(f32(f16 d_w[l]) * f32(f16 d_x[l]), (float) dot4_e[l], acc_e)
with dot4_e the exact integer dot of elements 4e .. 4e+3 of weight block and activation block (|dot4| <= 4 * 128 * 127 < 2^24: int -> f32 is exact).
Activations: per 32 values amax; d = f16(amax / 127.f); id = amax != 0 ? 127.f / amax : 0; q = round-half-even(x * id) (an f32 product).
The fma is lowbit_ref.fma32 (exact, see there)."""
import ctypes as C
import hashlib
import os

import numpy as np

from lowbit_ref import fma32

Q4_0, Q5_0, Q8_0 = 2, 6, 8
TYPES = (Q8_0, Q4_0, Q5_0)
BB = {Q4_0: 18, Q5_0: 22, Q8_0: 34}
QS_OFF = {Q4_0: 2, Q5_0: 6, Q8_0: 2}
NAME = {Q4_0: "q4_0", Q5_0: "q5_0", Q8_0: "q8_0"}
VEC_DOT = {t: "ggml_vec_dot_%s_q8_0" % NAME[t] for t in TYPES}
DEQUANT = {t: "dequantize_row_%s" % NAME[t] for t in TYPES}
SGEMM_TYPES = (Q8_0, Q4_0)                      # llamafile_sgemm serves these two (sgemm.cpp:961-1007); Q5_0 goes through ggml_vec_dot
KS = [256, 512, 4096, 11008]
SCALES = (1e-3, 1.0, 50.0)
ROWS = 32
EDGE_K = 1024
EDGE_WKINDS = {Q8_0: ("random", "neg_d", "zero_d", "subnormal_d", "big_d", "quants_min", "quants_max"),
               Q4_0: ("random", "neg_d", "zero_d", "subnormal_d", "big_d", "quants_min", "quants_max"),
               Q5_0: ("random", "neg_d", "zero_d", "subnormal_d", "big_d", "quants_min", "quants_max", "qh_0", "qh_1")}
EDGE_AKINDS = ("random", "zero", "neg_max", "ties", "tiny", "single")
EDGE_NVEC = 6
DEQ_ROWS = (0, 15, 31)
SGEMM_COLS = lambda n: [(2 * j + 1) % n for j in range(5)]      # which vectors form the five columns of the n = 5 llamafile_sgemm call
REF = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "libggml_ref.so")


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def _digest(blocks, xs):
    h = hashlib.sha256(np.ascontiguousarray(blocks).tobytes())
    for x in xs:
        h.update(np.ascontiguousarray(x, np.float32).tobytes())
    return h.hexdigest()


def rand_case(t, K):
    """32 rows of random raw blocks (every byte pattern of qs / qh; finite positive f16 d), three activation magnitudes"""
    from booster_amd.gguf import random_q0_tensor
    rng = np.random.default_rng(6007 * t + K)
    blocks = random_q0_tensor(t, K, ROWS, rng)
    xs = [(rng.standard_normal(K) * s).astype(np.float32) for s in SCALES]
    return blocks, xs, _digest(blocks, xs)


def _f16(v):
    return np.asarray([v], np.float16).view(np.uint8)


def _cycle(kinds, n, rng):
    tags = np.array([kinds[i % len(kinds)] for i in range(n)], dtype=object)
    rng.shuffle(tags)
    return tags


def edge_blocks(t, K, rows, rng, kinds=None):
    """raw blocks with one edge kind per 32-block (all kinds in a shuffled cycle): d negative, +-0, f16-subnormal, large; all quants at the low / high end
    (Q8_0: -128 / 127; Q4_0: nibbles 0 / 15; Q5_0: nibbles and qh bits all 0 / all 1); Q5_0 qh all 0 / all 1 under random nibbles.
    Returns (bytes, tags [rows][K/32])."""
    from booster_amd.gguf import random_q0_tensor
    kinds = kinds or EDGE_WKINDS[t]
    nb = K // 32
    blk = random_q0_tensor(t, K, rows, rng).reshape(rows * nb, BB[t]).copy()
    tags = _cycle(kinds, rows * nb, rng)
    qo = QS_OFF[t]
    for b, k in enumerate(tags):
        d = float(blk[b, 0:2].copy().view(np.float16)[0])
        if k == "neg_d":
            blk[b, 0:2] = _f16(-d)
        elif k == "zero_d":
            blk[b, 0:2] = _f16(-0.0 if rng.random() < 0.5 else 0.0)
        elif k == "subnormal_d":
            blk[b, 0:2] = np.array([int(rng.integers(1, 256)), int(rng.integers(0, 4)) | (0x80 if rng.random() < 0.5 else 0)], np.uint8)
        elif k == "big_d":
            blk[b, 0:2] = _f16((1.0 if rng.random() < 0.5 else -1.0) * rng.uniform(100.0, 2000.0))
        elif k == "quants_min":
            blk[b, qo:] = 0x80 if t == Q8_0 else 0x00
            if t == Q5_0: blk[b, 2:6] = 0x00
        elif k == "quants_max":
            blk[b, qo:] = 0x7f if t == Q8_0 else 0xff
            if t == Q5_0: blk[b, 2:6] = 0xff
        elif k == "qh_0":
            blk[b, 2:6] = 0x00
        elif k == "qh_1":
            blk[b, 2:6] = 0xff
        elif k != "random":
            raise ValueError(k)
    return blk.reshape(-1), tags.reshape(rows, nb)


def edge_activations(K, rng, kind_of):
    """an activation vector with one kind per 32-block:
      zero     all zero (id = 0, d = 0)
      neg_max  the extremum is negative (the block maximum is of |x|)
      ties     amax = 127 exactly (id = 1), every other value an odd multiple of 0.5: x * id lands on .5 and rounds to even
      tiny     |x| <= ~2e-6: d = amax / 127 is an f16 subnormal or zero while the quants are not
      single   one non-zero value"""
    x = np.zeros(K, np.float32)
    for b, k in enumerate(kind_of):
        v = (rng.standard_normal(32) * 10.0 ** rng.uniform(-2, 2)).astype(np.float32)
        if k == "zero":
            v[:] = 0.0
        elif k == "neg_max":
            v = np.abs(v); v[int(rng.integers(0, 32))] = -2.0 * v.max() - 1.0
        elif k == "ties":
            v = (rng.integers(-126, 126, 32) + 0.5).astype(np.float32)
            v[int(rng.integers(0, 32))] = 127.0 if rng.random() < 0.5 else -127.0
        elif k == "tiny":
            v = (rng.standard_normal(32) * 10.0 ** rng.uniform(-9, -6)).astype(np.float32)
        elif k == "single":
            j = int(rng.integers(0, 32)); s = v[j] if v[j] != 0 else np.float32(1.0); v[:] = 0.0; v[j] = s
        elif k != "random":
            raise ValueError(k)
        x[32 * b:32 * b + 32] = v
    return x


def edge_case(t):
    rng = np.random.default_rng(130003 + t)
    blocks, wtags = edge_blocks(t, EDGE_K, ROWS, rng)
    nb = EDGE_K // 32
    xt = _cycle(EDGE_AKINDS, EDGE_NVEC * nb, rng).reshape(EDGE_NVEC, nb)
    xs = [edge_activations(EDGE_K, rng, xt[i]) for i in range(EDGE_NVEC)]
    return blocks, xs, _digest(blocks, xs), wtags, xt


def all_cases(t):
    """(key, blocks, activation vectors, inputs digest, rows whose dequantisation is stored) of every stored case of type t"""
    for K in KS:
        blocks, xs, digest = rand_case(t, K)
        yield "%s_K%d" % (NAME[t], K), blocks, xs, digest, DEQ_ROWS
    blocks, xs, digest, _, _ = edge_case(t)
    yield "%s_edge" % NAME[t], blocks, xs, digest, tuple(range(ROWS))


# ---- activations ----------------------------------------------------------------------------------------------------------------------------
def quantize_row_q8_0(x):
    """block_q8_0 bytes {f16 d, i8 qs[32]} of an f32 vector (AVX2 branch: ggml-quants.c:936-994)"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 32)
    with np.errstate(all="ignore"):
        amax = np.abs(x).max(axis=1)
        d = (amax / np.float32(127.0)).astype(np.float32)
        idv = np.where(amax != 0, np.float32(127.0) / amax, np.float32(0.0)).astype(np.float32)
        q = np.rint((x * idv[:, None]).astype(np.float32)).astype(np.int32)        # f32 product, then round half to even
    assert np.abs(q).max(initial=0) <= 127
    out = np.zeros((x.shape[0], 34), np.uint8)
    out[:, 0:2] = d.astype(np.float16).view(np.uint8).reshape(-1, 2)
    out[:, 2:] = q.astype(np.int8).view(np.uint8)
    return out.reshape(-1)


def q8_0_fields(q8):
    b = np.asarray(q8, np.uint8).reshape(-1, 34)
    return np.ascontiguousarray(b[:, 0:2]).view(np.float16).reshape(-1).astype(np.float32), b[:, 2:].copy().view(np.int8).astype(np.int32)


# ---- weights --------------------------------------------------------------------------------------------------------------------------------
def unpack(t, raw):
    """raw blocks -> (d f32 [n], q int32 [n][32]) with the offsets applied (Q4_0: nibble - 8, Q5_0: 5 bits - 16)"""
    b = np.asarray(raw, np.uint8).reshape(-1, BB[t])
    d = np.ascontiguousarray(b[:, 0:2]).view(np.float16).reshape(-1).astype(np.float32)
    if t == Q8_0:
        return d, b[:, 2:].copy().view(np.int8).astype(np.int32)
    qs = b[:, QS_OFF[t]:].astype(np.int32)
    q = np.concatenate([qs & 15, qs >> 4], axis=1)                              # elements 0-15 low nibbles, 16-31 high nibbles
    if t == Q4_0:
        return d, q - 8
    qh = np.ascontiguousarray(b[:, 2:6]).view(np.uint32).reshape(-1).astype(np.int64)
    bit = ((qh[:, None] >> np.arange(32)) & 1).astype(np.int32)
    return d, (q | (bit << 4)) - 16


def dequantize(t, raw):
    """dequantize_row_q*_0: y = (float) q * d, one f32 product"""
    d, q = unpack(t, raw)
    with np.errstate(all="ignore"):
        return (q.astype(np.float32) * d[:, None]).astype(np.float32).reshape(-1)


# ---- the chain ------------------------------------------------------------------------------------------------------------------------------
def vec_dot_rows(t, raw, q8):
    """the reference's dot product of every row with the Q8_0 vector: float32 [rows]"""
    yd, qa = q8_0_fields(q8)
    nb = yd.size
    wd, wq = unpack(t, raw)
    rows = wd.size // nb
    wd = wd.reshape(rows, nb); wq = wq.reshape(rows, nb, 8, 4)
    dots = (wq * qa.reshape(1, nb, 8, 4)).sum(axis=3)                          # exact: lane e = elements 4e .. 4e+3
    assert np.abs(dots).max(initial=0) <= 4 * 128 * 127
    acc = np.zeros((rows, 8), np.float32)
    with np.errstate(all="ignore"):
        for l in range(nb):
            s = (wd[:, l] * yd[l]).astype(np.float32)
            acc = fma32(s[:, None], dots[:, l].astype(np.float32), acc)
        r = acc[:, 0:4] + acc[:, 4:8]                                          # hsum (sgemm.cpp:63-76 = hsum_float_8, ggml-quants.c:47-53)
        r = r[:, 0:2] + r[:, 2:4]
        return (r[:, 0] + r[:, 1]).astype(np.float32)


def mul_mat(t, W, rows, K, x, chunk=1024):
    """y = W . Q8_0(x) as the reference computes it"""
    W = np.asarray(W, np.uint8)
    rb = K // 32 * BB[t]
    assert W.size == rows * rb
    q8 = quantize_row_q8_0(x)
    return np.concatenate([vec_dot_rows(t, W[r * rb:min(rows, r + chunk) * rb], q8) for r in range(0, rows, chunk)])


# ---- the genuine reference, where it is built (oracle/_ref/libggml_ref.so: `make -C oracle ref`) ---------------------------------------------------
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
    L.quantize_row_q8_0.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    for n in VEC_DOT.values():
        getattr(L, n).argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]
    for n in DEQUANT.values():
        getattr(L, n).argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.llamafile_sgemm.restype = C.c_bool
    L.llamafile_sgemm.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    return L


def reference_outputs(L, t, blocks, xs, deq_rows):
    """the live reference: dots f32 [vectors][rows] of ggml_vec_dot, sha256 of its Q8_0 bytes per vector, dequantised rows f32 [len(deq_rows)][K], and for
    Q8_0 / Q4_0 the llamafile_sgemm outputs at n = 1 (every vector on its own: [vectors][rows]) and at n = 5 (columns = vectors SGEMM_COLS(len(xs)), all
    at once: [5][rows]), else None"""
    K = xs[0].size
    rb = K // 32 * BB[t]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    blocks = np.ascontiguousarray(blocks, np.uint8)
    dots = np.zeros((len(xs), ROWS), np.float32)
    q8all = np.zeros((len(xs), K // 32 * 34), np.uint8)
    q8sha = []
    for i, x in enumerate(xs):
        L.quantize_row_q8_0(p(np.ascontiguousarray(x, np.float32)), p(q8all[i]), K)
        q8sha.append(hashlib.sha256(q8all[i].tobytes()).hexdigest())
        for r in range(ROWS):
            s = C.c_float(0)
            getattr(L, VEC_DOT[t])(K, C.byref(s), 0, C.c_void_p(blocks.ctypes.data + r * rb), 0, p(q8all[i]), 0, 1)
            dots[i, r] = s.value
    deq = np.zeros((len(deq_rows), K), np.float32)
    for i, r in enumerate(deq_rows):
        getattr(L, DEQUANT[t])(C.c_void_p(blocks.ctypes.data + r * rb), p(deq[i]), K)
    sg1 = sgn = None
    if t in SGEMM_TYPES:
        sg1 = np.zeros((len(xs), ROWS), np.float32); sgn = np.zeros((5, ROWS), np.float32)
        for i in range(len(xs)):
            assert L.llamafile_sgemm(ROWS, 1, K // 32, p(blocks), K // 32, p(q8all[i]), K // 32, p(sg1[i]), ROWS, 0, 1, t, Q8_0, 0)
        q85 = np.ascontiguousarray(q8all[SGEMM_COLS(len(xs))])
        assert L.llamafile_sgemm(ROWS, 5, K // 32, p(blocks), K // 32, p(q85), K // 32, p(sgn), ROWS, 0, 1, t, Q8_0, 0)
    return dots, q8sha, deq, sg1, sgn
