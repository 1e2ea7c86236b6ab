"""Q4_1 / Q5_1 (Q8_1 activations): seeded inputs of their tests and a numpy restatement of what the kernels compute — the reference's AVX2
quantize_row_q8_1 (ggml-quants.c:1272-1333), ggml_vec_dot_q4_1_q8_1 (:4344-4377), ggml_vec_dot_q5_1_q8_1 (:5009-5034) and dequantize_row_q4_1 / q5_1
(:1535-1551, :1582-1604).  llamafile_sgemm has no case for these types (sgemm.cpp:961-1007), so one token and many go through ggml_vec_dot.

The restatement is held to the genuine reference's outputs stored in tests/golden/legacy1_kats.npz (tests/golden/gen_legacy1_kats.py, tests/test_legacy1_ref.py).

Activations: quantize_row_q8_0's d, id and bytes (legacy_ref.quantize_row_q8_0), plus s = f16(d_f32 * (float) sum(q)): the UNROUNDED f32 d times the exact
integer sum of the block's 32 quants (|sum| <= 4064); s overflows to +-inf from |d * sum| >= 65520.
Weights: unsigned quants (Q4_1: the nibble 0..15; Q5_1: nibble | qh bit << 4, 0..31), value = q * d + m.
One dot product = TWO accumulators over the 32-blocks l = 0 .. K/32 - 1 in order:
    the eight SIMD lanes e of the Q8_0 family:  acc_e = fma(f32(d_w[l]) * f32(d_x[l]), (float) dot4_e[l], acc_e)       (|dot4| <= 4 * 31 * 127: exact in f32)
    one scalar per row:                         summs = summs + f32(m_w[l]) * f32(s_x[l])
and the result hsum(acc) + summs.

WHAT THE RECORDED ANSWERS DECIDED: whether the pinned reference build (oracle flavour A2: -O3 -std=c11 -march=x86-64-v3) evaluates the scalar statement
`summs += a * b`, and `x * d + m` in dequantize_row_q4_1 / _q5_1, as a separate multiply and add or as a fused multiply-add CANNOT be told from its outputs,
and does not matter: the restatement reproduces every stored output bit for bit with EITHER form (tests/test_legacy1_ref.py runs both).  The reason is that
each of these products is exact in f32 — m_w and s_x are widened f16 values (11 significant bits each: 22 in the product, exponent within [-48, 32]), and
x * d is an integer below 32 times a widened f16 (16 bits) — so rounding the product first changes nothing.  The restatement and the kernels use the
separate form (CONTRACTED = False below; the kernels are compiled with -ffp-contract=off)."""
import ctypes as C
import hashlib

import numpy as np

import legacy_ref as lg
from lowbit_ref import fma32

Q4_1, Q5_1 = 3, 7
TYPES = (Q4_1, Q5_1)
BB = {Q4_1: 20, Q5_1: 24}
QS_OFF = {Q4_1: 4, Q5_1: 8}
QMAX = {Q4_1: 15, Q5_1: 31}
NAME = {Q4_1: "q4_1", Q5_1: "q5_1"}
VEC_DOT = {t: "ggml_vec_dot_%s_q8_1" % NAME[t] for t in TYPES}
DEQUANT = {t: "dequantize_row_%s" % NAME[t] for t in TYPES}
CONTRACTED = False                              # see the module text: the form used; the fused one gives the same bits
KS = [256, 512, 4096, 11008]
SCALES = (1e-3, 1.0, 50.0)
ROWS = 32
EDGE_K = 1024
EDGE_WKINDS = {Q4_1: ("random", "neg_d", "zero_d", "subnormal_d", "big_d", "zero_m", "neg_m", "big_m", "quants_min", "quants_max"),
               Q5_1: ("random", "neg_d", "zero_d", "subnormal_d", "big_d", "zero_m", "neg_m", "big_m", "quants_min", "quants_max", "qh_0", "qh_1")}
EDGE_AKINDS = lg.EDGE_AKINDS + ("equal",)
EDGE_NVEC = 6
DEQ_ROWS = (0, 15, 31)
OVERFLOW_K = 256
REF = lg.REF


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def rand_case(t, K):
    """32 rows of random raw blocks (every byte pattern of qs / qh; finite f16 d and m of either sign), three activation magnitudes"""
    from booster_amd.gguf import random_q1_tensor
    rng = np.random.default_rng(7001 * t + K)
    blocks = random_q1_tensor(t, K, ROWS, rng)
    xs = [(rng.standard_normal(K) * s).astype(np.float32) for s in SCALES]
    return blocks, xs, lg._digest(blocks, xs)


def edge_blocks(t, K, rows, rng, kinds=None):
    """raw blocks with one edge kind per 32-block (all kinds in a shuffled cycle): d negative, +-0, f16-subnormal, large; m +-0, negative, large; all quants
    0 / all 15 (Q4_1) or 31 (Q5_1: nibbles and qh bits all 1); Q5_1 qh all 0 / all 1 under random nibbles.  Returns (bytes, tags [rows][K/32])."""
    from booster_amd.gguf import random_q1_tensor
    kinds = kinds or EDGE_WKINDS[t]
    nb = K // 32
    blk = random_q1_tensor(t, K, rows, rng).reshape(rows * nb, BB[t]).copy()
    tags = lg._cycle(kinds, rows * nb, rng)
    qo = QS_OFF[t]
    for b, k in enumerate(tags):
        d = float(blk[b, 0:2].copy().view(np.float16)[0])
        m = float(blk[b, 2:4].copy().view(np.float16)[0])
        sign = 1.0 if rng.random() < 0.5 else -1.0
        if k == "neg_d":
            blk[b, 0:2] = lg._f16(-abs(d))
        elif k == "zero_d":
            blk[b, 0:2] = lg._f16(-0.0 if rng.random() < 0.5 else 0.0)
        elif k == "subnormal_d":
            blk[b, 0:2] = np.array([int(rng.integers(1, 256)), int(rng.integers(0, 4)) | (0x80 if rng.random() < 0.5 else 0)], np.uint8)
        elif k == "big_d":
            blk[b, 0:2] = lg._f16(sign * rng.uniform(100.0, 2000.0))
        elif k == "zero_m":
            blk[b, 2:4] = lg._f16(-0.0 if rng.random() < 0.5 else 0.0)
        elif k == "neg_m":
            blk[b, 2:4] = lg._f16(-abs(m) - 1e-3)
        elif k == "big_m":
            blk[b, 2:4] = lg._f16(sign * rng.uniform(100.0, 2000.0))
        elif k == "quants_min":
            blk[b, qo:] = 0x00
            if t == Q5_1: blk[b, 4:8] = 0x00
        elif k == "quants_max":
            blk[b, qo:] = 0xff
            if t == Q5_1: blk[b, 4:8] = 0xff
        elif k == "qh_0":
            blk[b, 4:8] = 0x00
        elif k == "qh_1":
            blk[b, 4:8] = 0xff
        elif k != "random":
            raise ValueError(k)
    return blk.reshape(-1), tags.reshape(rows, nb)


def edge_activations(K, rng, kind_of):
    """legacy_ref.edge_activations' kinds (zero, neg_max, ties, tiny, single, random) and
      equal    32 equal values v, 0.5 <= |v| <= 1000: every quant is +-127, |sum| = 4064, s = f16(32 v) is finite"""
    x = lg.edge_activations(K, rng, ["zero" if k == "equal" else k for k in kind_of])
    for b, k in enumerate(kind_of):
        if k == "equal":
            x[32 * b:32 * b + 32] = np.float32((1.0 if rng.random() < 0.5 else -1.0) * rng.uniform(0.5, 1000.0))
    return x


def edge_case(t):
    rng = np.random.default_rng(170003 + t)
    blocks, wtags = edge_blocks(t, EDGE_K, ROWS, rng)
    nb = EDGE_K // 32
    xt = lg._cycle(EDGE_AKINDS, EDGE_NVEC * nb, rng).reshape(EDGE_NVEC, nb)
    xs = [edge_activations(EDGE_K, rng, xt[i]) for i in range(EDGE_NVEC)]
    return blocks, xs, lg._digest(blocks, xs), wtags, xt


def overflow_vector():
    """one activation vector used in NO dot: block 3 holds 32 equal values of 4096, so d * sum = 32 * 4096 overflows f16 and s = +inf; block 5 the same with
    -4096 (s = -inf); the other blocks are random.  Stored by the digest of the reference's quantize_row_q8_1 bytes only."""
    rng = np.random.default_rng(4096)
    x = (rng.standard_normal(OVERFLOW_K) * 3.0).astype(np.float32)
    x[96:128] = 4096.0
    x[160:192] = -4096.0
    return x


ROUND2_K = 2048


def double_rounding_vector():
    """one activation vector used in NO dot, every one of whose 64 blocks is a double-rounding case of s: f16(f32(d * sum)) — the reference rounds the
    product to f32 first, then to f16 — differs from f16(d * sum) rounded once from the exact product.  About one random block in a thousand is one; these
    are the first 64 of a seeded stream.  A quantiser that folds the multiply into the conversion gives other bytes.  Stored by the digest of the
    reference's quantize_row_q8_1 bytes only."""
    rng = np.random.default_rng(2222)
    found = []
    while len(found) < ROUND2_K // 32:
        xb = (rng.standard_normal((1 << 16, 32)) * 3.0).astype(np.float32)
        amax = np.abs(xb).max(axis=1)
        d = (amax / np.float32(127.0)).astype(np.float32)
        q = np.rint((xb * (np.float32(127.0) / amax)[:, None]).astype(np.float32)).astype(np.int64).sum(axis=1)
        twice = (d * q.astype(np.float32)).astype(np.float32).astype(np.float16)
        once = (d.astype(np.float64) * q).astype(np.float16)
        found.extend(xb[twice.view(np.uint16) != once.view(np.uint16)])
    return np.concatenate(found[:ROUND2_K // 32]).astype(np.float32)


def all_cases(t):
    """(key, blocks, activation vectors, inputs digest, rows whose dequantisation is stored) of every stored case of type t"""
    for K in KS:
        blocks, xs, digest = rand_case(t, K)
        yield "%s_K%d" % (NAME[t], K), blocks, xs, digest, DEQ_ROWS
    blocks, xs, digest, _, _ = edge_case(t)
    yield "%s_edge" % NAME[t], blocks, xs, digest, tuple(range(ROWS))


# ---- activations ----------------------------------------------------------------------------------------------------------------------------
def quantize_row_q8_1(x):
    """block_q8_1 bytes {f16 d, f16 s, i8 qs[32]} of an f32 vector (AVX2 branch: ggml-quants.c:1272-1333)"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 32)
    with np.errstate(all="ignore"):
        amax = np.abs(x).max(axis=1)
        d = (amax / np.float32(127.0)).astype(np.float32)
        idv = np.where(amax != 0, np.float32(127.0) / amax, np.float32(0.0)).astype(np.float32)
        q = np.rint((x * idv[:, None]).astype(np.float32)).astype(np.int32)        # f32 product, then round half to even
        qsum = q.sum(axis=1)                                                       # exact
        s = (d * qsum.astype(np.float32)).astype(np.float32)                       # the unrounded f32 d; int -> float is exact
        out = np.zeros((x.shape[0], 36), np.uint8)
        out[:, 0:2] = d.astype(np.float16).view(np.uint8).reshape(-1, 2)
        out[:, 2:4] = s.astype(np.float16).view(np.uint8).reshape(-1, 2)           # round to nearest even, overflow to +-inf (F16C)
    assert np.abs(q).max(initial=0) <= 127 and np.abs(qsum).max(initial=0) <= 4064
    out[:, 4:] = q.astype(np.int8).view(np.uint8)
    return out.reshape(-1)


def q8_1_fields(q8):
    """(d f32 [n], s f32 [n], q int32 [n][32])"""
    b = np.asarray(q8, np.uint8).reshape(-1, 36)
    h = np.ascontiguousarray(b[:, 0:4]).view(np.float16).reshape(-1, 2).astype(np.float32)
    return h[:, 0].copy(), h[:, 1].copy(), b[:, 4:].copy().view(np.int8).astype(np.int32)


def q8_1_as_q8_0(q8):
    """the block_q8_0 bytes with the same d and quants"""
    b = np.asarray(q8, np.uint8).reshape(-1, 36)
    return np.concatenate([b[:, 0:2], b[:, 4:]], axis=1).reshape(-1)


# ---- weights --------------------------------------------------------------------------------------------------------------------------------
def unpack(t, raw):
    """raw blocks -> (d f32 [n], m f32 [n], q int32 [n][32]), q unsigned and without an offset"""
    b = np.asarray(raw, np.uint8).reshape(-1, BB[t])
    h = np.ascontiguousarray(b[:, 0:4]).view(np.float16).reshape(-1, 2).astype(np.float32)
    qs = b[:, QS_OFF[t]:].astype(np.int32)
    q = np.concatenate([qs & 15, qs >> 4], axis=1)                              # elements 0-15 low nibbles, 16-31 high nibbles
    if t == Q5_1:
        qh = np.ascontiguousarray(b[:, 4:8]).view(np.uint32).reshape(-1).astype(np.int64)
        q = q | ((((qh[:, None] >> np.arange(32)) & 1).astype(np.int32)) << 4)
    return h[:, 0].copy(), h[:, 1].copy(), q


def dequantize(t, raw, contracted=CONTRACTED):
    """dequantize_row_q*_1: y = q * d + m"""
    d, m, q = unpack(t, raw)
    with np.errstate(all="ignore"):
        qf = q.astype(np.float32)
        if contracted:
            return fma32(qf, np.broadcast_to(d[:, None], qf.shape), np.broadcast_to(m[:, None], qf.shape)).astype(np.float32).reshape(-1)
        return ((qf * d[:, None]).astype(np.float32) + m[:, None]).astype(np.float32).reshape(-1)


# ---- the chains -----------------------------------------------------------------------------------------------------------------------------
def vec_dot_rows(t, raw, q8, contracted=CONTRACTED):
    """the reference's dot product of every row with the Q8_1 vector: float32 [rows]"""
    yd, ysum, qa = q8_1_fields(q8)
    nb = yd.size
    wd, wm, wq = unpack(t, raw)
    rows = wd.size // nb
    wd = wd.reshape(rows, nb); wm = wm.reshape(rows, nb); wq = wq.reshape(rows, nb, 8, 4)
    dots = (wq * qa.reshape(1, nb, 8, 4)).sum(axis=3)                          # exact: lane e = elements 4e .. 4e+3
    assert np.abs(dots).max(initial=0) <= 4 * 31 * 127
    acc = np.zeros((rows, 8), np.float32)
    summs = np.zeros(rows, np.float32)
    with np.errstate(all="ignore"):
        for l in range(nb):
            s = (wd[:, l] * yd[l]).astype(np.float32)
            acc = fma32(s[:, None], dots[:, l].astype(np.float32), acc)
            if contracted:
                summs = fma32(wm[:, l], np.full(rows, ysum[l], np.float32), summs).astype(np.float32)
            else:
                summs = (summs + (wm[:, l] * ysum[l]).astype(np.float32)).astype(np.float32)
        r = acc[:, 0:4] + acc[:, 4:8]                                          # hsum_float_8 (ggml-quants.c:47-53)
        r = r[:, 0:2] + r[:, 2:4]
        return ((r[:, 0] + r[:, 1]).astype(np.float32) + summs).astype(np.float32)


def mul_mat(t, W, rows, K, x, chunk=1024):
    """y = W . Q8_1(x) as the reference computes it"""
    W = np.asarray(W, np.uint8)
    rb = K // 32 * BB[t]
    assert W.size == rows * rb
    q8 = quantize_row_q8_1(x)
    return np.concatenate([vec_dot_rows(t, W[r * rb:min(rows, r + chunk) * rb], q8) for r in range(0, rows, chunk)])


# ---- the genuine reference, where it is built (oracle/_ref/libggml_ref.so: `make -C oracle ref`) ---------------------------------------------------
def load_ref():
    """the reference library, or None where it is not built"""
    L = lg.load_ref()
    if L is None:
        return None
    L.quantize_row_q8_1.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    for n in VEC_DOT.values():
        getattr(L, n).argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]
    for n in DEQUANT.values():
        getattr(L, n).argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    return L


def reference_q8_1(L, x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros(x.size // 32 * 36, np.uint8)
    L.quantize_row_q8_1(x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), x.size)
    return out


def reference_outputs(L, t, blocks, xs, deq_rows):
    """the live reference: dots f32 [vectors][rows] of ggml_vec_dot, sha256 of its Q8_1 bytes per vector, dequantised rows f32 [len(deq_rows)][K]"""
    K = xs[0].size
    rb = K // 32 * BB[t]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    blocks = np.ascontiguousarray(blocks, np.uint8)
    dots = np.zeros((len(xs), ROWS), np.float32)
    q8sha = []
    for i, x in enumerate(xs):
        q8 = reference_q8_1(L, x)
        q8sha.append(hashlib.sha256(q8.tobytes()).hexdigest())
        for r in range(ROWS):
            s = C.c_float(0)
            getattr(L, VEC_DOT[t])(K, C.byref(s), 0, C.c_void_p(blocks.ctypes.data + r * rb), 0, p(q8), 0, 1)
            dots[i, r] = s.value
    deq = np.zeros((len(deq_rows), K), np.float32)
    for i, r in enumerate(deq_rows):
        getattr(L, DEQUANT[t])(C.c_void_p(blocks.ctypes.data + r * rb), p(deq[i]), K)
    return dots, q8sha, deq
