"""Q3_K / Q2_K: seeded inputs of the low-bit tests and a numpy restatement of what the kernels compute — the reference's AVX2
ggml_vec_dot_q3_K_q8_K / ggml_vec_dot_q2_K_q8_K (ggml-quants.c:6161-6263, :5553-5617) and dequantize_row_q3_K / _q2_K (:2320, :1972).

The restatement is independent of oracle/booster_oracle.c (which has no Q2_K / Q3_K) and is itself held to the genuine reference's outputs
stored in tests/golden/lowbit_kats.npz (tests/golden/gen_lowbit_kats.py, tests/test_lowbit_ref.py).

One dot product = eight SIMD lanes e, each ONE sequential f32 fma chain over the super-blocks, closed by hsum_float_8:
  Q3_K: acc_e = fma(d, (float) sumi_e, acc_e)
  Q2_K: acc_e = fma(dmin, (float) prod_e, acc_e); acc_e = fma(d, (float) sumi_e, acc_e)        (the same accumulator, min term first)
with d = y.d * f16(x.d), dmin = -y.d * f16(x.dmin) (f32 products), sumi_e the exact integer sum over the elements n of the super-block with
(n & 31) >> 2 == e of scale[n >> 4] * q[n] * q8[n], and prod_e = mins[2e] * bsums[2e] + mins[2e+1] * bsums[2e+1].

The fma is EXACT: the f32 product is exact in float64, the float64 sum is corrected to round-to-odd with the error term of TwoSum, and a
round-to-odd value of 53 bits rounds to the correctly rounded 24-bit result (a plain float64 add would round twice).
"""
import ctypes as C
import hashlib
import os

import numpy as np

import edge_inputs as ei

Q2_K, Q3_K = 10, 11
BB = {Q2_K: 84, Q3_K: 110}
D_OFF = {Q2_K: 80, Q3_K: 108}
VEC_DOT = {Q2_K: "ggml_vec_dot_q2_K_q8_K", Q3_K: "ggml_vec_dot_q3_K_q8_K"}
DEQUANT = {Q2_K: "dequantize_row_q2_K", Q3_K: "dequantize_row_q3_K"}
KS = [256, 1024, 14336, 11008]                 # 11008: 43 super-blocks (the Llama-2-7B ffn_down)
SCALES = (1e-3, 1.0, 50.0)
ROWS = 32
EDGE_K = 1024
EDGE_WKINDS = {Q3_K: ("random", "neg_d", "zero_d", "subnormal_d", "big_d", "scales_lo", "scales_hi", "quants_min", "quants_max", "hmask_0", "hmask_1"),
               Q2_K: ("random", "neg_d", "zero_d", "subnormal_d", "big_d", "neg_dmin", "zero_dmin", "subnormal_dmin", "big_dmin", "scales_lo", "scales_hi",
                      "quants_min", "quants_max")}
EDGE_AKINDS = ("random", "constant", "zero", "single", "opposite_max", "ties")
EDGE_NVEC = 6
# per SIMD lane and super-block: |sumi| <= 32 * 4 * 128 * 32 (Q3_K), 32 * 3 * 128 * 15 (Q2_K), |prod| <= 2 * 15 * 2048: all below 2^24, so int -> f32 is exact
SUMI_BOUND = {Q3_K: 32 * 4 * 128 * 32, Q2_K: 32 * 3 * 128 * 15}
PROD_BOUND = 2 * 15 * 2048


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def _digest(blocks, xs):
    h = hashlib.sha256(np.ascontiguousarray(blocks).tobytes())
    for x in xs:
        h.update(np.ascontiguousarray(x, np.float32).tobytes())
    return h.hexdigest()


def rand_case(t, K):
    """32 rows of random raw blocks (every bit pattern of scales, quants and hmask; well-formed f16 d / dmin), three activation magnitudes"""
    from booster_amd.gguf import random_kquant_tensor
    rng = np.random.default_rng(7919 * t + K)
    blocks = random_kquant_tensor(t, K, ROWS, rng)
    xs = [(rng.standard_normal(K) * s).astype(np.float32) for s in SCALES]
    return blocks, xs, _digest(blocks, xs)


def _f16(v):
    return np.asarray([v], np.float16).view(np.uint8)


def edge_blocks(t, K, rows, rng, kinds=None):
    """raw blocks with one edge kind per super-block (all kinds in a shuffled cycle): d / dmin negative, zero, f16-subnormal, large; all scales at
    either end of their range (Q3_K: 0 and 63 before the - 32; Q2_K: scale and min nibbles 0 and 15); all quants at min / max; hmask all 0 / all 1.
    Returns (bytes, tags [rows][K/256])."""
    from booster_amd.gguf import random_kquant_tensor
    kinds = kinds or EDGE_WKINDS[t]
    nb = K // 256
    blk = random_kquant_tensor(t, K, rows, rng).reshape(rows * nb, BB[t]).copy()
    tags = ei._cycle(kinds, rows * nb, rng)
    do = D_OFF[t]
    for b, k in enumerate(tags):
        d = float(blk[b, do:do + 2].copy().view(np.float16)[0])
        if k == "neg_d":
            blk[b, do:do + 2] = _f16(-d)
        elif k == "zero_d":
            blk[b, do:do + 2] = _f16(-0.0 if rng.random() < 0.5 else 0.0)
        elif k == "subnormal_d":
            blk[b, do:do + 2] = np.array([int(rng.integers(1, 256)), int(rng.integers(0, 4)) | (0x80 if rng.random() < 0.5 else 0)], np.uint8)
        elif k == "big_d":
            blk[b, do:do + 2] = _f16(ei._sign(rng) * rng.uniform(1000.0, 60000.0))
        elif k in ("neg_dmin", "zero_dmin", "subnormal_dmin", "big_dmin"):
            m = float(blk[b, 82:84].copy().view(np.float16)[0])
            blk[b, 82:84] = {"neg_dmin": _f16(-m), "zero_dmin": _f16(-0.0 if rng.random() < 0.5 else 0.0),
                             "subnormal_dmin": np.array([int(rng.integers(1, 256)), int(rng.integers(0, 4))], np.uint8),
                             "big_dmin": _f16(ei._sign(rng) * rng.uniform(1000.0, 60000.0))}[k]
        elif k == "scales_lo":
            if t == Q3_K: blk[b, 96:108] = 0
            else: blk[b, 0:16] = 0
        elif k == "scales_hi":
            if t == Q3_K: blk[b, 96:108] = 0xff
            else: blk[b, 0:16] = 0xff
        elif k == "quants_min":                                   # Q3_K: low2 = 0, hbit = 0 -> -4; Q2_K: 0
            if t == Q3_K: blk[b, 0:32] = 0; blk[b, 32:96] = 0
            else: blk[b, 16:80] = 0
        elif k == "quants_max":                                   # Q3_K: low2 = 3, hbit = 1 -> 3; Q2_K: 3
            if t == Q3_K: blk[b, 0:32] = 0xff; blk[b, 32:96] = 0xff
            else: blk[b, 16:80] = 0xff
        elif k == "hmask_0":
            blk[b, 0:32] = 0
        elif k == "hmask_1":
            blk[b, 0:32] = 0xff
        elif k != "random":
            raise ValueError(k)
    return blk.reshape(-1), tags.reshape(rows, nb)


def edge_case(t):
    rng = np.random.default_rng(104729 + t)
    blocks, wtags = edge_blocks(t, EDGE_K, ROWS, rng)
    nb = EDGE_K // 256
    xt = ei._cycle(EDGE_AKINDS, EDGE_NVEC * nb, rng).reshape(EDGE_NVEC, nb)
    xs = [ei.edge_activations(EDGE_K, rng, kind_of=xt[i])[0] for i in range(EDGE_NVEC)]
    return blocks, xs, _digest(blocks, xs), wtags, xt


# ---- block fields ---------------------------------------------------------------------------------------------------------------------------
def unpack(t, raw):
    """raw blocks -> dict of per-block fields: d, dmin f32 [n]; scale, mn int16 [n][16] (Q3_K: scale - 32 applied, mn = 0); q int16 [n][256]"""
    b = np.asarray(raw, np.uint8).reshape(-1, BB[t])
    n = b.shape[0]
    el = np.arange(256)
    j, k, m = el >> 7, (el >> 5) & 3, el & 31
    if t == Q3_K:
        hm, qs, sc = b[:, 0:32], b[:, 32:96], b[:, 96:108].astype(np.int16)
        d = b[:, 108:110].copy().view(np.float16).reshape(n).astype(np.float32)
        dmin = np.zeros(n, np.float32)
        idx = np.arange(16)
        low4 = np.where(idx < 8, sc[:, idx % 8] & 15, sc[:, idx % 8] >> 4)
        hi2 = (sc[:, 8 + (idx & 3)] >> (2 * (idx >> 2))) & 3
        scale = (low4 | (hi2 << 4)) - 32
        mn = np.zeros((n, 16), np.int16)
        low2 = (qs[:, 32 * j + m] >> (2 * k).astype(np.uint8)) & 3
        hbit = (hm[:, m] >> (4 * j + k).astype(np.uint8)) & 1
        q = low2.astype(np.int16) + 4 * hbit.astype(np.int16) - 4
    else:
        sc, qs = b[:, 0:16].astype(np.int16), b[:, 16:80]
        d = b[:, 80:82].copy().view(np.float16).reshape(n).astype(np.float32)
        dmin = b[:, 82:84].copy().view(np.float16).reshape(n).astype(np.float32)
        scale, mn = sc & 15, sc >> 4
        q = ((qs[:, 32 * j + m] >> (2 * k).astype(np.uint8)) & 3).astype(np.int16)
    return dict(d=d, dmin=dmin, scale=scale, mn=mn, q=q)


def dequantize(t, raw):
    """dequantize_row_q3_K / _q2_K, operation for operation in f32: dl = d * sc; y = dl * q  |  dl = d * (sc & 15); ml = dmin * (sc >> 4); y = dl * q - ml"""
    f = unpack(t, raw)
    sub = np.arange(256) >> 4
    dl = f["d"][:, None] * f["scale"].astype(np.float32)                     # f32 x f32, one rounding
    y = dl[:, sub] * f["q"].astype(np.float32)
    if t == Q2_K:
        ml = f["dmin"][:, None] * f["mn"].astype(np.float32)
        y = y - ml[:, sub]
    return y.astype(np.float32).reshape(-1)


# ---- the chains -----------------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """correctly rounded float32 fma(a, b, c), element-wise (see the module docstring)"""
    a = np.asarray(a, np.float32).astype(np.float64); b = np.asarray(b, np.float32).astype(np.float64); c = np.asarray(c, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        p = a * b                                                            # exact: 24 + 24 bits
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)                                      # TwoSum: p + c = s + err exactly
        inexact = np.isfinite(s) & (err != 0.0)
        even = (s.view(np.int64) & 1) == 0
        # the true sum lies strictly between s and its neighbour on err's side: round-to-odd takes whichever of the two has an odd last bit
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(inexact & even, np.nextafter(s, toward), s)
        return s.astype(np.float32)


def q8_fields(q8):
    return ei.q8_fields(q8)


def lane_sums(t, raw, q8):
    """exact integer parts: raw = the blocks of `rows` rows x nb super-blocks, q8 = Q8_K bytes of the activation vector.
    Returns (sumi int64 [rows][nb][8], prod int64 [rows][nb][8])"""
    yd, qa, bsums = q8_fields(q8)
    nb = yd.size
    f = unpack(t, raw)
    rows = f["q"].shape[0] // nb
    w = (f["scale"][:, np.arange(256) >> 4] * f["q"]).reshape(rows, nb, 256)
    pr = w.astype(np.int32) * qa.astype(np.int32)[None]
    sumi = pr.reshape(rows, nb, 8, 8, 4).sum(axis=(2, 4), dtype=np.int64)                  # element n = 32 c + 4 e + u: lane e
    mb = f["mn"].astype(np.int64).reshape(rows, nb, 8, 2) * bsums.astype(np.int64).reshape(1, nb, 8, 2)
    prod = mb.sum(axis=3)
    return sumi, prod


def vec_dot_rows(t, raw, q8):
    """the reference's dot product of every row with the Q8_K vector: float32 [rows]"""
    yd, _, _ = q8_fields(q8)
    nb = yd.size
    f = unpack(t, raw)
    rows = f["d"].size // nb
    sumi, prod = lane_sums(t, raw, q8)
    assert np.abs(sumi).max(initial=0) <= SUMI_BOUND[t] and np.abs(prod).max(initial=0) <= PROD_BOUND
    xd, xm = f["d"].reshape(rows, nb), f["dmin"].reshape(rows, nb)
    acc = np.zeros((rows, 8), np.float32)
    with np.errstate(all="ignore"):
        for i in range(nb):
            d = (yd[i] * xd[:, i]).astype(np.float32)
            if t == Q2_K:
                dmin = ((-yd[i]) * xm[:, i]).astype(np.float32)
                acc = fma32(dmin[:, None], prod[:, i].astype(np.float32), acc)
            acc = fma32(d[:, None], sumi[:, i].astype(np.float32), acc)
        r = acc[:, 0:4] + acc[:, 4:8]                                        # hsum_float_8 (ggml-quants.c:47-53)
        r = r[:, 0:2] + r[:, 2:4]
        return (r[:, 0] + r[:, 1]).astype(np.float32)


def mul_mat(po, t, W, rows, K, x, chunk=512):
    """y = W . Q8_K(x) as the reference computes it; Q8_K from the oracle's quantize_row_q8_K (held to the reference by tests/test_oracle_vs_ref.py)"""
    W = np.asarray(W, np.uint8)
    rb = (K // 256) * BB[t]
    assert W.size == rows * rb
    q8 = po.quantize_q8_K(np.ascontiguousarray(x, np.float32))
    return np.concatenate([vec_dot_rows(t, W[r * rb:min(rows, r + chunk) * rb], q8) for r in range(0, rows, chunk)])


# ---- the genuine reference, where it is built (oracle/_ref/libggml_ref.so: `make -C oracle ref`) ---------------------------------------------------
NAME = {Q2_K: "q2_K", Q3_K: "q3_K"}
DEQ_ROWS = (0, 15, 31)
REF = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "libggml_ref.so")


def load_ref():
    """the reference library, or None where it is not built; a library that is there and does not load is an error (a broken build of oracle/_ref)"""
    if not os.path.exists(REF):
        return None
    L = C.CDLL(REF)
    class _InitParams(C.Structure):
        _fields_ = [("mem_size", C.c_size_t), ("mem_buffer", C.c_void_p), ("no_alloc", C.c_bool)]
    L.ggml_init.restype = C.c_void_p                            # ggml_init fills the f16 -> f32 table that GGML_FP16_TO_FP32 reads on x86
    L.ggml_init.argtypes = [_InitParams]
    L.ggml_init(_InitParams(1 << 20, None, False))
    L.quantize_row_q8_K.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    for n in VEC_DOT.values():
        getattr(L, n).argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]
    for n in DEQUANT.values():
        getattr(L, n).argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    return L


def all_cases(t):
    """(key, blocks, activation vectors, inputs digest, rows whose dequantisation is stored) of every stored case of type t"""
    for K in KS:
        blocks, xs, digest = rand_case(t, K)
        yield "%s_K%d" % (NAME[t], K), blocks, xs, digest, DEQ_ROWS
    blocks, xs, digest, _, _ = edge_case(t)
    yield "%s_edge" % NAME[t], blocks, xs, digest, tuple(range(ROWS))


def reference_outputs(L, t, blocks, xs, deq_rows):
    """the live reference: dots f32 [vectors][rows], sha256 of its Q8_K bytes per vector, dequantised rows f32 [len(deq_rows)][K]"""
    K = xs[0].size
    rb = K // 256 * BB[t]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    blocks = np.ascontiguousarray(blocks, np.uint8)
    dots = np.zeros((len(xs), ROWS), np.float32)
    q8sha = []
    for i, x in enumerate(xs):
        q8r = np.zeros(K // 256 * 292, np.uint8)
        L.quantize_row_q8_K(p(x), p(q8r), K)
        q8sha.append(hashlib.sha256(q8r.tobytes()).hexdigest())
        for r in range(ROWS):
            s = C.c_float(0)
            getattr(L, VEC_DOT[t])(K, C.byref(s), 0, C.c_void_p(blocks.ctypes.data + r * rb), 0, p(q8r), 0, 1)
            dots[i, r] = s.value
    deq = np.zeros((len(deq_rows), K), np.float32)
    for i, r in enumerate(deq_rows):
        getattr(L, DEQUANT[t])(C.c_void_p(blocks.ctypes.data + r * rb), p(deq[i]), K)
    return dots, q8sha, deq
