"""IQ4_NL: seeded inputs of the IQ4_NL tests and a numpy restatement of what the kernels compute — the reference's AVX2 ggml_vec_dot_iq4_nl_q8_0
(ggml-quants.c:11596-11670, AVX2 branch :11643-11670) over quantize_row_q8_0 activations (legacy_ref.quantize_row_q8_0) and dequantize_row_iq4_nl (:3550-3566).
llamafile_sgemm has no case for the type (sgemm.cpp:865-985), so one token and many run this chain per output element.

The restatement is held to the genuine reference's outputs stored in tests/golden/iq4nl_kats.npz (tests/golden/gen_iq4nl_kats.py, tests/test_iq4nl_ref.py).

A block_iq4_nl is {f16 d, u8 qs[16]}, 18 bytes: elements 0-15 are the low nibbles, 16-31 the high ones; a nibble indexes kvalues_iq4nl (:3548).
One dot product = eight SIMD lanes e, each TWO sequential f32 fma chains, closed by a lane-wise sum and the hsum tree:
    accum1_e = fma(f32(f16 d_x[l]) * f32(f16 d_w[l]), (float) p_e[l], accum1_e)   over the EVEN blocks l = 0, 2, .. in order
    accum2_e likewise over the ODD blocks l = 1, 3, ..
    sumf = hsum_float_8(accum1 + accum2)
with p_e the exact integer dot of the table values of elements 4e .. 4e+3 with the activation bytes (|p| <= 4 * 127 * 127 < 2^24: int -> f32 is exact; the
pair sums of mul_add_epi8 are at most 2 * 127 * 127 < 32767: nothing saturates).  K is a multiple of 256 here: the block count is even, the scalar tail
loop of the reference never runs.  The fma is lowbit_ref.fma32 (exact, see there)."""
import ctypes as C
import hashlib

import numpy as np

import legacy_ref as lg
from lowbit_ref import fma32

IQ4_NL = 20
BB = 18
KVALUES = np.array([-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113], np.int32)
KS = lg.KS
SCALES = lg.SCALES
ROWS = lg.ROWS
EDGE_K = lg.EDGE_K
EDGE_WKINDS = lg.EDGE_WKINDS[lg.Q4_0]          # quants_min / quants_max: all nibbles 0 (-127) / all nibbles 15 (113)
EDGE_AKINDS = lg.EDGE_AKINDS
EDGE_NVEC = lg.EDGE_NVEC
DEQ_ROWS = lg.DEQ_ROWS
SEED = 7001                                    # chosen so that at K = 4096 the one-accumulator order differs from the reference for every magnitude (gen_iq4nl_kats.py checks)
REF = lg.REF


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def rand_case(K):
    """32 rows of random raw blocks (every nibble pattern; finite positive f16 d), three activation magnitudes"""
    from booster_amd.gguf import random_iq4_nl_tensor
    rng = np.random.default_rng(SEED * IQ4_NL + K)
    blocks = random_iq4_nl_tensor(K, ROWS, rng)
    xs = [(rng.standard_normal(K) * s).astype(np.float32) for s in SCALES]
    return blocks, xs, lg._digest(blocks, xs)


def edge_blocks(K, rows, rng):
    """legacy_ref.edge_blocks's kinds for a type whose bytes are those of Q4_0: d negative, +-0, f16-subnormal, large; all nibbles 0 / all nibbles 15"""
    from booster_amd.gguf import random_iq4_nl_tensor
    nb = K // 32
    blk = random_iq4_nl_tensor(K, rows, rng).reshape(rows * nb, BB).copy()
    tags = lg._cycle(EDGE_WKINDS, rows * nb, rng)
    for b, k in enumerate(tags):
        d = float(blk[b, 0:2].copy().view(np.float16)[0])
        if k == "neg_d":
            blk[b, 0:2] = lg._f16(-d)
        elif k == "zero_d":
            blk[b, 0:2] = lg._f16(-0.0 if rng.random() < 0.5 else 0.0)
        elif k == "subnormal_d":
            blk[b, 0:2] = np.array([int(rng.integers(1, 256)), int(rng.integers(0, 4)) | (0x80 if rng.random() < 0.5 else 0)], np.uint8)
        elif k == "big_d":
            blk[b, 0:2] = lg._f16((1.0 if rng.random() < 0.5 else -1.0) * rng.uniform(100.0, 2000.0))
        elif k == "quants_min":
            blk[b, 2:] = 0x00
        elif k == "quants_max":
            blk[b, 2:] = 0xff
        elif k != "random":
            raise ValueError(k)
    return blk.reshape(-1), tags.reshape(rows, nb)


def edge_case():
    rng = np.random.default_rng(130003 + IQ4_NL)
    blocks, wtags = edge_blocks(EDGE_K, ROWS, rng)
    nb = EDGE_K // 32
    xt = lg._cycle(EDGE_AKINDS, EDGE_NVEC * nb, rng).reshape(EDGE_NVEC, nb)
    xs = [lg.edge_activations(EDGE_K, rng, xt[i]) for i in range(EDGE_NVEC)]
    return blocks, xs, lg._digest(blocks, xs), wtags, xt


def all_cases():
    """(key, blocks, activation vectors, inputs digest, rows whose dequantisation is stored) of every stored case"""
    for K in KS:
        blocks, xs, digest = rand_case(K)
        yield "iq4_nl_K%d" % K, blocks, xs, digest, DEQ_ROWS
    blocks, xs, digest, _, _ = edge_case()
    yield "iq4_nl_edge", blocks, xs, digest, tuple(range(ROWS))


# ---- weights --------------------------------------------------------------------------------------------------------------------------------
def unpack(raw):
    """raw blocks -> (d f32 [n], nibbles int32 [n][32], table values int32 [n][32])"""
    b = np.asarray(raw, np.uint8).reshape(-1, BB)
    d = np.ascontiguousarray(b[:, 0:2]).view(np.float16).reshape(-1).astype(np.float32)
    qs = b[:, 2:].astype(np.int32)
    nib = np.concatenate([qs & 15, qs >> 4], axis=1)                            # elements 0-15 low nibbles, 16-31 high nibbles
    return d, nib, KVALUES[nib]


def dequantize(raw):
    """dequantize_row_iq4_nl: y = d * (float) kvalues_iq4nl[nibble], one f32 product"""
    d, _, q = unpack(raw)
    with np.errstate(all="ignore"):
        return (d[:, None] * q.astype(np.float32)).astype(np.float32).reshape(-1)


# ---- the chain ------------------------------------------------------------------------------------------------------------------------------
def _hsum(acc):
    r = acc[:, 0:4] + acc[:, 4:8]                                               # hsum_float_8 (ggml-quants.c:47-53)
    r = r[:, 0:2] + r[:, 2:4]
    return (r[:, 0] + r[:, 1]).astype(np.float32)


def vec_dot_rows(raw, q8, one_accumulator=False):
    """the reference's dot product of every row with the Q8_0 vector: float32 [rows].  one_accumulator: the order of the Q4_0 chain (ONE accumulator over
    all blocks) on the same terms — NOT what the reference computes for this type; tests/test_iq4nl_ref.py shows that the stored outputs tell the two apart"""
    yd, qa = lg.q8_0_fields(q8)
    nb = yd.size
    assert nb % 2 == 0
    wd, _, wq = unpack(raw)
    rows = wd.size // nb
    wd = wd.reshape(rows, nb); wq = wq.reshape(rows, nb, 8, 4)
    dots = (wq * qa.reshape(1, nb, 8, 4)).sum(axis=3)                           # exact: lane e = elements 4e .. 4e+3
    assert np.abs(dots).max(initial=0) <= 4 * 127 * 127
    acc = [np.zeros((rows, 8), np.float32), np.zeros((rows, 8), np.float32)]
    with np.errstate(all="ignore"):
        for l in range(nb):
            s = (yd[l] * wd[:, l]).astype(np.float32)                          # exact: the product of two widened f16
            a = 0 if one_accumulator else l & 1
            acc[a] = fma32(s[:, None], dots[:, l].astype(np.float32), acc[a])
        return _hsum(acc[0] if one_accumulator else (acc[0] + acc[1]).astype(np.float32))


def mul_mat(W, rows, K, x, chunk=1024):
    """y = W . Q8_0(x) as the reference computes it"""
    W = np.asarray(W, np.uint8)
    rb = K // 32 * BB
    assert W.size == rows * rb
    q8 = lg.quantize_row_q8_0(x)
    return np.concatenate([vec_dot_rows(W[r * rb:min(rows, r + chunk) * rb], q8) for r in range(0, rows, chunk)])


# ---- the genuine reference, where it is built (oracle/_ref/libggml_ref.so: `make -C oracle ref`) ---------------------------------------------------
def load_ref():
    """the reference library, or None where it is not built"""
    L = lg.load_ref()
    if L is None:
        return None
    L.ggml_vec_dot_iq4_nl_q8_0.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]
    L.dequantize_row_iq4_nl.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    return L


def reference_outputs(L, blocks, xs, deq_rows):
    """the live reference: dots f32 [vectors][rows] of ggml_vec_dot_iq4_nl_q8_0, sha256 of its Q8_0 bytes per vector, dequantised rows f32 [len(deq_rows)][K]"""
    K = xs[0].size
    rb = K // 32 * BB
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    blocks = np.ascontiguousarray(blocks, np.uint8)
    dots = np.zeros((len(xs), ROWS), np.float32)
    q8sha = []
    for i, x in enumerate(xs):
        q8 = np.zeros(K // 32 * 34, np.uint8)
        L.quantize_row_q8_0(p(np.ascontiguousarray(x, np.float32)), p(q8), K)
        q8sha.append(hashlib.sha256(q8.tobytes()).hexdigest())
        for r in range(ROWS):
            s = C.c_float(0)
            L.ggml_vec_dot_iq4_nl_q8_0(K, C.byref(s), 0, C.c_void_p(blocks.ctypes.data + r * rb), 0, p(q8), 0, 1)
            dots[i, r] = s.value
    deq = np.zeros((len(deq_rows), K), np.float32)
    for i, r in enumerate(deq_rows):
        L.dequantize_row_iq4_nl(C.c_void_p(blocks.ctypes.data + r * rb), p(deq[i]), K)
    return dots, q8sha, deq
