"""IQ4_XS: seeded inputs of the IQ4_XS tests and a numpy restatement of what the kernels compute — the x86 AVX2 branch of the reference's
ggml_vec_dot_iq4_xs_q8_K (ggml-quants.c:11855-11890) over quantize_row_q8_K activations, and dequantize_row_iq4_xs (:3568-3589).

The restatement is held to the genuine reference's outputs stored in tests/golden/iq4xs_kats.npz (tests/golden/gen_iq4xs_kats.py, tests/test_iq4xs_ref.py).

A block_iq4_xs is {f16 d, u16 scales_h, u8 scales_l[4], u8 qs[128]}, 136 bytes, 256 weights as eight 32-blocks ib:
    ls_ib = (scales_l[ib / 2] >> 4 * (ib % 2) & 0xf) | (scales_h >> 2 * ib & 3) << 4, used as ls_ib - 32 (-32 .. 31)
    qs[16 ib + j]: the low nibble is weight 32 ib + j, the high nibble weight 32 ib + 16 + j; a nibble indexes kvalues_iq4nl (:3548)
One dot product = eight SIMD lanes e, each ONE sequential f32 fma chain over the super-blocks, closed by hsum_float_8:
    acc_e = fma(f32(f16 x.d) * y.d, (float) sumi_e, acc_e)
with sumi_e the integer sum over the eight 32-blocks of (ls_ib - 32) x p_e[ib], p_e[ib] what mul_add_epi8 / madd_epi16 give for the four weights
32 ib + 4 e .. + 3 and the Q8_K bytes at the same positions (lanes e and e + 4 read the same qs bytes: low and high nibbles — Q4_0's geometry, not Q4_K's).

THE -128 RULE.  mul_add_epi8 (:10958-10962) is maddubs(sign(x, x), sign(y, x)): the activation byte y is negated where the table value x is negative, and
-(-128) wraps to -128 in int8.  So a NEGATIVE value w against an activation byte of -128 contributes w * 128, not w * (-128):
    p = sum(w * a) + 256 * sum(w over the bytes with a == -128 and w < 0)
WHERE IT ACTS.  Not on quantised activations: quantize_row_q8_K scales by iscale = -127 / max (:3613-3618; the line with -128 is commented out there), the
largest-magnitude element of a super-block becomes -127 and no byte is ever -128 (tests/test_iq4xs_ref.py asserts it for every stored vector), so on everything
an engine feeds it the product sum is the plain signed dot.  The rule is restated all the same and held to the reference on HAND-MADE Q8_K blocks that do hold
-128 (with_m128, pairs_q8: the reference's vec_dot takes any block_q8_K), so that the day a quantiser stores that byte the known answers say what to compute.
Nothing saturates (pair sums <= 2 * 127 * 128 < 32768; madd_epi16 widens), |sumi_e| <= 8 * 4 * 127 * 128 * 32 < 2^24: int -> f32 is exact.

dequantize_row_iq4_xs rounds TWICE: dl = d * (ls - 32) in f32, then y = dl * value.  An fma, or d * ((ls - 32) * value), gives other bits.
The fma is lowbit_ref.fma32 (exact, see there)."""
import ctypes as C
import hashlib

import numpy as np

import edge_inputs as ei
import lowbit_ref as lr
from lowbit_ref import fma32

IQ4_XS = 23
BB = 136
KVALUES = np.array([-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113], np.int32)
KS = [256, 768, 4096, 14336]
SCALES = lr.SCALES                             # (1e-3, 1.0, 50.0)
ROWS = lr.ROWS                                 # 32
DEQ_ROWS = lr.DEQ_ROWS                         # rows of a random case whose dequantisation is stored
EDGE_K = 1024
EDGE_WKINDS = ("random", "ls_0", "ls_31", "ls_32", "ls_63", "qs_00", "qs_ff", "d_min_subnormal", "d_max", "neg_d", "zero_d")
EDGE_AKINDS = ("all_bytes", "zero", "random", "constant", "single", "opposite_max", "ties")
EDGE_NVEC = 7
PAIRS_NVEC = 3
SUMI_BOUND = 8 * 4 * 127 * 128 * 32
SEED = 4243                                    # chosen so that at K = 4096 the three wrong variants of test_iq4xs_ref.py differ from the reference (gen_iq4xs_kats.py checks)
REF = lr.REF
_digest = lr._digest


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def rand_case(K):
    """32 rows of random raw blocks (every nibble pattern, every scale bit pattern; finite positive f16 d), three activation magnitudes"""
    from booster_amd.gguf import random_iq4_xs_tensor
    rng = np.random.default_rng(SEED * IQ4_XS + K)
    blocks = random_iq4_xs_tensor(K, ROWS, rng)
    xs = [(rng.standard_normal(K) * s).astype(np.float32) for s in SCALES]
    return blocks, xs, _digest(blocks, xs)


def pack_scales(blk, ls):
    """write the eight 6-bit scales ls [8] into bytes 2..7 of one raw block (scales_h, scales_l)"""
    ls = np.asarray(ls, np.int64)
    sh = 0
    for ib in range(8):
        sh |= int(ls[ib] >> 4) << (2 * ib)
    blk[2] = sh & 0xff; blk[3] = sh >> 8
    for k in range(4):
        blk[4 + k] = int(ls[2 * k] & 15) | (int(ls[2 * k + 1] & 15) << 4)


def all_bytes_block(rng):
    """256 integer-valued floats: every value -127 .. 127 once and one of them twice, shuffled.  The largest magnitude is 127, so iscale = -127 / +-127 = -+1
    exactly and every element quantises to itself or to its negative: the Q8_K bytes are every value a quantised block can hold, -127 .. 127"""
    v = np.concatenate([np.arange(-127, 128), [int(rng.integers(-126, 127))]])
    return rng.permutation(v).astype(np.float32)


def with_m128(q8):
    """Q8_K bytes with every quant of -127 (the largest-magnitude element of each non-zero super-block is one) replaced by -128, bsums to match: what
    iscale = -128 / max would have stored.  No quantiser here writes this; the reference's vec_dot takes it"""
    b = np.array(q8, np.uint8).reshape(-1, 292).copy()
    qs = b[:, 4:260].view(np.int8)
    qs[qs == -127] = -128
    b[:, 260:292] = qs.astype(np.int16).reshape(-1, 16, 16).sum(axis=2).astype(np.int16).view(np.uint8).reshape(-1, 32)
    return b.reshape(-1)


def pairs_q8(rng):
    """three hand-made Q8_K super-blocks (d = 1) that hold every byte -128 .. 127 once: increasing, decreasing, shuffled"""
    inc = np.arange(-128, 128)
    out = []
    for q in (inc, inc[::-1], rng.permutation(inc)):
        b = np.zeros(292, np.uint8)
        b[0:4] = np.array([1.0], np.float32).view(np.uint8)
        b[4:260] = q.astype(np.int8).view(np.uint8)
        b[260:292] = q.reshape(16, 16).sum(axis=1).astype(np.int16).view(np.uint8)
        out.append(b)
    return out


def edge_blocks(K, rows, rng):
    """raw blocks with one edge kind per super-block (all kinds in a shuffled cycle): every scale of the block 0, 31, 32 or 63 (-32, -1, 0, 31 after the - 32);
    qs all 0x00 (every value -127) / all 0xFF (every value 113); d the smallest f16 subnormal, the largest finite f16, negative, +-0.
    Returns (bytes, tags [rows][K/256])."""
    from booster_amd.gguf import random_iq4_xs_tensor
    nb = K // 256
    blk = random_iq4_xs_tensor(K, rows, rng).reshape(rows * nb, BB).copy()
    tags = ei._cycle(EDGE_WKINDS, rows * nb, rng)
    for r in range(4):                                            # the four scale kinds in EVERY block position of the row: rows 0-3, rotated
        for c in range(nb):
            tags[r * nb + c] = ("ls_0", "ls_31", "ls_32", "ls_63")[(r + c) % 4]
    for b, k in enumerate(tags):
        d = float(blk[b, 0:2].copy().view(np.float16)[0])
        if k in ("ls_0", "ls_31", "ls_32", "ls_63"):
            pack_scales(blk[b], [int(k[3:])] * 8)
        elif k == "qs_00":
            blk[b, 8:] = 0x00
        elif k == "qs_ff":
            blk[b, 8:] = 0xff
        elif k == "d_min_subnormal":
            blk[b, 0:2] = np.array([0x01, 0x80 if rng.random() < 0.5 else 0x00], np.uint8)
        elif k == "d_max":
            blk[b, 0:2] = np.array([0xff, 0x7b | (0x80 if rng.random() < 0.5 else 0x00)], np.uint8)
        elif k == "neg_d":
            blk[b, 0:2] = lr._f16(-d)
        elif k == "zero_d":
            blk[b, 0:2] = lr._f16(-0.0 if rng.random() < 0.5 else 0.0)
        elif k != "random":
            raise ValueError(k)
    return blk.reshape(-1), tags.reshape(rows, nb)


def edge_case():
    """edge weight blocks x edge activation blocks at K = 1024: every weight kind in every block position somewhere, every activation kind"""
    rng = np.random.default_rng(160001 + IQ4_XS)
    blocks, wtags = edge_blocks(EDGE_K, ROWS, rng)
    nb = EDGE_K // 256
    xt = ei._cycle(EDGE_AKINDS, EDGE_NVEC * nb, rng).reshape(EDGE_NVEC, nb)
    xs = [np.concatenate([all_bytes_block(rng) if k == "all_bytes" else ei._block(k, rng, 1e30) for k in xt[i]]).astype(np.float32) for i in range(EDGE_NVEC)]
    return blocks, xs, _digest(blocks, xs), wtags, xt


def pairs_case():
    """every (nibble, activation byte) pair: K = 256, weight n of row r has nibble (n + r) % 16 (rows 0-15 reach all sixteen at every position; rows 16-31 again
    under other scales), against three activation blocks that quantise to every byte -127 .. 127 (all_bytes_block) and, as the fourth return value, three
    hand-made Q8_K blocks that hold every byte -128 .. 127 once (pairs_q8)"""
    from booster_amd.gguf import random_iq4_xs_tensor
    rng = np.random.default_rng(160002 + IQ4_XS)
    blk = random_iq4_xs_tensor(256, ROWS, rng).reshape(ROWS, BB).copy()
    n = np.arange(256)
    for r in range(ROWS):
        nib = (n + r) % 16
        w = nib.reshape(8, 2, 16)                                 # [ib][low | high][j]
        blk[r, 8:] = (w[:, 0, :] | (w[:, 1, :] << 4)).reshape(128)
    xs = [all_bytes_block(rng) for _ in range(PAIRS_NVEC)]
    q8s = pairs_q8(rng)
    blocks = blk.reshape(-1)
    return blocks, xs, _digest(blocks, xs + [q.view(np.float32) for q in q8s]), q8s


def all_cases():
    """(key, blocks, activation vectors, inputs digest, rows whose dequantisation is stored) of every stored case"""
    for K in KS:
        blocks, xs, digest = rand_case(K)
        yield "iq4_xs_K%d" % K, blocks, xs, digest, DEQ_ROWS
    blocks, xs, digest, _, _ = edge_case()
    yield "iq4_xs_edge", blocks, xs, digest, tuple(range(ROWS))
    blocks, xs, digest, _ = pairs_case()
    yield "iq4_xs_pairs", blocks, xs, digest, tuple(range(ROWS))


M128_KEYS = ("iq4_xs_K4096", "iq4_xs_edge", "iq4_xs_pairs")


def m128_q8(key, q8s):
    """the hand-made Q8_K vectors of a case in M128_KEYS (stored as <key>_dots_m128): the case's own quantised vectors q8s through with_m128; the pairs case:
    its pairs_q8 blocks"""
    if key == "iq4_xs_pairs":
        return pairs_case()[3]
    return [with_m128(q) for q in q8s]


# ---- weights --------------------------------------------------------------------------------------------------------------------------------
def unpack(raw):
    """raw blocks -> (d f32 [n], ls - 32 int32 [n][8], nibbles int32 [n][256], table values int32 [n][256]), weights in element order"""
    b = np.asarray(raw, np.uint8).reshape(-1, BB)
    n = b.shape[0]
    d = np.ascontiguousarray(b[:, 0:2]).view(np.float16).reshape(-1).astype(np.float32)
    sh = np.ascontiguousarray(b[:, 2:4]).view(np.uint16).reshape(-1).astype(np.int32)
    sl = b[:, 4:8].astype(np.int32)
    ib = np.arange(8)
    ls = ((sl[:, ib // 2] >> (4 * (ib % 2))) & 15) | (((sh[:, None] >> (2 * ib)) & 3) << 4)
    qs = b[:, 8:].astype(np.int32).reshape(n, 8, 16)
    nib = np.concatenate([qs & 15, qs >> 4], axis=2).reshape(n, 256)            # 32-block ib: elements 0-15 low nibbles, 16-31 high nibbles
    return d, ls - 32, nib, KVALUES[nib]


def dequantize(raw, fused=False):
    """dequantize_row_iq4_xs: dl = d * (float) (ls - 32), rounded to f32; y = dl * (float) value.  fused: d * ((ls - 32) * value) with ONE rounding — NOT what the
    reference computes; tests/test_iq4xs_ref.py shows that the stored rows tell the two apart"""
    d, ls, _, q = unpack(raw)
    with np.errstate(all="ignore"):
        if fused:
            return (d.astype(np.float64)[:, None] * (np.repeat(ls, 32, axis=1) * q).astype(np.float64)).astype(np.float32).reshape(-1)
        dl = (d[:, None] * ls.astype(np.float32)).astype(np.float32)
        return (np.repeat(dl, 32, axis=1) * q.astype(np.float32)).astype(np.float32).reshape(-1)


# ---- the chain ------------------------------------------------------------------------------------------------------------------------------
def lane_sums(raw, q8, rule=True, q4k_lanes=False):
    """exact integer lane sums [rows][nb][8].  rule = False: the plain signed dot, without the -128 rule.  q4k_lanes = True: the Q4_K lane mapping (lane e of
    32-block pair j reads qs[32 j + 4 e ..], low nibbles for block 2 j and high ones for 2 j + 1).  Neither is what the reference computes"""
    yd, qa, _ = ei.q8_fields(q8)
    nb = yd.size
    _, ls, nib, w = unpack(raw)
    rows = w.shape[0] // nb
    if q4k_lanes:
        qs = np.asarray(raw, np.uint8).reshape(-1, BB)[:, 8:].astype(np.int32).reshape(-1, 4, 32)
        w = KVALUES[np.stack([qs & 15, qs >> 4], axis=2).reshape(-1, 256)]          # element 64 j + 32 h + l = nibble h of qs[32 j + l]
    w = w.reshape(rows, nb, 256).astype(np.int32)                                 # (int32 throughout: every partial sum stays below SUMI_BOUND < 2^24)
    a = qa.astype(np.int32)[None]
    pr = w * a
    if rule and (a == -128).any():
        pr = pr + 256 * w * ((a == -128) & (w < 0))
    p = pr.reshape(rows, nb, 8, 8, 4).sum(axis=4, dtype=np.int32)                 # [ib][e]: element 32 ib + 4 e + u
    return (p * ls.reshape(rows, nb, 8, 1)).sum(axis=2, dtype=np.int32).astype(np.int64)


def vec_dot_rows(raw, q8, rule=True, q4k_lanes=False):
    """the reference's dot product of every row with the Q8_K vector: float32 [rows]"""
    yd, _, _ = ei.q8_fields(q8)
    nb = yd.size
    d, _, _, _ = unpack(raw)
    rows = d.size // nb
    sumi = lane_sums(raw, q8, rule, q4k_lanes)
    assert np.abs(sumi).max(initial=0) <= SUMI_BOUND
    xd = d.reshape(rows, nb)
    acc = np.zeros((rows, 8), np.float32)
    with np.errstate(all="ignore"):
        for i in range(nb):
            s = (xd[:, i] * yd[i]).astype(np.float32)
            acc = fma32(s[:, None], sumi[:, i].astype(np.float32), acc)
        r = acc[:, 0:4] + acc[:, 4:8]                                             # hsum_float_8 (ggml-quants.c:47-53)
        r = r[:, 0:2] + r[:, 2:4]
        return (r[:, 0] + r[:, 1]).astype(np.float32)


def mul_mat(po, W, rows, K, x, chunk=512):
    """y = W . Q8_K(x) as the reference computes it; Q8_K from the oracle's quantize_row_q8_K (held to the reference by tests/test_oracle_vs_ref.py)"""
    W = np.asarray(W, np.uint8)
    rb = (K // 256) * BB
    assert W.size == rows * rb
    q8 = po.quantize_q8_K(np.ascontiguousarray(x, np.float32))
    return np.concatenate([vec_dot_rows(W[r * rb:min(rows, r + chunk) * rb], q8) for r in range(0, rows, chunk)])


# ---- the genuine reference, where it is built (oracle/_ref/libggml_ref.so: `make -C oracle ref`) ---------------------------------------------------
def load_ref():
    """the reference library, or None where it is not built"""
    L = lr.load_ref()
    if L is None:
        return None
    L.ggml_vec_dot_iq4_xs_q8_K.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]
    L.dequantize_row_iq4_xs.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    return L


def reference_dots(L, blocks, K, q8):
    """ggml_vec_dot_iq4_xs_q8_K of every row with the Q8_K bytes q8: f32 [ROWS]"""
    rb = K // 256 * BB
    blocks = np.ascontiguousarray(blocks, np.uint8); q8 = np.ascontiguousarray(q8, np.uint8)
    out = np.zeros(ROWS, np.float32)
    for r in range(ROWS):
        s = C.c_float(0)
        L.ggml_vec_dot_iq4_xs_q8_K(K, C.byref(s), 0, C.c_void_p(blocks.ctypes.data + r * rb), 0, q8.ctypes.data_as(C.c_void_p), 0, 1)
        out[r] = s.value
    return out


def reference_outputs(L, blocks, xs, deq_rows, q8_out=None):
    """the live reference: dots f32 [vectors][rows] of ggml_vec_dot_iq4_xs_q8_K, sha256 of its Q8_K bytes per vector, dequantised rows f32 [len(deq_rows)][K];
    q8_out: a list that receives the reference's Q8_K bytes of every vector"""
    K = xs[0].size
    rb = K // 256 * BB
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    blocks = np.ascontiguousarray(blocks, np.uint8)
    dots = np.zeros((len(xs), ROWS), np.float32)
    q8sha = []
    for i, x in enumerate(xs):
        q8 = np.zeros(K // 256 * 292, np.uint8)
        L.quantize_row_q8_K(p(np.ascontiguousarray(x, np.float32)), p(q8), K)
        q8sha.append(hashlib.sha256(q8.tobytes()).hexdigest())
        if q8_out is not None:
            q8_out.append(q8)
        dots[i] = reference_dots(L, blocks, K, q8)
    deq = np.zeros((len(deq_rows), K), np.float32)
    for i, r in enumerate(deq_rows):
        L.dequantize_row_iq4_xs(C.c_void_p(blocks.ctypes.data + r * rb), p(deq[i]), K)
    return dots, q8sha, deq
