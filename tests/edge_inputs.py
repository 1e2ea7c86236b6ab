"""Seeded edge-input generators shared by the CPU edge tests (tests/test_oracle_edges.py), their fixture generator
(tests/golden/gen_edge_kats.py) and the GPU edge tests (tests/test_gpu_edges.py).

The kernels keep the reference's bits only because of bounds and branches that gentle random inputs never reach: the f16 exactness of
the matrix-core operands (|isum| < 2^24 for Q6_K, the S = 2 S_h + S_l split of the Q4_K min term), the first-max rule and the byte trick
of the Q8_K prologue, the overflow / underflow branches of v_expf.  Each generator returns its inputs together with one short tag per
super-block (weights) or 256-block (activations), so that a test can assert which edges it reached.

Finiteness rule: the generators keep every expected output finite, and every test asserts np.isfinite on the oracle's output.  A NaN
has no single right bit pattern here (the x86 default NaN is 0xFFC00000, the GPU's 0x7FC00000), and the contract does not cover NaN
payloads.  A `big_d` weight block therefore never meets a `huge` activation block (edge_matvec_inputs), so that no dot product overflows.
"""
import numpy as np

Q4_K, Q5_K, Q6_K = 12, 13, 14
BLOCK_BYTES = {Q4_K: 144, Q5_K: 176, Q6_K: 210}
WEIGHT_KINDS = ("random", "max", "split", "neg_d", "zero_d", "subnormal_d", "big_d")
ACT_KINDS = ("random", "constant", "near_constant", "zero", "single", "opposite_max", "tiny_max", "overflow_iscale", "huge", "ties")
# Q6_K scales around the sa / sl split of the matrix-core kernel (sa = sc & ~15, sl = sc & 15)
Q6_SPLIT_SCALES = np.array([-128, -113, -112, -1, 0, 15, 16, 112, 127], np.int8)
# 6-bit Q4_K / Q5_K scales and mins at the nibble boundaries and the ends of their range
K4_SPLIT_SCALES = np.array([0, 1, 15, 16, 31, 32, 47, 48, 62, 63], np.uint8)
# the largest |isum| of one 32-element integer product (bamd_prefill2.hip: the Q6_K matrix-core path is exact because |isum| < 2^24)
ISUM_BOUND = {Q4_K: 32 * 63 * 15 * 127, Q5_K: 32 * 63 * 31 * 127, Q6_K: 32 * 128 * 32 * 127}


def _f16_bytes(v):
    return np.asarray([v], np.float16).view(np.uint8)


def _sign(rng):
    return 1.0 if rng.random() < 0.5 else -1.0


def _cycle(kinds, n, rng):
    """n tags: every kind in turn, then shuffled (so that every kind appears once n >= len(kinds))"""
    tags = np.array([kinds[i % len(kinds)] for i in range(n)], dtype=object)
    rng.shuffle(tags)
    return tags


def pack_k4_scales(sc, mn):
    """the 12 scale bytes of a Q4_K / Q5_K super-block from eight 6-bit scales and mins (inverse of get_scale_min_k4)"""
    sc = np.asarray(sc, np.uint8); mn = np.asarray(mn, np.uint8)
    q = np.zeros(12, np.uint8)
    q[0:4] = (sc[0:4] & 63) | ((sc[4:8] >> 4) << 6)
    q[4:8] = (mn[0:4] & 63) | ((mn[4:8] >> 4) << 6)
    q[8:12] = (sc[4:8] & 15) | ((mn[4:8] & 15) << 4)
    return q


def unpack_k4_scales(q):
    """get_scale_min_k4 over the 12 scale bytes of each super-block: q [n][12] -> (sc, mn) int64 [n][8]"""
    q = np.asarray(q, np.uint8).reshape(-1, 12).astype(np.int64)
    sc = np.zeros((q.shape[0], 8), np.int64); mn = np.zeros_like(sc)
    sc[:, 0:4] = q[:, 0:4] & 63; mn[:, 0:4] = q[:, 4:8] & 63
    sc[:, 4:8] = (q[:, 8:12] & 15) | ((q[:, 0:4] >> 6) << 4)
    mn[:, 4:8] = (q[:, 8:12] >> 4) | ((q[:, 4:8] >> 6) << 4)
    return sc, mn


def pack_q6_quants(q):
    """the 192 ql | qh bytes of a Q6_K super-block from its 256 unsigned 6-bit quants (inverse of dequantize_row_q6_K's unpacking)"""
    q = np.asarray(q, np.int64).reshape(2, 4, 32)                 # [half][group of 32][l]
    ql = np.zeros((2, 64), np.int64); qh = np.zeros((2, 32), np.int64)
    ql[:, 0:32] = (q[:, 0] & 15) | ((q[:, 2] & 15) << 4)
    ql[:, 32:64] = (q[:, 1] & 15) | ((q[:, 3] & 15) << 4)
    qh[:, :] = (q[:, 0] >> 4) | ((q[:, 1] >> 4) << 2) | ((q[:, 2] >> 4) << 4) | ((q[:, 3] >> 4) << 6)
    return np.concatenate([ql.reshape(-1), qh.reshape(-1)]).astype(np.uint8)


def unpack_quants(t, blocks):
    """integer view of K-quant super-blocks in the reference's element order: (q [n][256] unsigned quants, sc [n][16] (Q6_K, signed) or
    [n][8], mn [n][8] or None)"""
    b = np.asarray(blocks, np.uint8).reshape(-1, BLOCK_BYTES[t])
    q = np.zeros((b.shape[0], 256), np.int64)
    if t == Q6_K:                                                 # dequantize_row_q6_K: two halves of 128 elements
        ql, qh = b[:, 0:128].astype(np.int64), b[:, 128:192].astype(np.int64)
        for h in range(2):
            L, H, o = ql[:, 64 * h:64 * h + 64], qh[:, 32 * h:32 * h + 32], 128 * h
            q[:, o + 0:o + 32] = (L[:, 0:32] & 15) | ((H & 3) << 4)
            q[:, o + 32:o + 64] = (L[:, 32:64] & 15) | (((H >> 2) & 3) << 4)
            q[:, o + 64:o + 96] = (L[:, 0:32] >> 4) | (((H >> 4) & 3) << 4)
            q[:, o + 96:o + 128] = (L[:, 32:64] >> 4) | (((H >> 6) & 3) << 4)
        return q, b[:, 192:208].copy().view(np.int8).astype(np.int64), None
    sc, mn = unpack_k4_scales(b[:, 4:16])
    qs = (b[:, 16:144] if t == Q4_K else b[:, 48:176]).astype(np.int64)
    for j in range(4):                                            # dequantize_row_q4_K / q5_K: 64 elements per step, low then high nibbles
        q[:, 64 * j:64 * j + 32] = qs[:, 32 * j:32 * j + 32] & 15
        q[:, 64 * j + 32:64 * j + 64] = qs[:, 32 * j:32 * j + 32] >> 4
        if t == Q5_K:
            qh = b[:, 16:48].astype(np.int64)
            q[:, 64 * j:64 * j + 32] += ((qh >> (2 * j)) & 1) << 4
            q[:, 64 * j + 32:64 * j + 64] += ((qh >> (2 * j + 1)) & 1) << 4
    return q, sc, mn


def edge_kquant_tensor(t, K, rows, rng, kinds=WEIGHT_KINDS, kind_of=None):
    """Raw blocks of an [rows, K] K-quant matrix, one kind per super-block (all of `kinds` in a shuffled cycle, or named by kind_of [rows][K/256]):
      random       random bytes, a positive normal-range d / dmin (booster_amd.gguf.random_kquant_tensor)
      max          the largest integer products: Q4_K / Q5_K scales and mins 63, quants 15 / 31; Q6_K scales -128 / 127, quants 0 / 63
      split        Q6_K scales around the sa / sl split (Q6_SPLIT_SCALES); Q4_K / Q5_K scales and mins from K4_SPLIT_SCALES
      neg_d        negative d (and dmin for Q4_K / Q5_K)
      zero_d       d = +0 or -0 (and, for half of the Q4_K / Q5_K blocks, dmin)
      subnormal_d  f16 subnormal d and dmin
      big_d        |d| (and dmin) in [2^10, 2^14]
    Returns (uint8 blocks [rows * K/256 * bytes], tags [rows][K/256])."""
    from booster_amd.gguf import random_kquant_tensor
    bb, nb = BLOCK_BYTES[t], K // 256
    blk = random_kquant_tensor(t, K, rows, rng).reshape(rows * nb, bb).copy()
    tags = _cycle(kinds, rows * nb, rng) if kind_of is None else np.asarray(kind_of, dtype=object).reshape(-1)
    dpos = 208 if t == Q6_K else 0
    for i in range(rows * nb):
        k, b = tags[i], blk[i]
        if k == "random":
            continue
        if k == "max":
            if t == Q6_K:                                         # every quant 0 (-> -32) or 63 (-> +31)
                b[0:192] = pack_q6_quants(np.where(rng.random(256) < 0.5, 0, 63))
                b[192:208] = np.where(rng.random(16) < 0.5, -128, 127).astype(np.int8).view(np.uint8)
            else:
                b[4:bb] = 255                                     # scales / mins 63, quants 15 / 31
        elif k == "split":
            if t == Q6_K:
                b[192:208] = rng.choice(Q6_SPLIT_SCALES, 16).view(np.uint8)
            else:
                b[4:16] = pack_k4_scales(rng.choice(K4_SPLIT_SCALES, 8), rng.choice(K4_SPLIT_SCALES, 8))
        elif k == "neg_d":
            b[dpos:dpos + 2] = _f16_bytes(-abs(float(b[dpos:dpos + 2].view(np.float16)[0])) * rng.uniform(0.5, 2.0))
            if t != Q6_K:
                b[2:4] = _f16_bytes(-abs(float(b[2:4].view(np.float16)[0])))
        elif k == "zero_d":
            b[dpos:dpos + 2] = _f16_bytes(-0.0 if rng.random() < 0.5 else 0.0)
            if t != Q6_K and rng.random() < 0.5:
                b[2:4] = _f16_bytes(-0.0 if rng.random() < 0.5 else 0.0)
        elif k == "subnormal_d":
            b[dpos:dpos + 2] = np.array([(0x8000 if rng.random() < 0.5 else 0) | int(rng.integers(1, 1024))], np.uint16).view(np.uint8)
            if t != Q6_K:
                b[2:4] = np.array([int(rng.integers(1, 1024))], np.uint16).view(np.uint8)
        elif k == "big_d":
            b[dpos:dpos + 2] = _f16_bytes(2.0 ** rng.uniform(10, 14) * _sign(rng))
            if t != Q6_K:
                b[2:4] = _f16_bytes(2.0 ** rng.uniform(10, 14))
        else:
            raise ValueError(k)
    return blk.reshape(-1), tags.reshape(rows, nb)


def _block(kind, rng, huge_max):
    """one 256-element activation block of the given kind (float32)"""
    x = (rng.standard_normal(256) * 3).astype(np.float32)
    if kind == "random":
        return x
    if kind == "constant":                                        # every quant -127 (iscale * max = -127): |S| = 4064, even, exact in f16
        return np.full(256, np.float32(_sign(rng) * 10.0 ** rng.uniform(-3, 3)), np.float32)
    if kind == "near_constant":                                   # one quant 127 - o per 32 elements, o odd: |S| = 4064 - o, odd and > 2048
        c = np.float32(_sign(rng) * 10.0 ** rng.uniform(-3, 3))
        x = np.full(256, c, np.float32)
        for g in range(8):
            o = 2 * int(rng.integers(0, 32)) + 1
            x[g * 32 + int(rng.integers(1, 32))] = c * np.float32((127 - o) / 127.0)
        return x
    if kind == "zero":
        x = np.zeros(256, np.float32)
        x[rng.random(256) < 0.5] = -0.0
        return x
    if kind == "single":
        x = np.zeros(256, np.float32)
        x[rng.random(256) < 0.3] = -0.0
        x[int(rng.integers(0, 256))] = np.float32(_sign(rng) * 10.0 ** rng.uniform(-5, 5))
        return x
    if kind == "opposite_max":                                    # |max| twice with opposite signs: the FIRST one sets the sign of d
        M = np.float32(np.abs(x).max() * 1.5)
        if rng.random() < 0.5:                                    # within one prologue lane (4 consecutive elements)
            lane, a = int(rng.integers(0, 64)), int(rng.integers(0, 3))
            i, j = 4 * lane + a, 4 * lane + int(rng.integers(a + 1, 4))
        else:                                                     # in two lanes, the later one possibly in a lower element slot
            i = int(rng.integers(0, 252))
            j = int(rng.integers((i // 4 + 1) * 4, 256))
        s = _sign(rng)
        x[i], x[j] = s * M, -s * M
        return x
    if kind == "tiny_max":
        return (x / np.abs(x).max() * np.float32(1e-30 * rng.uniform(0.5, 2))).astype(np.float32)
    if kind == "overflow_iscale":                                 # max below 127 / FLT_MAX: iscale = -127 / max is -+inf, d = 1 / iscale = -+0
        return (x / np.abs(x).max() * np.float32(10.0 ** rng.uniform(-37.9, -36.5))).astype(np.float32)
    if kind == "huge":
        return (x * np.float32(10.0 ** rng.uniform(15, np.log10(huge_max)))).astype(np.float32)
    if kind == "ties":                                            # max +-127 * 2^e: iscale = -+2^-e exactly, iscale * x = -+(k + 1/2)
        e = int(rng.integers(-12, 12))
        x = ((rng.integers(-127, 127, 256) + 0.5) * 2.0 ** e).astype(np.float32)
        x[int(rng.integers(0, 256))] = np.float32(_sign(rng) * 127 * 2.0 ** e)
        return x
    raise ValueError(kind)


def edge_activations(K, rng, kinds=ACT_KINDS, huge_max=1e30, kind_of=None):
    """f32 activations of length K, one kind per 256-block (all of `kinds` in a shuffled cycle, or named by kind_of [K/256]):
      random           standard normal x 3
      constant         one value, positive or negative: every quant -127
      near_constant    constant but for one element per 32 (quant 127 - odd): odd 32-element pair sums |S| > 2048
      zero             all zero, -0.0 included
      single           one non-zero element among +-0
      opposite_max     the largest |x| twice with opposite signs, in one lane or in two lanes: the first one wins
      tiny_max         block maximum about 1e-30
      overflow_iscale  block maximum below 127 / FLT_MAX: iscale overflows to -+inf (defined and deterministic under -DNDEBUG)
      huge             about 1e15 .. huge_max
      ties             values at exact .5 ties of iscale * x
    Returns (x float32 [K], tags [K/256])."""
    tags = _cycle(kinds, K // 256, rng) if kind_of is None else np.asarray(kind_of, dtype=object)
    return np.concatenate([_block(k, rng, huge_max) for k in tags]).astype(np.float32), tags


def edge_matvec_inputs(t, K, rows, rng, n_vec=1, wkinds=WEIGHT_KINDS, akinds=ACT_KINDS, huge_max=1e30):
    """an edge matrix and n_vec edge activation vectors (the activation kinds cycled over all n_vec vectors); `huge` activation blocks sit in
    the even super-block columns only and `big_d` weight blocks in the odd ones (K >= 512).
    Returns (W, wtags [rows][K/256], X [n_vec][K], xtags [n_vec][K/256])."""
    nb = K // 256
    xt = _cycle(akinds, n_vec * nb, rng).reshape(n_vec, nb)
    for i, j in zip(*np.nonzero(xt[:, 1::2] == "huge")):          # a huge block in odd column 2j + 1 changes places with column 2j
        xt[i, 2 * j], xt[i, 2 * j + 1] = xt[i, 2 * j + 1], xt[i, 2 * j]
    X = np.stack([edge_activations(K, rng, huge_max=huge_max, kind_of=xt[i])[0] for i in range(n_vec)])
    kind_of = _cycle(wkinds, rows * nb, rng).reshape(rows, nb)
    kind_of[:, 0::2] = np.where(kind_of[:, 0::2] == "big_d", "random", kind_of[:, 0::2])
    W, wt = edge_kquant_tensor(t, K, rows, rng, kind_of=kind_of)
    return W, wt, X, xt


# ---- helpers for coverage assertions ------------------------------------------------------------------------
def q8_fields(q8):
    """Q8_K bytes [n * 292] -> (d f32 [n], qs int8 [n][256], bsums int16 [n][16])"""
    b = np.asarray(q8, np.uint8).reshape(-1, 292)
    return b[:, 0:4].copy().view(np.float32).reshape(-1), b[:, 4:260].copy().view(np.int8), b[:, 260:292].copy().view(np.int16)


def pair_sums(q8):
    """the 32-element sums S of every sub-block pair (the Q4_K min-term operand, split S = 2 S_h + S_l): int64 [n][8]"""
    return q8_fields(q8)[1].astype(np.int64).reshape(-1, 8, 32).sum(axis=2)


def odd_pair_sums_above_2048(q8):
    S = pair_sums(q8)
    return int(np.count_nonzero((np.abs(S) > 2048) & (S % 2 != 0)))


def isum32(t, blocks, q8):
    """the exact int64 integer sums over every 32-element group of sc x q' x q8, q' the signed quant (Q4_K / Q5_K: q; Q6_K: q - 32),
    of each weight row against ONE Q8_K row: [rows][nb][8]"""
    q, sc, _ = unpack_quants(t, blocks)
    qs = q8_fields(q8)[1].astype(np.int64)
    nb = qs.shape[0]
    q = q.reshape(-1, nb, 256)
    if t == Q6_K:
        prod = np.repeat(sc.reshape(-1, nb, 16), 16, axis=2) * (q - 32) * qs[None]
    else:
        prod = np.repeat(sc.reshape(-1, nb, 8), 32, axis=2) * q * qs[None]
    return prod.reshape(q.shape[0], nb, 8, 32).sum(axis=3)


def first_max_sign(x):
    """per 256-block: the sign of the FIRST element of largest magnitude (quantize_row_q8_K), 0 for an all-zero block"""
    b = np.asarray(x, np.float32).reshape(-1, 256)
    return np.sign(b[np.arange(b.shape[0]), np.argmax(np.abs(b), axis=1)])


def f16_ties_of(n, rng, lo, hi):
    """n f32 values exactly halfway between two neighbouring normal f16 values, exponents lo .. hi - 1, random signs"""
    v = (1024 + rng.integers(0, 1023, n) + 0.5) * 2.0 ** (rng.integers(lo, hi, n) - 10)
    return (v * np.where(rng.random(n) < 0.5, -1.0, 1.0)).astype(np.float32)


def f16_edge_values(n, rng, lo=-14, hi=4):
    """f32 values that rounding to f16 (the KV store) meets at its edges, a quarter each: exact ties of round-to-nearest-even
    (exponents lo .. hi - 1), f16 subnormals, ties between f16 subnormals, -0.0"""
    kind = rng.integers(0, 4, n)
    sgn = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    sub = rng.integers(1, 1024, n) * 2.0 ** -24 * sgn
    subtie = (rng.integers(0, 1023, n) + 0.5) * 2.0 ** -24 * sgn
    v = np.select([kind == 0, kind == 1, kind == 2], [f16_ties_of(n, rng, lo, hi), sub, subtie], -0.0)
    return v.astype(np.float32)


def f16_ties(x):
    """how many elements of x lie exactly halfway between two neighbouring f16 values"""
    x = np.asarray(x, np.float32)
    r = x.astype(np.float16)
    xd, rd = x.astype(np.float64), r.astype(np.float64)
    up = np.nextafter(r, np.float16(np.inf)).astype(np.float64)
    dn = np.nextafter(r, np.float16(-np.inf)).astype(np.float64)
    return int(np.count_nonzero((xd != rd) & ((xd == (rd + up) / 2) | (xd == (rd + dn) / 2))))
