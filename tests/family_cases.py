"""The eleven weight types added after Q4_K / Q5_K / Q6_K in one table, and the deterministic case lists of tests/test_gpu_sweep_families.py.
A plain helper module (as bitcheck.py): no fixtures.  tests/test_sweep_cases.py holds the lists to the classes they must contain, without a GPU.

Every list comes from np.random.default_rng(<fixed seed>) alone, so it is the same on every machine and every case is a pytest id.  K is drawn as
nb = K / 256.  The named nb values are grouped in CLASSES, one class per branch of the kernels (b32_stream_depth and the batch kernel's ring in
bamd_matvec_b32.h / bamd_prefill_b32.h, flt_unit's chunk pairs in bamd_matvec_flt.hip, q0_can_split / q0_split_nbuf); a list takes one draw from every class
of its type and as many uniform draws as there are common classes, so no class depends on the luck of the seed and about half of a list is uniform."""
import collections

import numpy as np

import float_ref as fr
import iq4nl_ref as nl
import legacy1_ref as l1
import legacy_ref as lg
import lowbit_ref as lr
from booster_amd.gguf import (random_float_tensor, random_iq4_nl_tensor, random_kquant_tensor, random_q0_tensor, random_q1_tensor)

F32, F16, Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q2_K, Q3_K, Q6_K, IQ4_NL, BF16 = 0, 1, 2, 3, 6, 7, 8, 10, 11, 14, 20, 30

Family = collections.namedtuple("Family", "name gen ref act modes switch")
#   gen(t, K, rows, rng, amp) -> raw bytes; ref(po, t, W, rows, K, x) -> f32 [rows], the restatement the CPU tests hold to the genuine reference's outputs;
#   act: the activation form; modes: the mat-vec launch modes the type has (2 = split-K); switch: the type's name in mfma_harness.prefill_switches (None: no
#   matrix-core prompt kernel)
_kq = (lambda t, K, rows, rng, amp=1.0: random_kquant_tensor(t, K, rows, rng, amp), lambda po, t, W, rows, K, x: lr.mul_mat(po, t, W, rows, K, x))
_q0 = (lambda t, K, rows, rng, amp=1.0: random_q0_tensor(t, K, rows, rng, amp), lambda po, t, W, rows, K, x: lg.mul_mat(t, W, rows, K, x))
_q1 = (lambda t, K, rows, rng, amp=1.0: random_q1_tensor(t, K, rows, rng, amp), lambda po, t, W, rows, K, x: l1.mul_mat(t, W, rows, K, x))
_nl = (lambda t, K, rows, rng, amp=1.0: random_iq4_nl_tensor(K, rows, rng, amp), lambda po, t, W, rows, K, x: nl.mul_mat(W, rows, K, x))
_fl = (lambda t, K, rows, rng, amp=4.0: random_float_tensor(t, K, rows, rng, amp), lambda po, t, W, rows, K, x: fr.mul_mat(t, W, rows, K, x))
FAMILIES = {
    Q2_K:   Family("Q2_K", *_kq, "q8_K", (0, 1, 2), "lowbit"),
    Q3_K:   Family("Q3_K", *_kq, "q8_K", (0, 1, 2), "lowbit"),
    Q8_0:   Family("Q8_0", *_q0, "q8_0", (0, 1, 2), "q0"),
    Q4_0:   Family("Q4_0", *_q0, "q8_0", (0, 1, 2), "q0"),
    Q5_0:   Family("Q5_0", *_q0, "q8_0", (0, 1, 2), "q0"),
    Q4_1:   Family("Q4_1", *_q1, "q8_1", (0, 1), "q1"),
    Q5_1:   Family("Q5_1", *_q1, "q8_1", (0, 1), "q1"),
    IQ4_NL: Family("IQ4_NL", *_nl, "q8_0", (0, 1), "nl"),
    F16:    Family("F16", *_fl, "f32", (0,), "flt"),          # (the float launcher reads no mode: one kernel)
    BF16:   Family("BF16", *_fl, "bf16", (0,), None),
    F32:    Family("F32", *_fl, "f32", (0,), "flt"),
}
TYPES = list(FAMILIES)
SPLIT_TYPES = (Q8_0, Q4_0, Q5_0)                 # whose split-K kernel is q0_split (bamd_matvec_b32.h); Q2_K / Q3_K split in the K-quant kernels, whose edges are others
FLOAT_TYPES = (F16, BF16, F32)
# a Q6_K segment beside Q2_K / Q3_K ones in the fused launches: the oracle is its expectation, as in tests/test_gpu_segments.py
_ORACLE = Family("Q6_K", _kq[0], lambda po, t, W, rows, K, x: po.mul_mat_q(t, W, rows, K, np.ascontiguousarray(x, np.float32), nthreads=8)[0], "q8_K", (0, 1, 2), None)


def family(t):
    return _ORACLE if t == Q6_K else FAMILIES[t]


def blob_bytes(nb):
    """BAMD_BLOB_BYTES(nb) = BAMD_ACT_RED_OFF(nb), bamd_device.h: the bytes of one token's quantised activations"""
    return (nb * (256 + 32 + 4) + 15) & ~15


# launch_matmul_batch_b32 (bamd_prefill_b32.h) and bamd_launch_matmul_batch (bamd_prefill.hip): tt = BAMD_TT * BAMD_BLOB_BYTES(nb) <= 160 KiB ? BAMD_TT : 4
BAMD_TT = 8
TILE8_NB = max(nb for nb in range(1, 200) if BAMD_TT * blob_bytes(nb) <= 160 * 1024)        # the last nb with token tiles of 8; TILE8_NB + 1 takes tiles of 4


def q0_can_split(nb):
    """q0_can_split, bamd_matvec_b32.h"""
    return 8 <= nb <= 56


def q0_split_nbuf(nb):
    """q0_split_nbuf, bamd_matvec_b32.h: two term buffers where mv_terms_off(nb) + 2 * nb * q0_term_floats * 4 fits BAMD_LDS_CU_BYTES, else one; mv_terms_off =
    BAMD_ACT_RED_OFF + 16 doubles (bamd_mv_select.h), q0_term_floats = 576 (bamd_b32_device.h)"""
    return 2 if blob_bytes(nb) + 16 * 8 + 2 * nb * 576 * 4 <= 160 * 1024 else 1


# the last nb with two term buffers and the first with one, inside q0_can_split (tests/test_sweep_cases.py holds the pair to its own restatement of the header lines)
SPLIT_NBUF_EDGE = (max(nb for nb in range(1, 100) if q0_can_split(nb) and q0_split_nbuf(nb) == 2), min(nb for nb in range(1, 100) if q0_can_split(nb) and q0_split_nbuf(nb) == 1))

COMMON = collections.OrderedDict([
    ("nb1", (1,)),                               # one record: D = 1, one chunk
    ("odd", (3, 11, 43)),                        # D = 1, more than one chunk; F16 / BF16: an odd chunk count above 1 (flt_unit's m1 false in the last round)
    ("2mod4", (6, 14, 22)),                      # D = 2 with more than one chunk: the in-row refill of the depth-2 ring; the batch kernel's (nb & 1) == 0 branch (but see batch_classes)
    ("0mod4", (4, 16, 32)),                      # D = 4
])
SPLIT_EDGES = (7, 8, 9, 15) + SPLIT_NBUF_EDGE + (56, 57)      # 7 / 57: a mode-2 request falls to mode A; 8: one record per wave; 9, 15: shares of 1 and 2
ROW_EDGES = (1, 7, 8, 9, 13, 16, 17, 63, 64, 65, 72, 520, 2047, 4100)
BATCH_T = (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 65, 100)


def classes(t):
    """name -> nb values, the mat-vec K classes of a type"""
    c = collections.OrderedDict(COMMON)
    if t in SPLIT_TYPES:
        for nb in SPLIT_EDGES:
            c["split%d" % nb] = (nb,)
    return c


def batch_classes(t):
    """the batch kernel of the 32-weight block types takes ring depth 2 where nb is even, but at token tiles of 8 not in the kernel that has IQ4_NL and not in the
    gate/up instance of Q4_1 / Q5_1 (bamd_prefill_b32.h): the class tile4even, an even nb on the tiles-of-4 side, is where valu_segment<B32Row<..>, 2, .., 4> runs for
    every type, and the only place where an IQ4_NL launch takes depth 2"""
    c = collections.OrderedDict((k, v) for k, v in COMMON.items() if k != "nb1")
    if t not in FLOAT_TYPES:                     # the float batch kernel keeps no blobs in LDS: no such switch
        c["tile8"] = (TILE8_NB,)
        c["tile4"] = (TILE8_NB + 1,)             # odd: ring depth 1
        c["tile4even"] = (TILE8_NB + 2,)
    else:
        c["nb1"] = COMMON["nb1"]
    return c


def class_of(t, nb):
    """the names of the classes of `t` that hold nb's branch (a uniform draw counts for its branch too)"""
    out = set()
    if nb == 1:
        out.add("nb1")
    elif nb & 1:
        out.add("odd")
    elif nb & 3:
        out.add("2mod4")
    else:
        out.add("0mod4")
    if t in SPLIT_TYPES and nb in SPLIT_EDGES:
        out.add("split%d" % nb)
    return out


def _cost_cap(t):
    """rows x nb a case may have so that its restatement stays well under a second on the CPU (Q2_K / Q3_K: about four times slower per weight)"""
    return 12000 if t in (Q2_K, Q3_K) else 48000


def _rows(rng, t, nb, edges=ROW_EDGES, top=3000):
    cap = max(8, _cost_cap(t) // nb)
    fit = [r for r in edges if r <= cap]
    return int(rng.choice(fit)) if rng.integers(0, 2) else int(rng.integers(1, min(top, cap) + 1))


MatVecCase = collections.namedtuple("MatVecCase", "i t K rows norm resid")


def matvec_cases(t, seed=20261020):
    """one draw from every class of the type, then four uniform ones (nb 1 .. 64)"""
    rng = np.random.default_rng([seed, t])
    nbs = [int(rng.choice(v)) for v in classes(t).values()] + [int(rng.integers(1, 65)) for _ in COMMON]
    flags = np.concatenate([rng.permutation(4) for _ in range((len(nbs) + 3) // 4)])      # RMSNorm x residual: every combination, in a seeded order
    out = []
    for i, nb in enumerate(nbs):
        out.append(MatVecCase(i, t, nb * 256, _rows(rng, t, nb), bool(flags[i] & 1), bool(flags[i] & 2)))
    return out


PairCase = collections.namedtuple("PairCase", "i t K rows")


def pair_cases(t, seed, edges):
    """three (K, rows) for the gate/up and arg-max launches: the depth-2 refill class, the odd class and one of the others; rows from `edges`, all ragged"""
    rng = np.random.default_rng([seed, t])
    c = classes(t)
    nbs = [int(rng.choice(c["2mod4"])), int(rng.choice(c["odd"])), int(rng.choice(c["0mod4"] + c["nb1"] + (SPLIT_NBUF_EDGE if t in SPLIT_TYPES else ())))]
    out = []
    for i, nb in enumerate(nbs):
        cap = _cost_cap(t) // 2 // nb
        out.append(PairCase(i, t, nb * 256, int(rng.choice([r for r in edges if r <= cap]))))
    return out


GATEUP_ROWS = (13, 63, 65, 513, 2047, 4100)     # none a multiple of 8
ARGMAX_ROWS = (63, 65, 513, 2047, 4100)         # at least eight row-groups: the tie sits in two workgroups


def gateup_cases(t):
    return pair_cases(t, 20261021, GATEUP_ROWS)


def argmax_cases(t):
    return pair_cases(t, 20261022, ARGMAX_ROWS)


# ---- fused launches over two and three segments of one activation form --------------------------------------------------------------------------
MIXES = [
    ("q8_0", (Q8_0, Q4_0, Q5_0)), ("q8_0", (IQ4_NL, Q8_0)), ("q8_0", (Q4_0, IQ4_NL)), ("q8_0", (Q5_0, IQ4_NL, Q8_0)),
    ("q8_1", (Q4_1, Q5_1)), ("q8_1", (Q5_1, Q4_1, Q5_1)),
    ("f32", (F16, F32)), ("f32", (F32, F16, F32)),
    ("q8_K", (Q2_K, Q3_K, Q6_K)), ("q8_K", (Q6_K, Q2_K)), ("q8_K", (Q3_K, Q6_K)),
    ("bf16", (BF16, BF16, BF16)),                # one type only in this form: the slot arithmetic of the kernel's BF16 instance
]
GRID = 256                                       # workgroups of a mat-vec launch on the MI355X (units of two row-groups for the float kernels)
SegCase = collections.namedtuple("SegCase", "i form types K rows modes")


def mix_modes(types):
    """the launch modes every segment of the mix has (a launch with an IQ4_NL segment has no split-K)"""
    m = set(family(types[0]).modes)
    for t in types[1:]:
        m &= set(family(t).modes)
    return tuple(sorted(m))


def segment_cases(seed=20261023):
    """three cases per mix, then two split-K ones (below).  Pattern 0: every non-last segment has an odd row-group count; pattern 1: every non-last segment is ragged as well; pattern 2: a
    segment of fewer row-groups than the grid beside one of more.  K from the classes; the pure Q8_0 / Q4_0 / Q5_0 mix takes one K inside q0_can_split (pattern
    0) and one outside (pattern 1)."""
    rng = np.random.default_rng(seed)
    out = []
    for form, types in MIXES:
        slow = any(t in (Q2_K, Q3_K) for t in types)
        for pattern in range(3):
            n = len(types)
            rows = []
            for s in range(n):
                last = s == n - 1
                if pattern == 2:
                    nrg = int(rng.integers(2, 30)) if s % 2 == 0 else int(rng.integers(GRID * (2 if form in ("f32", "bf16") else 1) + 1, 2 * GRID + 90))
                else:
                    nrg = int(rng.integers(1, 80)) if last else 2 * int(rng.integers(0, 40)) + 1
                ragged = (pattern == 1 and not last) or bool(rng.integers(0, 2))
                rows.append(8 * nrg - (int(rng.integers(1, 8)) if ragged else 0))
            pure_q0 = all(t in SPLIT_TYPES for t in types)
            if pure_q0 and pattern == 0:
                nb = int(rng.choice([9, 14, 22]))            # inside q0_can_split, with the uneven shares
            elif pure_q0 and pattern == 1:
                nb = int(rng.choice([3, 6, 7]))              # outside: mode 2 falls to mode A
            else:
                fit = [v for vs in COMMON.values() for v in vs if v * sum(rows) <= (12000 if slow else 48000)]
                nb = int(rng.choice(fit))
            out.append(SegCase(len(out), form, types, nb * 256, tuple(rows), mix_modes(types)))
    # split-K over differently typed segments with more row-groups than workgroups: matvec_q0_split_kernel deals row-groups g, g + 256, g + 512 to workgroup g, so
    # its `ctr` (the term buffer's parity and the chain wave) carries from a segment of one record size into the next.  Two term buffers with three walks (nb 8 .. 11),
    # then the one-buffer path (the first nb beyond SPLIT_NBUF_EDGE)
    rng = np.random.default_rng([seed, 1])
    for nb, lo, hi in ((int(rng.integers(8, 12)), 150, 250), (SPLIT_NBUF_EDGE[1], 90, 125)):
        rows = [8 * (2 * int(rng.integers(lo // 2, hi // 2)) + 1), 8 * int(rng.integers(lo, hi)) - int(rng.integers(1, 8)), 8 * int(rng.integers(lo, hi))]
        out.append(SegCase(len(out), "q8_0", (Q8_0, Q4_0, Q5_0), nb * 256, tuple(rows), (0, 1, 2)))
    return out


def slot_segments(rows, grid=GRID):
    """for every workgroup slot of a split-K launch over segments of `rows`, the segments its row-groups g, g + grid, ... lie in, in walk order"""
    ends = np.cumsum([(r + 7) // 8 for r in rows])
    g = min(grid, int(ends[-1]))
    return [[int(np.searchsorted(ends, rg, side="right")) for rg in range(slot, int(ends[-1]), g)] for slot in range(g)]


# ---- more row-groups than the grid has waves ---------------------------------------------------------------------------------------------------------
WAVE_SLOTS = GRID * 8                            # mode A: 256 workgroups of 8 waves, a row-group (float kernels: a unit of two) per wave and walk
TallCase = collections.namedtuple("TallCase", "t K nrg rows epi")


def tall_cases(t):
    """(K, row-groups, epilogue) with more row-groups than wave slots: 2049 gives one wave a second walk, 4099 gives every wave a second and three waves a third;
    the float kernels take two row-groups per walk, so their counts are doubled.  The last row-group is ragged (rows = 8 x nrg - 3).  K = 1536, 256, 1024: ring
    depth 2 with three chunks, depth 1, depth 4.  Q2_K / Q3_K (a slow restatement): K = 256 and 2049 row-groups only"""
    f = 2 if t in FLOAT_TYPES else 1
    if t in (Q2_K, Q3_K):
        shapes = [(256, 2049, "add"), (256, 2049, "gateup"), (256, 2049, "argmax")]
    else:
        shapes = [(1536, 2049 * f, "add"), (256, 4099 * f, "gateup"), (1024, 2049 * f, "argmax")]
        if f == 1:                                   # the gate -> up -> next gate hand-over of a second walk with a ring of more than one slot
            shapes.append((1536, 2049, "gateup"))
    return [TallCase(t, K, nrg, 8 * nrg - 3, epi) for K, nrg, epi in shapes]


# ---- prompt evaluation ---------------------------------------------------------------------------------------------------------------------------
BatchCase = collections.namedtuple("BatchCase", "i t K rows T norm resid")
BATCH_ROWS = (7, 8, 13, 16, 17, 63, 64, 65, 72, 520)


def batch_cases(t, seed=20261024):
    """one draw from every batch class of the type (both sides of the token-tile switch where the kernel has one)"""
    rng = np.random.default_rng([seed, t])
    out = []
    for i, vs in enumerate(batch_classes(t).values()):
        nb = int(rng.choice(vs))
        cap = max(16, _cost_cap(t) // 3 // nb)                        # three tokens go through the restatement
        rows = int(rng.choice([r for r in BATCH_ROWS if r <= cap])) if rng.integers(0, 2) else int(rng.integers(1, min(600, cap) + 1))
        out.append(BatchCase(i, t, nb * 256, rows, int(rng.choice(BATCH_T)), bool(rng.integers(0, 2)), bool(rng.integers(0, 2))))
    return out


# two per activation form: (types of q | k | v, rows — the middle segment ragged, K, T) and the type of the gate / up pair
BATCH_SEG = {
    "q8_0": ((Q8_0, IQ4_NL, Q5_0), (72, 13, 24), 1536, 17, Q4_0),
    "q8_1": ((Q4_1, Q5_1, Q4_1), (72, 13, 24), 1536, 17, Q5_1),
    "f32":  ((F16, F32, F16), (72, 13, 24), 768, 17, F32),
    "bf16": ((BF16, BF16, BF16), (72, 13, 24), 768, 17, BF16),
    "q8_K": ((Q2_K, Q6_K, Q3_K), (72, 13, 24), 1536, 17, Q3_K),
}
