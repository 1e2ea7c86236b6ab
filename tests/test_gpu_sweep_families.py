"""GPU: the seeded shape sweep of tests/test_gpu_sweep.py for the eleven weight types added after Q4_K / Q5_K / Q6_K: Q2_K / Q3_K, Q8_0 / Q4_0 / Q5_0, Q4_1 / Q5_1,
IQ4_NL, F16 / BF16 / F32.  The fixed lists of the per-family op tests pin the shapes the models use; this sweep is for the branches those lists never reach:
the depth-2 ring refilling inside a row (K / 256 = 6, 14, 22), a wave's second and third row-group in mode A, the edges of split-K for the Q8_0 family, odd
chunk counts and units without a second row-group in the float kernel, ragged and odd-sized segments in the middle of a fused launch.

The case lists come from tests/family_cases.py (seeded; tests/test_sweep_cases.py holds them to their classes on the CPU).  Every expectation is the numpy
restatement that the CPU tests hold to the genuine reference's outputs; bit equality throughout (bitcheck.assert_bits, which also wants the expectation finite),
and every expectation is checked not to be all zero."""
import numpy as np
import pytest

import family_cases as fc
from bitcheck import EPS, SILU_MUL, STORE, assert_bits, normed, silu_mul
from mfma_harness import ENV, prefill_switches

pytestmark = pytest.mark.gpu


def name(t):
    return fc.family(t).name


def ids(cases):
    fmt = (("i", "%d"), ("K", "K%d"), ("rows", "r%d"), ("T", "T%d"), ("epi", "%s"))
    return ["-".join([name(c.t)] + [f % getattr(c, k) for k, f in fmt if hasattr(c, k)]) for c in cases]


def want_of(po, t, W, rows, K, a):
    y = fc.family(t).ref(po, t, W, rows, K, a)
    assert np.isfinite(y).all() and np.any(y != 0), "the expectation is finite and not all zero"
    return y


def activation(rng, K, i):
    """a vector whose scale moves over 10^+-2; every fifth case has an all-zero leading block (K = 256: half a block, the vector is not to be all zero)"""
    x = (rng.standard_normal(K) * 10 ** rng.uniform(-2, 2)).astype(np.float32)
    if i % 5 == 0:
        x[:min(256, K // 2)] = 0.0
    return x


def norm_weight(rng, K):
    return (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)


# ---- 1. mat-vec ------------------------------------------------------------------------------------------------------------------------------------
MATVEC = [c for t in fc.TYPES for c in fc.matvec_cases(t)]


@pytest.mark.parametrize("c", MATVEC, ids=ids(MATVEC))
def test_mul_mat_vec_sweep(bamd, po, c):
    """every launch mode the type has gives the restatement's bits: 0 (the launcher's choice), 1 (one wave per row-group) and, where split-K exists, 2 — which
    at K / 256 = 7 and 57 must fall back to one wave per row-group"""
    f = fc.FAMILIES[c.t]
    rng = np.random.default_rng([7100, c.t, c.i])
    W = f.gen(c.t, c.K, c.rows, rng, float(10 ** rng.uniform(-1, 1)))
    x = activation(rng, c.K, c.i)
    w = norm_weight(rng, c.K) if c.norm else None
    res = rng.standard_normal(c.rows).astype(np.float32) if c.resid else None
    want = want_of(po, c.t, W, c.rows, c.K, x if w is None else normed(po, x, w))
    if res is not None:
        want = want + res
    for mode in f.modes:
        got = bamd.op_mul_mat_vec(c.t, W, c.rows, c.K, x, norm_w=w, eps=EPS, residual=res, mode=mode)
        assert_bits(got, want, "%s K %d rows %d norm %d residual %d mode %d" % (f.name, c.K, c.rows, c.norm, c.resid, mode))


# ---- 2. gate/up and arg-max ------------------------------------------------------------------------------------------------------------------------
GATEUP = [c for t in fc.TYPES for c in fc.gateup_cases(t)]
ARGMAX = [c for t in fc.TYPES for c in fc.argmax_cases(t)]


@pytest.mark.parametrize("c", GATEUP, ids=ids(GATEUP))
def test_ffn_gate_up_sweep(bamd, po, c):
    """the fused gate/up launch (RMSNorm prologue, SiLU epilogue) at ragged rows"""
    f = fc.FAMILIES[c.t]
    rng = np.random.default_rng([7200, c.t, c.i])
    Wg = f.gen(c.t, c.K, c.rows, rng, 4.0)
    Wu = f.gen(c.t, c.K, c.rows, rng, 4.0)
    x = (rng.standard_normal(c.K) * 2).astype(np.float32)
    w = norm_weight(rng, c.K)
    a = normed(po, x, w)
    want = silu_mul(po, want_of(po, c.t, Wg, c.rows, c.K, a), want_of(po, c.t, Wu, c.rows, c.K, a))
    assert_bits(bamd.op_ffn_gate_up(c.t, Wg, Wu, c.rows, c.K, x, norm_w=w, eps=EPS), want, "gate/up %s K %d rows %d" % (f.name, c.K, c.rows))


def plant_tie(po, t, W, rows, K, a, tied):
    """moves the row with the largest logit into the rows `tied` (and the row with the smallest to where it was); returns the matrix and its expectation, whose
    maximum then sits in exactly those rows.  A row's logit depends on that row alone, so the expectation moves with the rows: one pass of the restatement"""
    W = W.reshape(rows, -1).copy()
    want = want_of(po, t, W.reshape(-1), rows, K, a)
    top = int(np.argmax(want))
    free = np.setdiff1d(np.arange(rows), tied)
    bottom = int(free[np.argmin(want[free])])
    best, peak = W[top].copy(), want[top]
    if top not in tied:
        W[top] = W[bottom]; want[top] = want[bottom]
    W[tied] = best; want[tied] = peak
    assert np.flatnonzero(want == want.max()).tolist() == sorted(tied)
    return W.reshape(-1), want


@pytest.mark.parametrize("c", ARGMAX, ids=ids(ARGMAX))
def test_argmax_sweep(bamd, po, c):
    """the lm_head launch with its arg-max epilogue at ragged rows; the largest logit is a tie between a row a third of the way down and the last valid row
    (the ragged row-group), which different workgroups own: logits and the lower row"""
    f = fc.FAMILIES[c.t]
    rng = np.random.default_rng([7300, c.t, c.i])
    W = f.gen(c.t, c.K, c.rows, rng, 4.0)
    x = (rng.standard_normal(c.K) * 2).astype(np.float32)
    w = norm_weight(rng, c.K)
    nrg = (c.rows + 7) // 8
    tied = [8 * (nrg // 3) + 5, c.rows - 1]
    per = 2 if c.t in fc.FLOAT_TYPES else 1          # the float kernels deal units of two row-groups
    walks = -(-nrg // per)
    assert (tied[0] // 8 // per) % min(fc.GRID, walks) != (tied[1] // 8 // per) % min(fc.GRID, walks), "the tied rows belong to different workgroups"
    W, want = plant_tie(po, c.t, W, c.rows, c.K, normed(po, x, w), tied)
    got, row = bamd.op_mul_mat_vec_argmax(c.t, W, c.rows, c.K, x, norm_w=w, eps=EPS, mode=0)
    assert_bits(got, want, "arg-max logits %s K %d rows %d" % (f.name, c.K, c.rows))
    assert row == tied[0], "the lower of the tied rows"


# ---- 3. fused launches over segments of one activation form ------------------------------------------------------------------------------------------
SEGMENTS = fc.segment_cases()


@pytest.mark.parametrize("c", SEGMENTS, ids=["%d-%s-K%d-%s" % (c.i, "|".join(name(t) for t in c.types), c.K, "|".join(map(str, c.rows))) for c in SEGMENTS])
def test_fused_segments_sweep(bamd, po, c):
    """two and three differently typed segments behind one RMSNorm prologue in one launch, in every mode the mix has: odd row-group counts and ragged rows in
    segments that are not the last, a segment smaller than the grid beside a larger one, and (the last two cases) split-K over Q8_0 | Q4_0 | Q5_0 with more
    row-groups than workgroups, so that a workgroup's buffer parity and chain wave carry from one segment's type into the next (family_cases.segment_cases)"""
    rng = np.random.default_rng([7400, c.i])
    Ws = [fc.family(t).gen(t, c.K, r, rng) for t, r in zip(c.types, c.rows)]
    x = (rng.standard_normal(c.K) * 2).astype(np.float32)
    w = norm_weight(rng, c.K)
    a = normed(po, x, w)
    want = np.concatenate([want_of(po, t, W, r, c.K, a) for t, W, r in zip(c.types, Ws, c.rows)])
    for mode in c.modes:
        got = bamd.op_fused_qkv(list(zip(c.types, Ws, c.rows)), c.K, x, w, eps=EPS, mode=mode)
        assert_bits(got, want, "segments %r rows %r K %d mode %d" % (c.types, c.rows, c.K, mode))


# ---- 4. more row-groups than the grid has waves --------------------------------------------------------------------------------------------------------
TALL = [c for t in fc.TYPES for c in fc.tall_cases(t)]


@pytest.mark.parametrize("c", TALL, ids=ids(TALL))
def test_tall_matrix_more_row_groups_than_wave_slots(bamd, po, c):
    """mode A on 256 workgroups of 8 waves gives a wave a second row-group only above 2048 row-groups (16 384 rows; the float kernels, which take two row-groups
    per walk, above 4096): here 2049 and 4099 (doubled for the float types), so that one wave, or all of them and three a third time, run the next-row-group
    prefetch, the `last` flag of the final refill and, under gate/up, the gate -> up -> next gate hand-over.  Residual add in mode 1, gate/up, and arg-max
    with the top tied between a row of the first row-group that only a second walk reaches and the last valid row: the lower one wins.  Every row is checked."""
    f = fc.FAMILIES[c.t]
    rng = np.random.default_rng([7500, c.t, c.K])
    x = (rng.standard_normal(c.K) * 2).astype(np.float32)
    what = "tall %s K %d row-groups %d %s" % (f.name, c.K, c.nrg, c.epi)
    if c.epi == "add":
        W = f.gen(c.t, c.K, c.rows, rng)
        res = rng.standard_normal(c.rows).astype(np.float32)
        want = want_of(po, c.t, W, c.rows, c.K, x) + res
        assert_bits(bamd.op_mul_mat_vec(c.t, W, c.rows, c.K, x, residual=res, mode=1), want, what)
    elif c.epi == "gateup":
        w = norm_weight(rng, c.K)
        a = normed(po, x, w)
        Wg = f.gen(c.t, c.K, c.rows, rng, 4.0)
        Wu = f.gen(c.t, c.K, c.rows, rng, 4.0)
        want = silu_mul(po, want_of(po, c.t, Wg, c.rows, c.K, a), want_of(po, c.t, Wu, c.rows, c.K, a))
        assert_bits(bamd.op_ffn_gate_up(c.t, Wg, Wu, c.rows, c.K, x, norm_w=w, eps=EPS), want, what)
    else:
        w = norm_weight(rng, c.K)
        per = 2 if c.t in fc.FLOAT_TYPES else 1
        tied = [8 * fc.WAVE_SLOTS * per + 1, c.rows - 1]           # both in row-groups that no wave holds in its first walk
        assert tied[0] < tied[1]
        W, want = plant_tie(po, c.t, f.gen(c.t, c.K, c.rows, rng, 4.0), c.rows, c.K, normed(po, x, w), tied)
        got, row = bamd.op_mul_mat_vec_argmax(c.t, W, c.rows, c.K, x, norm_w=w, eps=EPS, mode=1)
        assert_bits(got, want, what)
        assert row == tied[0], what + ": the lower of the tied rows"


# ---- 5. prompt evaluation ------------------------------------------------------------------------------------------------------------------------------
BATCH = [c for t in fc.TYPES for c in fc.batch_cases(t)]


@pytest.mark.parametrize("c", BATCH, ids=ids(BATCH))
def test_mul_mat_batch_sweep(bamd, po, c):
    """the integer-dot (float types: VALU) batch kernel against the restatement for the first, the middle and the last token, and, where the type has a matrix-core
    kernel, that kernel against the first for every token.  Its launch counter must advance by exactly one: a silent fall-back cannot pass.  The switch goes back
    to what the environment set"""
    f = fc.FAMILIES[c.t]
    rng = np.random.default_rng([7600, c.t, c.i])
    W = f.gen(c.t, c.K, c.rows, rng, float(10 ** rng.uniform(-1, 1)))
    X = (rng.standard_normal((c.T, c.K)) * 10 ** rng.uniform(-1, 1)).astype(np.float32)
    w = norm_weight(rng, c.K) if c.norm else None
    res = rng.standard_normal((c.T, c.rows)).astype(np.float32) if c.resid else None
    what = "batch %s K %d rows %d T %d norm %d residual %d" % (f.name, c.K, c.rows, c.T, c.norm, c.resid)
    plain = bamd.op_mul_mat_batch(c.t, W, c.rows, c.K, X, norm_w=w, eps=EPS, residual=res, impl=0)
    for tok in sorted({0, c.T // 2, c.T - 1}):
        want = want_of(po, c.t, W, c.rows, c.K, X[tok] if w is None else normed(po, X[tok], w))
        assert_bits(plain[tok], want if res is None else want + res[tok], what + " token %d" % tok)
    if f.switch is not None:
        with prefill_switches(bamd, **{f.switch: True}):
            before = bamd.prefill_mfma_runs(c.t)
            mfma = bamd.op_mul_mat_batch(c.t, W, c.rows, c.K, X, norm_w=w, eps=EPS, residual=res, impl=2)
            assert bamd.prefill_mfma_runs(c.t) == before + 1, what + ": one matrix-core launch"
        assert np.isfinite(plain).all()
        assert_bits(mfma, plain, what + ": matrix-core kernel vs impl 0")


# ---- 6. the segment form of the prompt mat-muls, mixed types ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(fc.BATCH_SEG))
def test_mul_mat_batch_seg_qkv_mixed_types(bamd, po, form):
    """q | k | v of three types of one activation form into [T][ldo], the middle segment ragged; the columns behind the rows keep their fill"""
    types, rows, K, T, _ = fc.BATCH_SEG[form]
    rng = np.random.default_rng([7700, K, T, len(form)])
    Ws = [fc.family(t).gen(t, K, r, rng) for t, r in zip(types, rows)]
    X = (rng.standard_normal((T, K)) * 2).astype(np.float32)
    w = norm_weight(rng, K)
    ldo = sum(rows) + 8
    got = bamd.op_mul_mat_batch_seg(list(zip(types, Ws, rows)), K, X, ldo, epi=STORE, norm_w=w, eps=EPS, fill=-7.0)
    want = np.full((T, ldo), -7.0, np.float32)
    for i in range(T):
        a = normed(po, X[i], w)
        want[i, :sum(rows)] = np.concatenate([want_of(po, t, W, r, K, a) for t, W, r in zip(types, Ws, rows)])
    assert_bits(got, want, "q | k | v %s" % form)


@pytest.mark.parametrize("form", sorted(fc.BATCH_SEG))
def test_mul_mat_batch_seg_gate_up(bamd, po, form):
    """gate and up of one type with the SiLU epilogue at 29 rows (ragged); K / 256 = 6 for the quantised forms, 3 for f32 and bf16"""
    _, _, K, T, t = fc.BATCH_SEG[form]
    rows = 29
    rng = np.random.default_rng([7800, K, T, len(form)])
    Wg, Wu = (fc.family(t).gen(t, K, rows, rng, 4.0) for _ in range(2))
    X = (rng.standard_normal((T, K)) * 2).astype(np.float32)
    w = norm_weight(rng, K)
    got = bamd.op_mul_mat_batch_seg([(t, Wg, rows), (t, Wu, rows)], K, X, rows, epi=SILU_MUL, norm_w=w, eps=EPS)
    A = [normed(po, X[i], w) for i in range(T)]
    want = np.stack([silu_mul(po, want_of(po, t, Wg, rows, K, a), want_of(po, t, Wu, rows, K, a)) for a in A])
    assert_bits(got, want, "gate / up %s" % form)


def test_the_switches_are_where_the_environment_set_them(bamd):
    """after the sweep (and on its own): a case with a family's switch off must be refused at impl 2 exactly when the environment left the switch off — the
    tests above restore what they set"""
    rng = np.random.default_rng(1)
    for t, f in fc.FAMILIES.items():
        if f.switch is None or ENV[f.switch]:
            continue
        W = f.gen(t, 256, 8, rng)
        with pytest.raises(bamd.BamdError, match="MFMA path: unsupported type/shape"):
            bamd.op_mul_mat_batch(t, W, 8, 256, np.ones((2, 256), np.float32), impl=2)
