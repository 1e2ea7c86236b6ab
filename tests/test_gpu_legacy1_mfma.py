"""GPU: the matrix-core prompt mat-mul for Q4_1 / Q5_1 weights (booster_amd/csrc/bamd_prefill2_b32.hip, behind set_prefill_q1 / BAMD_PREFILL_Q1=1; default off).
Every expectation is the genuine reference's stored output (tests/golden/legacy1_kats.npz, tests/golden/legacy1_*.bgld) or the numpy restatement that
tests/test_legacy1_ref.py holds to those (tests/legacy1_ref.py); bit equality throughout.  The switches are set through their setters and restored afterwards; the
launch counters (prefill_mfma_runs) tell the matrix-core kernel from the integer-dot kernel, which gives the same bits.

Tile edges of the kernel: a workgroup is 64 rows x 32 tokens, a wave 16 rows x two token tiles of 16, a record group 8 rows."""
import numpy as np
import pytest

import legacy1_ref as l1
import legacy_ref as lg
from bitcheck import ADD, EPS, FILL, SILU_MUL, STORE, assert_bits, normed, silu_mul
from booster_amd.gguf import random_q0_tensor, random_q1_tensor
from legacy1_ref import all_cases
from mfma_harness import layer_types, no_tables_with_the_switches_off, prefill_switches, prompt_step, runs, two_stages_on_the_matrix_cores
from refmodel import LEGACY1, load_fixture, model_for
from test_legacy1_ref import stored, stored_case  # noqa: F401  (stored: fixture)

pytestmark = pytest.mark.gpu
Q4_1, Q5_1 = l1.Q4_1, l1.Q5_1
Q4_0, Q5_0, Q8_0 = lg.Q4_0, lg.Q5_0, lg.Q8_0
TYPES = [Q4_1, Q5_1]
COUNTED = TYPES + [Q4_0, Q5_0, Q8_0, 14]


def ref_batch(t, W, rows, K, A):
    return np.stack([l1.mul_mat(t, W, rows, K, a) for a in A])


@pytest.mark.parametrize("t", TYPES)
def test_switch_is_off_by_default_and_refuses(bamd, t):
    """off: impl 2 declines the types as before and counts nothing — also with the OTHER family's switch on; on: it runs and counts.  (The first refusal is asked
    for before any setter call: under BAMD_PREFILL_Q1=1 in the environment this test fails, by design.)"""
    blocks, xs, _ = l1.rand_case(t, 256)
    before = runs(bamd, COUNTED)
    with pytest.raises(bamd.BamdError, match="MFMA path: unsupported type/shape"):
        bamd.op_mul_mat_batch(t, blocks, l1.ROWS, 256, np.stack(xs), impl=2)
    with prefill_switches(bamd, q1=False, q0=True):
        with pytest.raises(bamd.BamdError, match="MFMA path: unsupported type/shape"):
            bamd.op_mul_mat_batch(t, blocks, l1.ROWS, 256, np.stack(xs), impl=2)
    assert runs(bamd, COUNTED) == before
    with prefill_switches(bamd, q1=True, q0=False):
        bamd.op_mul_mat_batch(t, blocks, l1.ROWS, 256, np.stack(xs), impl=2)
    after = runs(bamd, COUNTED)
    assert after[t] == before[t] + 1 and all(after[u] == before[u] for u in after if u != t)


# ---- the reference's own outputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("T", [2, 7, 64])
def test_mul_mat_batch_kats(bamd, stored, t, T):
    """every stored case — K = 256, 512, 4096, 11008 and the edge matrix (d negative, zero, subnormal, large; m zero, negative, large; quants at both ends; Q5_1: qh
    all zeros and all ones) — on the matrix-core kernel"""
    rng = np.random.default_rng(T + t)
    with prefill_switches(bamd, q1=True, q0=False):
        for key, blocks, xs, digest, _ in all_cases(t):
            dots, _, _ = stored_case(stored, key, digest)
            K = xs[0].size
            pick = [i % len(xs) for i in range(T)]
            X = np.stack([xs[i] for i in pick])
            want = np.stack([dots[i] for i in pick])
            res = rng.standard_normal((T, l1.ROWS)).astype(np.float32)
            for r in (None, res):
                before = bamd.prefill_mfma_runs(t)
                got = bamd.op_mul_mat_batch(t, blocks, l1.ROWS, K, X, residual=r, impl=2)
                assert bamd.prefill_mfma_runs(t) == before + 1
                assert_bits(got, want if r is None else want + r, "%s T %d residual %d" % (key, T, r is not None))
            if T == 7:                                # the first 29 rows only: a ragged last row-group, and rows of 29 floats (unaligned stores)
                rb = K // 32 * l1.BB[t]
                got = bamd.op_mul_mat_batch(t, blocks[:29 * rb], 29, K, X, residual=res[:, :29], impl=2)
                assert_bits(got, want[:, :29] + res[:, :29], "%s T %d, 29 rows" % (key, T))


# ---- shapes, expectation from the restatement ------------------------------------------------------------------------------------------------------
SHAPE_ROWS, SHAPE_T = 72, 65
_shape_ref = {}


def shape_ref(po, t, K, norm):
    """one matrix of 72 rows and 65 token rows per (type, K), and W . Q8_1(x_t) of all of them with and without the RMSNorm prologue: the smaller shapes are the
    first rows and the first tokens of these"""
    if (t, K) not in _shape_ref:
        rng = np.random.default_rng(1013 * t + K)
        W = random_q1_tensor(t, K, SHAPE_ROWS, rng)
        X = (rng.standard_normal((SHAPE_T, K)) * 3).astype(np.float32)
        w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
        res = rng.standard_normal((SHAPE_T, SHAPE_ROWS)).astype(np.float32)
        _shape_ref[(t, K)] = dict(W=W, X=X, w=w, res=res)
    c = _shape_ref[(t, K)]
    if norm not in c:
        A = c["X"] if not norm else np.stack([normed(po, x, c["w"]) for x in c["X"]])
        c[norm] = ref_batch(t, c["W"], SHAPE_ROWS, K, A)
    return c, c[norm]


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("K", [256, 512, 768])                  # one record (the prologue's stage only), two, an odd count
@pytest.mark.parametrize("rows", [8, 24, 72])                   # less than a wave's 16 rows, an odd row-group count, a partial second 64-row workgroup
@pytest.mark.parametrize("T", [1, 16, 17, 32, 33, 64, 65])      # both sides of the 16-token tile and of the 32-token workgroup
def test_mul_mat_batch_shapes(bamd, po, t, K, rows, T):
    rb = K // 32 * l1.BB[t]
    with prefill_switches(bamd, q1=True, q0=False):
        for norm in (False, True):
            c, want = shape_ref(po, t, K, norm)
            for with_res in (False, True):
                res = np.ascontiguousarray(c["res"][:T, :rows]) if with_res else None
                got = bamd.op_mul_mat_batch(t, c["W"][:rows * rb], rows, K, c["X"][:T], norm_w=c["w"] if norm else None, eps=EPS, residual=res, impl=2)
                assert_bits(got, want[:T, :rows] + res if with_res else want[:T, :rows], "type %d K %d rows %d T %d norm %d residual %d" % (t, K, rows, T, norm, with_res))


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("rows", [16, 64])                      # exactly a wave's rows, exactly a workgroup's (the shapes above straddle both)
def test_mul_mat_batch_row_tile_edges(bamd, po, t, rows):
    K, T = 512, 33
    rb = K // 32 * l1.BB[t]
    c, want = shape_ref(po, t, K, False)
    with prefill_switches(bamd, q1=True, q0=False):
        assert_bits(bamd.op_mul_mat_batch(t, c["W"][:rows * rb], rows, K, c["X"][:T], impl=2), want[:T, :rows], "type %d rows %d" % (t, rows))


@pytest.mark.parametrize("t", TYPES)
def test_mul_mat_batch_43_records(bamd, po, t):
    """K = 11008, the 43 records of Llama-2's ffn_down"""
    K, rows, T = 11008, 8, 3
    rng = np.random.default_rng(43 + t)
    W = random_q1_tensor(t, K, rows, rng)
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    res = rng.standard_normal((T, rows)).astype(np.float32)
    with prefill_switches(bamd, q1=True, q0=False):
        assert_bits(bamd.op_mul_mat_batch(t, W, rows, K, X, impl=2), ref_batch(t, W, rows, K, X), "K 11008 plain")
        A = np.stack([normed(po, x, w) for x in X])
        assert_bits(bamd.op_mul_mat_batch(t, W, rows, K, X, norm_w=w, eps=EPS, residual=res, impl=2), ref_batch(t, W, rows, K, A) + res, "K 11008 norm + residual")


@pytest.mark.parametrize("t", TYPES)
def test_s_x_of_the_f16_records_is_rounded_twice(bamd, t):
    """a batch whose tokens include the double-rounding vector (every block's s = f16(f32(d * sum)) differs from the exact product rounded once), the matrix cut
    to its ROUND2_K columns: the f16 activation records must carry the twice-rounded s of the Q8_1 image.  That a once-rounded s gives other bits on this very
    matrix is asserted on the restatement first, so the case cannot lose its teeth silently"""
    K, rows = l1.ROUND2_K, 24
    rng = np.random.default_rng(2222 + t)
    W = random_q1_tensor(t, K, rows, rng)
    x2 = l1.double_rounding_vector()
    X = np.stack([(rng.standard_normal(K) * 3).astype(np.float32), x2, (rng.standard_normal(K) * 0.5).astype(np.float32), x2])
    want = ref_batch(t, W, rows, K, X)
    q8 = l1.quantize_row_q8_1(x2).reshape(-1, 36).copy()
    d32 = (np.abs(x2.reshape(-1, 32)).max(axis=1) / np.float32(127.0)).astype(np.float32)
    qsum = q8[:, 4:].copy().view(np.int8).astype(np.int64).sum(axis=1)
    q8[:, 2:4] = (d32.astype(np.float64) * qsum).astype(np.float16).view(np.uint8).reshape(-1, 2)
    once = l1.vec_dot_rows(t, W, q8.reshape(-1))
    assert (once.view(np.uint32) != want[1].view(np.uint32)).any(), "a once-rounded s gives the same bits: the case checks nothing"
    with prefill_switches(bamd, q1=True, q0=False):
        before = bamd.prefill_mfma_runs(t)
        got = bamd.op_mul_mat_batch(t, W, rows, K, X, impl=2)
        assert bamd.prefill_mfma_runs(t) == before + 1
    assert_bits(got, want, "double-rounding tokens, type %d" % t)


@pytest.mark.parametrize("t", TYPES)
def test_matrix_core_kernel_equals_integer_dot_kernel(bamd, t):
    K, rows, T = 4096, 256, 65
    rng = np.random.default_rng(4096 + t)
    W = random_q1_tensor(t, K, rows, rng)
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    with prefill_switches(bamd, q1=True, q0=False):
        before = bamd.prefill_mfma_runs(t)
        a = bamd.op_mul_mat_batch(t, W, rows, K, X, norm_w=w, eps=EPS, impl=2)
        assert bamd.prefill_mfma_runs(t) == before + 1
        b = bamd.op_mul_mat_batch(t, W, rows, K, X, norm_w=w, eps=EPS, impl=0)
        assert bamd.prefill_mfma_runs(t) == before + 1
    assert np.isfinite(b).all() and np.abs(b).max() > 0
    assert_bits(a, b, "impl 2 vs impl 0")


# ---- routing, as the engine issues the launches -------------------------------------------------------------------------------------------------------
def test_seg_q4_1_beside_q5_1_into_one_matrix(bamd, po):
    """Q4_1 | Q4_1 | Q5_1 (q | k | v) into one [T][ldo]: one launch per segment, the fill behind the rows untouched"""
    K, T, rows = 512, 17, [256, 64, 72]
    rng = np.random.default_rng(818)
    types = [Q4_1, Q4_1, Q5_1]
    Ws = [random_q1_tensor(t, K, r, rng) for t, r in zip(types, rows)]
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    A = np.stack([normed(po, x, w) for x in X])
    ldo = sum(rows) + 9
    want = np.concatenate([ref_batch(t, W, r, K, A) for t, W, r in zip(types, Ws, rows)], axis=1)
    with prefill_switches(bamd, q1=True, q0=False):
        before = runs(bamd, COUNTED)
        got = bamd.op_mul_mat_batch_seg([(t, W, r) for t, W, r in zip(types, Ws, rows)], K, X, ldo, epi=STORE, norm_w=w, eps=EPS, impl=2, fill=FILL)
        after = runs(bamd, COUNTED)
    assert after[Q4_1] == before[Q4_1] + 2 and after[Q5_1] == before[Q5_1] + 1 and all(after[u] == before[u] for u in after if u not in TYPES)
    assert_bits(got[:, :sum(rows)], want, "q | k | v")
    assert (got[:, sum(rows):] == FILL).all(), "wrote behind the rows"


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("T", [7, 65])
def test_seg_silu_mul_pair(bamd, po, t, T):
    """gate, then up with h = silu(gate) * up as its in-place epilogue (res == out): two launches of the type, nothing written behind the rows"""
    K, rows = 512, 768
    rng = np.random.default_rng([51, t, T])
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    Wg, Wu = random_q1_tensor(t, K, rows, rng), random_q1_tensor(t, K, rows, rng)
    A = np.stack([normed(po, x, w) for x in X])
    g, u = ref_batch(t, Wg, rows, K, A), ref_batch(t, Wu, rows, K, A)
    want = silu_mul(po, g.reshape(-1), u.reshape(-1)).reshape(T, rows)
    with prefill_switches(bamd, q1=True, q0=False):
        before = bamd.prefill_mfma_runs(t)
        got = bamd.op_mul_mat_batch_seg([(t, Wg, rows), (t, Wu, rows)], K, X, rows + 64, epi=SILU_MUL, norm_w=w, eps=EPS, impl=2, fill=FILL)
        assert bamd.prefill_mfma_runs(t) == before + 2
    assert_bits(got[:, :rows], want, "silu(gate) * up type %d T %d" % (t, T))
    assert (got[:, rows:] == FILL).all(), "wrote behind the rows"


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("ldo", [832, 835])           # rows of a token 16-byte aligned, and not
def test_seg_add_with_wide_rows(bamd, po, t, ldo):
    """residual add with ldo > rows: output and residual share the stride, the columns behind the rows stay untouched"""
    K, rows, T = 512, 760, 65
    rng = np.random.default_rng([61, t])
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    W = random_q1_tensor(t, K, rows, rng)
    res = rng.standard_normal((T, ldo)).astype(np.float32)
    want = ref_batch(t, W, rows, K, X) + res[:, :rows]
    with prefill_switches(bamd, q1=True, q0=False):
        before = bamd.prefill_mfma_runs(t)
        got = bamd.op_mul_mat_batch_seg([(t, W, rows)], K, X, ldo, epi=ADD, residual=res, impl=2, fill=FILL)
        assert bamd.prefill_mfma_runs(t) == before + 1
    assert_bits(got[:, :rows], want, "add type %d" % t)
    assert (got[:, rows:] == FILL).all(), "wrote behind the rows"


def test_seg_q4_0_beside_q4_1_is_still_refused(bamd):
    """both switches on: Q4_0 | Q4_0 | Q4_1 in ONE call needs two activation forms (Q8_0 and Q8_1) and is refused as before; nothing is launched"""
    K, T, rows = 512, 5, [64, 16, 16]
    rng = np.random.default_rng(828)
    segs = [(Q4_0, random_q0_tensor(Q4_0, K, rows[0], rng), rows[0]), (Q4_0, random_q0_tensor(Q4_0, K, rows[1], rng), rows[1]), (Q4_1, random_q1_tensor(Q4_1, K, rows[2], rng), rows[2])]
    X = rng.standard_normal((T, K)).astype(np.float32)
    with prefill_switches(bamd, q1=True, q0=True):
        before = runs(bamd, COUNTED)
        with pytest.raises(bamd.BamdError, match="different activation forms"):
            bamd.op_mul_mat_batch_seg(segs, K, X, sum(rows), epi=STORE, impl=2)
        assert runs(bamd, COUNTED) == before


def test_q4_0_gate_up_beside_a_q4_1_down_matrix(bamd, po):
    """the layer 0 of a Q4_0 file made with an importance matrix, both switches on: the Q4_0 gate / up pair and the Q4_1 ffn_down run in separate calls (each
    with its own activation form), each on the matrix-core kernel of its family"""
    E, F, T = 512, 768, 33
    rng = np.random.default_rng(838)
    X = (rng.standard_normal((T, E)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(E)).astype(np.float32)
    Wg, Wu = random_q0_tensor(Q4_0, E, F, rng, amp=4.0), random_q0_tensor(Q4_0, E, F, rng, amp=4.0)
    Wd = random_q1_tensor(Q4_1, F, E, rng)
    A = np.stack([normed(po, x, w) for x in X])
    g = np.stack([lg.mul_mat(Q4_0, Wg, F, E, a) for a in A]); u = np.stack([lg.mul_mat(Q4_0, Wu, F, E, a) for a in A])
    h = silu_mul(po, g.reshape(-1), u.reshape(-1)).reshape(T, F).astype(np.float32)
    res = rng.standard_normal((T, E)).astype(np.float32)
    want = ref_batch(Q4_1, Wd, E, F, h) + res
    with prefill_switches(bamd, q1=True, q0=True):
        before = runs(bamd, COUNTED)
        got_h = bamd.op_mul_mat_batch_seg([(Q4_0, Wg, F), (Q4_0, Wu, F)], E, X, F, epi=SILU_MUL, norm_w=w, eps=EPS, impl=2)
        mid = runs(bamd, COUNTED)
        got = bamd.op_mul_mat_batch_seg([(Q4_1, Wd, E)], F, got_h, E, epi=ADD, residual=res, impl=2)
        after = runs(bamd, COUNTED)
    assert mid[Q4_0] == before[Q4_0] + 2 and mid[Q4_1] == before[Q4_1]
    assert after[Q4_1] == mid[Q4_1] + 1 and after[Q4_0] == mid[Q4_0]
    assert_bits(got_h, h, "silu(gate) * up, Q4_0")
    assert_bits(got, want, "ffn_down, Q4_1")


# ---- whole models against the genuine reference's llama_decode ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["tiny_q4_1", "tiny_q5_1", "8bw_q4_1", "8bw_q5_1"])
def test_whole_model_prompt_on_the_matrix_cores(bamd, cfg, monkeypatch, capfd):
    """the prompt step only: tables built, no load-time complaint, the counters of the file's layer types move, logits bit-identical"""
    fx = load_fixture(LEGACY1, cfg)
    path = model_for(LEGACY1, cfg, fx)
    low = layer_types(path, COUNTED[:5])
    assert low and low <= set(TYPES)
    monkeypatch.setenv("BAMD_PREFILL_VERBOSE", "1")
    err, aux, before, after = prompt_step(bamd, path, capfd, COUNTED, dict(q1=True, q0=False), fam=LEGACY1, cfg=cfg, fx=fx)
    assert "prompts run without the matrix-core kernels" not in err, err
    assert aux > 0
    for t in low:
        assert after[t] > before[t], "no matrix-core launch of type %d" % t
    no_tables_with_the_switches_off(bamd, path, "q1", "q0")


@pytest.mark.parametrize("cfg,t0,t1", [("tiny_q4_0_imat", Q4_0, Q4_1), ("tiny_q5_0_imat", Q5_0, Q5_1)])
def test_imatrix_file_needs_both_switches(bamd, cfg, t0, t1, monkeypatch, capfd):
    """a Q4_0 / Q5_0 file made with an importance matrix (ffn_down of layer 0 is Q4_1 / Q5_1).  Both switches on: tables, both families' counters move.  Only the
    Q0 switch: no tables, the reason names the missing switch, nothing on the matrix cores.  Same logits — the reference's — either way"""
    fx = load_fixture(LEGACY1, cfg)
    path = model_for(LEGACY1, cfg, fx)
    assert layer_types(path, COUNTED[:5]) == {t0, t1}
    monkeypatch.setenv("BAMD_PREFILL_VERBOSE", "1")
    step = lambda q1, q0: prompt_step(bamd, path, capfd, COUNTED, dict(q1=q1, q0=q0), fam=LEGACY1, cfg=cfg, fx=fx)
    err, aux, before, after = step(q1=True, q0=True)
    assert "prompts run without the matrix-core kernels" not in err, err
    assert aux > 0
    assert after[t0] > before[t0] and after[t1] > before[t1], "both families on the matrix cores: %r -> %r" % (before, after)
    err, aux, before, after = step(q1=False, q0=True)
    assert aux == 0
    assert "prompts run without the matrix-core kernels" in err and "BAMD_PREFILL_Q1 is off" in err and "all-or-nothing per model" in err and "integer-dot kernel" in err, err
    assert after == before, "a launch on the matrix cores without side tables"
    err, aux, before, after = step(q1=True, q0=False)
    assert aux == 0
    assert "prompts run without the matrix-core kernels" in err and "BAMD_PREFILL_Q0 is off" in err, err
    assert after == before
    no_tables_with_the_switches_off(bamd, path, "q1", "q0")


def test_prompt_through_two_stages_on_the_matrix_cores(bamd):
    """tiny_q5_1 through two layer-split stages (bamd_stage_prefill): the stage path takes the same routing"""
    cfg = "tiny_q5_1"
    low = layer_types(model_for(LEGACY1, cfg, load_fixture(LEGACY1, cfg)), COUNTED[:5])
    assert low
    two_stages_on_the_matrix_cores(bamd, LEGACY1, cfg, COUNTED, low, dict(q1=True, q0=False))
