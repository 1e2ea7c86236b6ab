"""GPU: the matrix-core prompt mat-mul for Q8_0 / Q4_0 / Q5_0 weights (booster_amd/csrc/bamd_prefill2_b32.hip, behind set_prefill_q0 / BAMD_PREFILL_Q0=1; default
off).  Every expectation is the genuine reference's stored output (tests/golden/legacy_kats.npz, tests/golden/legacy_*.bgld) or the numpy restatement that
tests/test_legacy_ref.py holds to those (tests/legacy_ref.py); bit equality throughout.  The switch is set through the setter and restored afterwards; the launch
counters (prefill_mfma_runs) tell the matrix-core kernel from the integer-dot kernel, which gives the same bits.

Tile edges of the kernel: a workgroup is 64 rows x 32 tokens, a wave 16 rows x two token tiles of 16, a record group 8 rows."""
import numpy as np
import pytest

import legacy_ref as lg
from bitcheck import ADD, EPS, FILL, SILU_MUL, STORE, assert_bits, normed, silu_mul
from booster_amd.gguf import random_q0_tensor
from legacy_ref import all_cases
from mfma_harness import layer_types, no_tables_with_the_switches_off, prefill_switches, prompt_step, runs, two_stages_on_the_matrix_cores
from refmodel import LEGACY, load_fixture, model_for
from test_legacy_ref import stored, stored_case  # noqa: F401  (stored: fixture)

pytestmark = pytest.mark.gpu
Q4_0, Q5_0, Q8_0 = lg.Q4_0, lg.Q5_0, lg.Q8_0
TYPES = [Q8_0, Q4_0, Q5_0]
COUNTED = TYPES + [14]


def ref_batch(t, W, rows, K, A):
    return np.stack([lg.mul_mat(t, W, rows, K, a) for a in A])


@pytest.mark.parametrize("t", TYPES)
def test_switch_is_off_by_default_and_refuses(bamd, t):
    """off: impl 2 declines the types as before and counts nothing; on: it runs and counts"""
    blocks, xs, _ = lg.rand_case(t, 256)
    before = runs(bamd, COUNTED)
    with pytest.raises(bamd.BamdError, match="MFMA path: unsupported type/shape"):
        bamd.op_mul_mat_batch(t, blocks, lg.ROWS, 256, np.stack(xs), impl=2)
    assert runs(bamd, COUNTED) == before
    with prefill_switches(bamd, q0=True):
        bamd.op_mul_mat_batch(t, blocks, lg.ROWS, 256, np.stack(xs), impl=2)
    after = runs(bamd, COUNTED)
    assert after[t] == before[t] + 1 and all(after[u] == before[u] for u in after if u != t)


# ---- the reference's own outputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("T", [2, 7, 64])
def test_mul_mat_batch_kats(bamd, stored, t, T):
    """every stored case — K = 256, 512, 4096, 11008 and the edge matrix (weight byte -128, all-zero blocks, subnormal and zero f16 d) — on the matrix-core kernel"""
    rng = np.random.default_rng(T + t)
    with prefill_switches(bamd, q0=True):
        for key, blocks, xs, digest, _ in all_cases(t):
            dots, _, _ = stored_case(stored, key, digest)
            K = xs[0].size
            pick = [i % len(xs) for i in range(T)]
            X = np.stack([xs[i] for i in pick])
            want = np.stack([dots[i] for i in pick])
            res = rng.standard_normal((T, lg.ROWS)).astype(np.float32)
            for r in (None, res):
                before = bamd.prefill_mfma_runs(t)
                got = bamd.op_mul_mat_batch(t, blocks, lg.ROWS, K, X, residual=r, impl=2)
                assert bamd.prefill_mfma_runs(t) == before + 1
                assert_bits(got, want if r is None else want + r, "%s T %d residual %d" % (key, T, r is not None))
            if T == 7:                                # the first 29 rows only: a ragged last row-group, and rows of 29 floats (unaligned stores)
                rb = K // 32 * lg.BB[t]
                got = bamd.op_mul_mat_batch(t, blocks[:29 * rb], 29, K, X, residual=res[:, :29], impl=2)
                assert_bits(got, want[:, :29] + res[:, :29], "%s T %d, 29 rows" % (key, T))


# ---- shapes, expectation from the restatement ------------------------------------------------------------------------------------------------------
SHAPE_ROWS, SHAPE_T = 72, 65
_shape_ref = {}


def shape_ref(po, t, K, norm):
    """one matrix of 72 rows and 65 token rows per (type, K), and W . Q8_0(x_t) of all of them with and without the RMSNorm prologue: the smaller shapes are the
    first rows and the first tokens of these"""
    if (t, K) not in _shape_ref:
        rng = np.random.default_rng(1013 * t + K)
        W = random_q0_tensor(t, K, SHAPE_ROWS, rng)
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
    rb = K // 32 * lg.BB[t]
    with prefill_switches(bamd, q0=True):
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
    rb = K // 32 * lg.BB[t]
    c, want = shape_ref(po, t, K, False)
    with prefill_switches(bamd, q0=True):
        assert_bits(bamd.op_mul_mat_batch(t, c["W"][:rows * rb], rows, K, c["X"][:T], impl=2), want[:T, :rows], "type %d rows %d" % (t, rows))


@pytest.mark.parametrize("t", TYPES)
def test_mul_mat_batch_43_records(bamd, po, t):
    """K = 11008, the 43 records of Llama-2's ffn_down"""
    K, rows, T = 11008, 8, 3
    rng = np.random.default_rng(43 + t)
    W = random_q0_tensor(t, K, rows, rng)
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    res = rng.standard_normal((T, rows)).astype(np.float32)
    with prefill_switches(bamd, q0=True):
        assert_bits(bamd.op_mul_mat_batch(t, W, rows, K, X, impl=2), ref_batch(t, W, rows, K, X), "K 11008 plain")
        A = np.stack([normed(po, x, w) for x in X])
        assert_bits(bamd.op_mul_mat_batch(t, W, rows, K, X, norm_w=w, eps=EPS, residual=res, impl=2), ref_batch(t, W, rows, K, A) + res, "K 11008 norm + residual")


@pytest.mark.parametrize("t", TYPES)
def test_matrix_core_kernel_equals_integer_dot_kernel(bamd, t):
    K, rows, T = 4096, 256, 65
    rng = np.random.default_rng(4096 + t)
    W = random_q0_tensor(t, K, rows, rng)
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    with prefill_switches(bamd, q0=True):
        before = bamd.prefill_mfma_runs(t)
        a = bamd.op_mul_mat_batch(t, W, rows, K, X, norm_w=w, eps=EPS, impl=2)
        assert bamd.prefill_mfma_runs(t) == before + 1
        b = bamd.op_mul_mat_batch(t, W, rows, K, X, norm_w=w, eps=EPS, impl=0)
        assert bamd.prefill_mfma_runs(t) == before + 1
    assert np.isfinite(b).all() and np.abs(b).max() > 0
    assert_bits(a, b, "impl 2 vs impl 0")


# ---- routing, as the engine issues the launches -------------------------------------------------------------------------------------------------------
def test_seg_q4_0_beside_q8_0_into_one_matrix(bamd, po):
    """Q4_0 | Q8_0 | Q8_0 (q | k | v of a mixed file) into one [T][ldo]: one launch per segment, the fill behind the rows untouched"""
    K, T, rows = 512, 17, [256, 64, 72]
    rng = np.random.default_rng(808)
    types = [Q4_0, Q8_0, Q8_0]
    Ws = [random_q0_tensor(t, K, r, rng) for t, r in zip(types, rows)]
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    A = np.stack([normed(po, x, w) for x in X])
    ldo = sum(rows) + 9
    want = np.concatenate([ref_batch(t, W, r, K, A) for t, W, r in zip(types, Ws, rows)], axis=1)
    with prefill_switches(bamd, q0=True):
        before = runs(bamd, COUNTED)
        got = bamd.op_mul_mat_batch_seg([(t, W, r) for t, W, r in zip(types, Ws, rows)], K, X, ldo, epi=STORE, norm_w=w, eps=EPS, impl=2, fill=FILL)
        after = runs(bamd, COUNTED)
    assert after[Q4_0] == before[Q4_0] + 1 and after[Q8_0] == before[Q8_0] + 2 and after[Q5_0] == before[Q5_0]
    assert_bits(got[:, :sum(rows)], want, "q | k | v")
    assert (got[:, sum(rows):] == FILL).all(), "wrote behind the rows"


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("T", [7, 65])
def test_seg_silu_mul_pair(bamd, po, t, T):
    """gate, then up with h = silu(gate) * up as its in-place epilogue (res == out): two launches of the type, nothing written behind the rows"""
    K, rows = 512, 768
    rng = np.random.default_rng([50, t, T])
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    Wg, Wu = random_q0_tensor(t, K, rows, rng, amp=4.0), random_q0_tensor(t, K, rows, rng, amp=4.0)
    A = np.stack([normed(po, x, w) for x in X])
    g, u = ref_batch(t, Wg, rows, K, A), ref_batch(t, Wu, rows, K, A)
    want = silu_mul(po, g.reshape(-1), u.reshape(-1)).reshape(T, rows)
    with prefill_switches(bamd, q0=True):
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
    rng = np.random.default_rng([60, t])
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    W = random_q0_tensor(t, K, rows, rng)
    res = rng.standard_normal((T, ldo)).astype(np.float32)
    want = ref_batch(t, W, rows, K, X) + res[:, :rows]
    with prefill_switches(bamd, q0=True):
        before = bamd.prefill_mfma_runs(t)
        got = bamd.op_mul_mat_batch_seg([(t, W, rows)], K, X, ldo, epi=ADD, residual=res, impl=2, fill=FILL)
        assert bamd.prefill_mfma_runs(t) == before + 1
    assert_bits(got[:, :rows], want, "add type %d" % t)
    assert (got[:, rows:] == FILL).all(), "wrote behind the rows"


# ---- whole models against the genuine reference's llama_decode ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["tiny_q8_0", "tiny_q4_0", "tiny_q5_0", "8bw_q5_0", "l2w_q5_0", "8b_q4_0"])
def test_whole_model_prompt_on_the_matrix_cores(bamd, cfg, monkeypatch, capfd):
    """the prompt step only (8b_q4_0: the one full-size case, a 128-token prompt = four token tiles of 32)"""
    fx = load_fixture(LEGACY, cfg)
    path = model_for(LEGACY, cfg, fx)
    low = layer_types(path, TYPES)
    assert low, "the fixture holds no Q8_0 / Q4_0 / Q5_0 layer matrix"
    monkeypatch.setenv("BAMD_PREFILL_VERBOSE", "1")
    err, aux, before, after = prompt_step(bamd, path, capfd, COUNTED, dict(q0=True), fam=LEGACY, cfg=cfg, fx=fx)
    assert "prompts run without the matrix-core kernels" not in err, err
    assert aux > 0
    for t in low:
        assert after[t] > before[t], "no matrix-core launch of type %d" % t
    no_tables_with_the_switches_off(bamd, path, "q0")


def test_prompt_through_two_stages_on_the_matrix_cores(bamd):
    """tiny_q5_0 through two layer-split stages (bamd_stage_prefill): the stage path takes the same routing"""
    cfg = "tiny_q5_0"
    low = layer_types(model_for(LEGACY, cfg, load_fixture(LEGACY, cfg)), TYPES)
    assert low, "the fixture holds no Q8_0 / Q4_0 / Q5_0 layer matrix"
    two_stages_on_the_matrix_cores(bamd, LEGACY, cfg, COUNTED, low, dict(q0=True))
