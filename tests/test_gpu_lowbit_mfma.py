"""GPU: the matrix-core prompt mat-muls for Q3_K / Q2_K weights (matmul_mfma2_kernel with the X2LowBit policies, behind set_prefill_lowbit / BAMD_PREFILL_LOWBIT=1; default off).
Every expectation is the genuine reference's stored output (tests/golden/lowbit_kats.npz, tests/golden/lowbit_*.bgld) or the numpy restatement that
tests/test_lowbit_ref.py holds to those (tests/lowbit_ref.py); bit equality throughout.  The switch is set through the setter and restored afterwards; the
launch counters (prefill_mfma_runs) tell the matrix-core kernel from the integer-dot kernel, which gives the same bits."""
import numpy as np
import pytest

import lowbit_ref as lr
from bitcheck import ADD, EPS, FILL, SILU_MUL, assert_bits, normed, silu_mul
from booster_amd.gguf import random_kquant_tensor
from lowbit_ref import all_cases
from mfma_harness import layer_types, no_tables_with_the_switches_off, prefill_switches, prompt_step, runs
from refmodel import LOWBIT, load_fixture, model_for
from test_gpu_segments import Q2, Q3, Q6, batch_inputs, qkv_batch_case, ref_mul_mat
from test_lowbit_ref import stored, stored_case  # noqa: F401  (stored: fixture)

pytestmark = pytest.mark.gpu
TYPES = [Q2, Q3]
COUNTED = [Q2, Q3, Q6]


def test_switch_is_off_by_default_and_refuses(bamd):
    """off: impl 2 declines the types as before and counts nothing; on: it runs and counts"""
    blocks, xs, _ = lr.rand_case(Q3, 256)
    before = runs(bamd, COUNTED)
    with pytest.raises(bamd.BamdError, match="MFMA path: unsupported type/shape"):
        bamd.op_mul_mat_batch(Q3, blocks, lr.ROWS, 256, np.stack(xs), impl=2)
    assert runs(bamd, COUNTED) == before
    with prefill_switches(bamd, lowbit=True):
        bamd.op_mul_mat_batch(Q3, blocks, lr.ROWS, 256, np.stack(xs), impl=2)
    assert runs(bamd, COUNTED)[Q3] == before[Q3] + 1


# ---- the reference's own outputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("T", [2, 7, 64, 512])
def test_mul_mat_batch_kats(bamd, stored, t, T):
    """the stored cases of test_gpu_lowbit_ops.test_mul_mat_batch_kats — K = 256, 1024, 14336, 11008 and the edge matrices — on the matrix-core kernel"""
    rng = np.random.default_rng(T + t)
    with prefill_switches(bamd, lowbit=True):
        for key, blocks, xs, digest, _ in all_cases(t):
            dots, _, _ = stored_case(stored, key, digest)
            K = xs[0].size
            pick = [i % len(xs) for i in range(T)]
            X = np.stack([xs[i] for i in pick])
            res = rng.standard_normal((T, lr.ROWS)).astype(np.float32) if T % 2 else None
            before = bamd.prefill_mfma_runs(t)
            got = bamd.op_mul_mat_batch(t, blocks, lr.ROWS, K, X, residual=res, impl=2)
            assert bamd.prefill_mfma_runs(t) == before + 1
            want = np.stack([dots[i] for i in pick])
            if res is not None:
                want = want + res
            assert_bits(got, want, "%s T %d" % (key, T))
            if T == 7:                                # the first 29 rows only: a ragged last row-group, and rows of 29 floats (the epilogue's element-wise stores)
                rb = K // 256 * lr.BB[t]
                got = bamd.op_mul_mat_batch(t, blocks[:29 * rb], 29, K, X, residual=res[:, :29], impl=2)
                assert_bits(got, want[:, :29], "%s T %d, 29 rows" % (key, T))


# ---- shapes, expectation from the restatement ------------------------------------------------------------------------------------------------------
SHAPE_ROWS, SHAPE_T = 72, 65
_shape_ref = {}


def shape_ref(po, t, K, norm):
    """one matrix of 72 rows and 65 token rows per (type, K), and W . Q8_K(x_t) of all of them with and without the RMSNorm prologue: the smaller shapes are the
    first rows and the first tokens of these"""
    if (t, K) not in _shape_ref:
        rng = np.random.default_rng(1009 * t + K)
        W = random_kquant_tensor(t, K, SHAPE_ROWS, rng)
        X = (rng.standard_normal((SHAPE_T, K)) * 3).astype(np.float32)
        w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
        res = rng.standard_normal((SHAPE_T, SHAPE_ROWS)).astype(np.float32)
        _shape_ref[(t, K)] = dict(W=W, X=X, w=w, res=res)
    c = _shape_ref[(t, K)]
    if norm not in c:
        A = c["X"] if not norm else np.stack([normed(po, x, c["w"]) for x in c["X"]])
        c[norm] = ref_mul_mat(po, t, c["W"], SHAPE_ROWS, K, A)
    return c, c[norm]


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("K", [256, 512, 768])        # one super-block (the ring's prologue only), two, an odd count (the `ci + 1 < nb` tail)
@pytest.mark.parametrize("rows", [8, 24, 72])         # fewer than a 16-row tile, an odd row-group count, a partial second 64-row block
@pytest.mark.parametrize("T", [1, 16, 17, 64, 65])    # the 16- and 64-token tile edges
def test_mul_mat_batch_shapes(bamd, po, t, K, rows, T):
    rb = K // 256 * lr.BB[t]
    with prefill_switches(bamd, lowbit=True):
        for norm in (False, True):
            c, want = shape_ref(po, t, K, norm)
            for with_res in (False, True):
                res = np.ascontiguousarray(c["res"][:T, :rows]) if with_res else None
                got = bamd.op_mul_mat_batch(t, c["W"][:rows * rb], rows, K, c["X"][:T], norm_w=c["w"] if norm else None, eps=EPS, residual=res, impl=2)
                assert_bits(got, want[:T, :rows] + res if with_res else want[:T, :rows], "type %d K %d rows %d T %d norm %d residual %d" % (t, K, rows, T, norm, with_res))


@pytest.mark.parametrize("t", TYPES)
def test_mul_mat_batch_43_super_blocks(bamd, po, t):
    """K = 11008, the 43 super-blocks of Llama-2's ffn_down"""
    K, rows, T = 11008, 8, 3
    rng = np.random.default_rng(43 + t)
    W = random_kquant_tensor(t, K, rows, rng)
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    res = rng.standard_normal((T, rows)).astype(np.float32)
    with prefill_switches(bamd, lowbit=True):
        assert_bits(bamd.op_mul_mat_batch(t, W, rows, K, X, impl=2), ref_mul_mat(po, t, W, rows, K, X), "K 11008 plain")
        A = np.stack([normed(po, x, w) for x in X])
        assert_bits(bamd.op_mul_mat_batch(t, W, rows, K, X, norm_w=w, eps=EPS, residual=res, impl=2), ref_mul_mat(po, t, W, rows, K, A) + res, "K 11008 norm + residual")


@pytest.mark.parametrize("t", TYPES)
def test_matrix_core_kernel_equals_integer_dot_kernel(bamd, t):
    K, rows, T = 4096, 256, 65
    rng = np.random.default_rng(4096 + t)
    W = random_kquant_tensor(t, K, rows, rng)
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    with prefill_switches(bamd, lowbit=True):
        before = bamd.prefill_mfma_runs(t)
        a = bamd.op_mul_mat_batch(t, W, rows, K, X, norm_w=w, eps=EPS, impl=2)
        assert bamd.prefill_mfma_runs(t) == before + 1
        b = bamd.op_mul_mat_batch(t, W, rows, K, X, norm_w=w, eps=EPS, impl=0)
        assert bamd.prefill_mfma_runs(t) == before + 1
    assert np.isfinite(b).all() and np.abs(b).max() > 0
    assert_bits(a, b, "impl 2 vs impl 0")


# ---- routing, as the engine issues the launches -------------------------------------------------------------------------------------------------------
def test_seg_q3_k_beside_q6_k(bamd, po):
    with prefill_switches(bamd, lowbit=True):
        before = runs(bamd, COUNTED)
        qkv_batch_case(bamd, po, Q3, Q6, 17, (2,), "batched QKV, Q3_K | Q6_K on the matrix cores", r0=256, r1=1024)
        after = runs(bamd, COUNTED)
    assert after[Q3] == before[Q3] + 1 and after[Q6] == before[Q6] + 1 and after[Q2] == before[Q2]


def test_seg_q2_k_beside_q3_k_into_one_matrix(bamd, po):
    with prefill_switches(bamd, lowbit=True):
        before = runs(bamd, COUNTED)
        qkv_batch_case(bamd, po, Q2, Q3, 5, (2,), "batched QKV, Q2_K | Q3_K on the matrix cores", r0=256, r1=1024)
        after = runs(bamd, COUNTED)
    assert after[Q2] == before[Q2] + 1 and after[Q3] == before[Q3] + 1


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("T", [7, 65])
def test_seg_silu_mul_pair(bamd, po, t, T):
    """gate, then up with h = silu(gate) * up as its in-place epilogue (res == out): two launches of the type, nothing written behind the rows"""
    K, rows = 512, 768
    rng, X, w = batch_inputs(K, T, 50 + t)
    Wg, Wu = random_kquant_tensor(t, K, rows, rng, amp=4.0), random_kquant_tensor(t, K, rows, rng, amp=4.0)
    A = np.stack([normed(po, x, w) for x in X])
    want = silu_mul(po, ref_mul_mat(po, t, Wg, rows, K, A), ref_mul_mat(po, t, Wu, rows, K, A))
    with prefill_switches(bamd, lowbit=True):
        before = bamd.prefill_mfma_runs(t)
        got = bamd.op_mul_mat_batch_seg([(t, Wg, rows), (t, Wu, rows)], K, X, rows + 64, epi=SILU_MUL, norm_w=w, eps=EPS, impl=2, fill=FILL)
        assert bamd.prefill_mfma_runs(t) == before + 2
    assert_bits(got[:, :rows], want, "silu(gate) * up type %d T %d" % (t, T))
    assert (got[:, rows:] == FILL).all(), "wrote behind the rows"


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("ldo", [832, 835])           # 16-byte stores per lane; rows of a token not 16-byte aligned: element-wise stores
def test_seg_add_with_wide_rows(bamd, po, t, ldo):
    """residual add with ldo > rows: output and residual share the stride, the columns behind the rows stay untouched"""
    K, rows, T = 512, 760, 65
    rng, X, _ = batch_inputs(K, T, 60 + t)
    W = random_kquant_tensor(t, K, rows, rng)
    res = rng.standard_normal((T, ldo)).astype(np.float32)
    want = ref_mul_mat(po, t, W, rows, K, X) + res[:, :rows]
    with prefill_switches(bamd, lowbit=True):
        before = bamd.prefill_mfma_runs(t)
        got = bamd.op_mul_mat_batch_seg([(t, W, rows)], K, X, ldo, epi=ADD, residual=res, impl=2, fill=FILL)
        assert bamd.prefill_mfma_runs(t) == before + 1
    assert_bits(got[:, :rows], want, "add type %d" % t)
    assert (got[:, rows:] == FILL).all(), "wrote behind the rows"


# ---- whole models against the genuine reference's llama_decode ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["tiny_q3_k_m", "tiny_q2_k", "8bw_q2_k_mix"])
def test_whole_model_prompt_on_the_matrix_cores(bamd, cfg, monkeypatch, capfd):
    fx = load_fixture(LOWBIT, cfg)
    path = model_for(LOWBIT, cfg, fx)
    low = layer_types(path, TYPES)
    assert low, "the fixture holds no low-bit layer matrix"
    monkeypatch.setenv("BAMD_PREFILL_VERBOSE", "1")
    err, aux, before, after = prompt_step(bamd, path, capfd, COUNTED, dict(lowbit=True), fam=LOWBIT, cfg=cfg, fx=fx)
    assert "prompts run without the matrix-core kernels" not in err, err
    assert aux > 0
    for t in low:
        assert after[t] > before[t], "no matrix-core launch of type %d" % t
    no_tables_with_the_switches_off(bamd, path, "lowbit")
