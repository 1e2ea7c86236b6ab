"""GPU: the Q3_K / Q2_K kernels through the C-ABI (include/bamd.h bamd_op_*) against the genuine reference's stored outputs (tests/golden/lowbit_kats.npz) and,
at the shapes the stored cases do not have, against the numpy restatement that tests/test_lowbit_ref.py holds to those outputs (tests/lowbit_ref.py).
Bit equality throughout; every expectation is finite (the finiteness rule of tests/edge_inputs.py)."""
import numpy as np
import pytest

import lowbit_ref as lr
from bitcheck import assert_bits, bits, EPS, normed, silu_mul
from booster_amd.gguf import random_kquant_tensor
from lowbit_ref import all_cases
from test_lowbit_ref import stored_case, stored  # noqa: F401  (stored: fixture)

pytestmark = pytest.mark.gpu
TYPES = [lr.Q2_K, lr.Q3_K]


# ---- the reference's own outputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("mode", [0, 1, 2, 16])
def test_mul_mat_vec_kats(bamd, stored, t, mode):
    """every stored case — K = 256, 1024, 14336, 11008 (43 super-blocks: uneven split-K) and the edge blocks — in every launch mode (16: generic kernels forced)"""
    for key, blocks, xs, digest, _ in all_cases(t):
        dots, _, _ = stored_case(stored, key, digest)
        K = xs[0].size
        for i, x in enumerate(xs):
            got = bamd.op_mul_mat_vec(t, blocks, lr.ROWS, K, x, mode=mode)
            assert_bits(got, dots[i], "%s vector %d mode %d" % (key, i, mode))


@pytest.mark.parametrize("t", TYPES)
def test_mul_mat_vec_kats_residual_and_ragged_rows(bamd, stored, t):
    """the stored dots with a residual add, and the first 29 rows only (a ragged last row-group)"""
    rng = np.random.default_rng(5 + t)
    for key, blocks, xs, digest, _ in all_cases(t):
        dots, _, _ = stored_case(stored, key, digest)
        K = xs[0].size
        rb = K // 256 * lr.BB[t]
        res = rng.standard_normal(lr.ROWS).astype(np.float32)
        for mode in (0, 1, 2):
            assert_bits(bamd.op_mul_mat_vec(t, blocks, lr.ROWS, K, xs[1], residual=res, mode=mode), dots[1] + res, key + " + residual")
            assert_bits(bamd.op_mul_mat_vec(t, blocks[:29 * rb], 29, K, xs[2], mode=mode), dots[2][:29], key + " 29 rows")


@pytest.mark.parametrize("t", TYPES)
def test_get_row_kats(bamd, stored, t):
    """embedding rows (dequantize_row_q3_K / _q2_K): first, middle and last row of every stored matrix, every row of the edge matrix"""
    for key, blocks, xs, digest, deq_rows in all_cases(t):
        _, _, deq = stored_case(stored, key, digest)
        K = xs[0].size
        for i, r in enumerate(deq_rows):
            assert_bits(bamd.op_get_row(t, blocks, lr.ROWS, K, r), deq[i], "%s get_row %d" % (key, r))


@pytest.mark.parametrize("t", TYPES)
def test_ffn_gate_up_kats(bamd, po, stored, t):
    """gate = rows 0-15, up = rows 16-31 of the stored matrices.  The launch always has an RMSNorm prologue, so its activations are the normalised stored vector
    and the expectation is silu(gate) * up of the restatement's dots on that vector; the restatement is anchored to the stored dots first."""
    for key, blocks, xs, digest, _ in all_cases(t):
        dots, _, _ = stored_case(stored, key, digest)
        K = xs[0].size
        rb = K // 256 * lr.BB[t]
        # the stored dots themselves through the restatement (the same check as tests/test_lowbit_ref.py, here as the anchor of this test)
        assert np.array_equal(bits(lr.mul_mat(po, t, blocks, lr.ROWS, K, xs[1])), bits(dots[1]))
        w = np.ones(K, np.float32)
        a = normed(po, xs[1], w)
        y = lr.mul_mat(po, t, blocks, lr.ROWS, K, a)
        got = bamd.op_ffn_gate_up(t, blocks[:16 * rb], blocks[16 * rb:], 16, K, xs[1], norm_w=w, eps=EPS)
        assert_bits(got, silu_mul(po, y[:16], y[16:]), key + " gate/up")


# ---- every kernel family, expectation from the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("K,rows", [(256, 8), (768, 13), (2048, 4104), (4096, 512), (4096, 510), (8192, 24), (8192, 2056), (14336, 64), (14336, 2060),
                                    (11008, 4096), (11008, 20), (28672, 24), (28672, 2056)])
def test_mul_mat_vec_shapes(bamd, po, t, K, rows):
    """mode A rings of depth 8 / 4 / 2 / 1, split-K with 1, 2, 4, 7 records per wave, the uneven split of 43 super-blocks, K = 28672 (112 super-blocks: one wave per
    row-group); plain and RMSNorm prologue, with and without residual, ragged last row-groups"""
    rng = np.random.default_rng(1000 * t + K + rows)
    W = random_kquant_tensor(t, K, rows, rng)
    x = (rng.standard_normal(K) * 3).astype(np.float32)
    res = rng.standard_normal(rows).astype(np.float32) if rows % 16 in (8, 12, 13, 14) else None
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32) if rows % 3 == 0 or K == 4096 else None
    a = x if w is None else normed(po, x, w)
    want = lr.mul_mat(po, t, W, rows, K, a)
    if res is not None:
        want = want + res
    for mode in (0, 1, 2):
        got = bamd.op_mul_mat_vec(t, W, rows, K, x, norm_w=w, eps=EPS, residual=res, mode=mode)
        assert_bits(got, want, "mul_mat_vec type %d K %d rows %d mode %d" % (t, K, rows, mode))


@pytest.mark.parametrize("t", TYPES)
def test_fused_qkv_and_wo_shapes(bamd, po, t):
    """the 8B launches: RMSNorm + store over 6144 rows at K = 4096 (three row-groups per workgroup), plain + residual over 4096 rows at K = 4096 (wo) and at
    K = 14336 (ffn_down)"""
    rng = np.random.default_rng(31 + t)
    for K, rows, norm in ((4096, 6144, True), (4096, 4096, False), (14336, 4096, False)):
        W = random_kquant_tensor(t, K, rows, rng)
        x = (rng.standard_normal(K) * 2).astype(np.float32)
        w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32) if norm else None
        res = None if norm else rng.standard_normal(rows).astype(np.float32)
        want = lr.mul_mat(po, t, W, rows, K, x if w is None else normed(po, x, w))
        if res is not None:
            want = want + res
        for mode in (0, 1, 2):
            got = bamd.op_mul_mat_vec(t, W, rows, K, x, norm_w=w, eps=EPS, residual=res, mode=mode)
            assert_bits(got, want, "type %d K %d rows %d mode %d" % (t, K, rows, mode))


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("K,mode", [(4096, 0), (4096, 16), (1024, 0)])
def test_argmax(bamd, po, t, K, mode):
    """the lm_head launch with its greedy arg-max epilogue, the largest logit tied over three workgroups: logits and the lowest tied row"""
    rows = 4096
    rng = np.random.default_rng(60 + t + K + mode)
    W = random_kquant_tensor(t, K, rows, rng).reshape(rows, -1)
    x = (rng.standard_normal(K) * 2).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    a = normed(po, x, w)
    y0 = lr.mul_mat(po, t, W.reshape(-1), rows, K, a)
    grid = min(256, rows // 8)
    tied = [8 * (grid - 1) + 5, 8 * grid + 2, 8 * grid + 6, 8 * (grid + 44) + 1]
    top, bottom = int(np.argmax(y0)), int(np.argmin(y0))
    best = W[top].copy()
    W[top] = W[bottom]
    W[tied] = best
    want = lr.mul_mat(po, t, W.reshape(-1), rows, K, a)
    assert np.flatnonzero(want == want.max()).tolist() == tied
    got, row = bamd.op_mul_mat_vec_argmax(t, W.reshape(-1), rows, K, x, norm_w=w, eps=EPS, mode=mode)
    assert_bits(got, want, "lm_head logits")
    assert row == int(np.argmax(want)) == tied[0]


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("K,rows", [(512, 768), (4096, 1024), (4096, 14336), (8192, 28672), (2816, 40)])   # 14336 / 28672 rows on 256 CUs: seven / fourteen row-group pairs per workgroup
def test_ffn_gate_up_shapes(bamd, po, t, K, rows):
    rng = np.random.default_rng(5 * t + K)
    Wg = random_kquant_tensor(t, K, rows, rng, amp=4.0)
    Wu = random_kquant_tensor(t, K, rows, rng, amp=4.0)
    x = (rng.standard_normal(K) * 2).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    a = normed(po, x, w)
    want = silu_mul(po, lr.mul_mat(po, t, Wg, rows, K, a), lr.mul_mat(po, t, Wu, rows, K, a))
    got = bamd.op_ffn_gate_up(t, Wg, Wu, rows, K, x, norm_w=w, eps=EPS)
    assert_bits(got, want, "ffn gate/up type %d K %d rows %d" % (t, K, rows))


# ---- prompt evaluation ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("T", [2, 7, 64, 512])
def test_mul_mat_batch_kats(bamd, po, stored, t, T):
    """the integer-dot batched kernel: token rows cycle through the stored activation vectors (expectation = the stored dots); ragged token tiles; a residual at odd T"""
    rng = np.random.default_rng(T + t)
    for key, blocks, xs, digest, _ in all_cases(t):
        dots, _, _ = stored_case(stored, key, digest)
        K = xs[0].size
        pick = [i % len(xs) for i in range(T)]
        X = np.stack([xs[i] for i in pick])
        res = rng.standard_normal((T, lr.ROWS)).astype(np.float32) if T % 2 else None
        got = bamd.op_mul_mat_batch(t, blocks, lr.ROWS, K, X, residual=res, impl=0)
        want = np.stack([dots[i] for i in pick])
        if res is not None:
            want = want + res
        assert_bits(got, want, "%s T %d" % (key, T))


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("K,rows,T", [(4096, 520, 9), (28672, 16, 5), (2816, 24, 3)])   # eight-token tiles; four-token tiles (K > 17920); ring depth 1 (11 super-blocks)
def test_mul_mat_batch_shapes(bamd, po, t, K, rows, T):
    rng = np.random.default_rng(77 * t + K + T)
    W = random_kquant_tensor(t, K, rows, rng)
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    got = bamd.op_mul_mat_batch(t, W, rows, K, X, norm_w=w, eps=EPS, impl=0)
    for i in range(T):
        assert_bits(got[i], lr.mul_mat(po, t, W, rows, K, normed(po, X[i], w)), "batch K %d token %d" % (K, i))


@pytest.mark.parametrize("t", TYPES)
def test_matrix_core_path_refuses_the_type(bamd, stored, t):
    """the matrix-core prefill kernels have no Q2_K / Q3_K: asking for them is an error, never wrong numbers.  The matrix-core implementation is impl 2 of
    bamd_op_mul_mat_batch (impl 1 and 3 were earlier generations, removed: any impl but 2 is the integer-dot kernel), so the error is asserted on impl 2 and
    impl 1 is asserted to give the reference's bits like impl 0"""
    blocks, xs, digest = lr.rand_case(t, 1024)
    dots, _, _ = stored_case(stored, "%s_K1024" % lr.NAME[t], digest)
    with pytest.raises(bamd.BamdError, match="MFMA path: unsupported type/shape"):
        bamd.op_mul_mat_batch(t, blocks, lr.ROWS, 1024, np.stack(xs), impl=2)
    assert_bits(bamd.op_mul_mat_batch(t, blocks, lr.ROWS, 1024, np.stack(xs), impl=1), dots, "impl 1")
