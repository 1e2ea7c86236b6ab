"""GPU: the matrix-core prompt mat-muls at the edges of their shared epilogue (bamd_prefill2.hip: the hsum tree and the row-of-four store that close the eight-wave body
matmul_mfma2_kernel and the sixteen-wave matmul_mfma3_q4k_kernel) and, for Q6_K, at the edges of the eight-wave body that tests/test_gpu_lowbit_mfma.py
pins for its Q3_K / Q2_K instances: one, two and an odd number of super-blocks, row counts under a 16-row tile / with an odd row-group count / with a ragged last
group of four / into a second 64-row block, the 16- and 64-token tile edges, 16-byte and element-wise stores, the in-place silu(gate) * up.
Every expectation is the oracle's mul_mat_q of the oracle's normalised activations; bit equality throughout, impl 2, and the launch counter of the type tells
that the matrix-core kernel ran."""
import numpy as np
import pytest

from booster_amd.gguf import random_kquant_tensor
from bitcheck import ADD, EPS, FILL, SILU_MUL, assert_bits, normed, silu_mul
from test_gpu_segments import Q4, Q5, Q6, batch_inputs, ref_mul_mat, row_bytes

pytestmark = pytest.mark.gpu
SHAPE_ROWS, SHAPE_T = 72, 65
_shape_ref = {}


def shape_ref(po, t, K, norm):
    """one matrix of 72 rows and 65 token rows per (type, K), and W . Q8_K(x_t) of all of them with and without the RMSNorm prologue: the smaller shapes are the
    first rows and the first tokens of these"""
    if (t, K) not in _shape_ref:
        rng = np.random.default_rng(2003 * t + K)
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


# Q6_K: fewer rows than a 16-row tile, an odd row-group count, a ragged last group of four, a partial second 64-row block; Q4_K / Q5_K: the ragged group
@pytest.mark.parametrize("t,rows", [(Q6, 8), (Q6, 24), (Q6, 29), (Q6, 72), (Q4, 29), (Q5, 29)])
@pytest.mark.parametrize("K", [256, 512, 768])        # one super-block (the ring's prologue only), two, an odd count (the `ci + 1 < nb` tail)
@pytest.mark.parametrize("T", [1, 16, 17, 64, 65])    # the 16- and 64-token tile edges
def test_mul_mat_batch_shapes(bamd, po, t, rows, K, T):
    rb = row_bytes(t, K)
    for norm in (False, True):
        c, want = shape_ref(po, t, K, norm)
        for with_res in (False, True):
            res = np.ascontiguousarray(c["res"][:T, :rows]) if with_res else None
            before = bamd.prefill_mfma_runs(t)
            got = bamd.op_mul_mat_batch(t, c["W"][:rows * rb], rows, K, c["X"][:T], norm_w=c["w"] if norm else None, eps=EPS, residual=res, impl=2)
            assert bamd.prefill_mfma_runs(t) == before + 1
            assert_bits(got, want[:T, :rows] + res if with_res else want[:T, :rows], "type %d K %d rows %d T %d norm %d residual %d" % (t, K, rows, T, norm, with_res))


@pytest.mark.parametrize("t", [Q6, Q4, Q5])
# 16-byte stores per lane; rows of a token not 16-byte aligned: element-wise stores; a ragged last group of four behind full ones with aligned rows: both in one launch
@pytest.mark.parametrize("rows,ldo", [(760, 832), (760, 835), (758, 832)])
def test_seg_add_with_wide_rows(bamd, po, t, rows, ldo):
    """residual add with ldo > rows: output and residual share the stride, the columns behind the rows stay untouched"""
    K, T = 512, 65
    rng, X, _ = batch_inputs(K, T, 70 + t)
    W = random_kquant_tensor(t, K, rows, rng)
    res = rng.standard_normal((T, ldo)).astype(np.float32)
    want = ref_mul_mat(po, t, W, rows, K, X) + res[:, :rows]
    before = bamd.prefill_mfma_runs(t)
    got = bamd.op_mul_mat_batch_seg([(t, W, rows)], K, X, ldo, epi=ADD, residual=res, impl=2, fill=FILL)
    assert bamd.prefill_mfma_runs(t) == before + 1
    assert_bits(got[:, :rows], want, "add type %d rows %d ldo %d" % (t, rows, ldo))
    assert (got[:, rows:] == FILL).all(), "wrote behind the rows"


@pytest.mark.parametrize("T", [7, 65])
def test_seg_silu_mul_pair_q6_k(bamd, po, T):
    """gate, then up with h = silu(gate) * up as its in-place epilogue (res == out): two launches, nothing written behind the rows"""
    t, K, rows = Q6, 512, 768
    rng, X, w = batch_inputs(K, T, 80 + t)
    Wg, Wu = random_kquant_tensor(t, K, rows, rng, amp=4.0), random_kquant_tensor(t, K, rows, rng, amp=4.0)
    A = np.stack([normed(po, x, w) for x in X])
    want = silu_mul(po, ref_mul_mat(po, t, Wg, rows, K, A), ref_mul_mat(po, t, Wu, rows, K, A))
    before = bamd.prefill_mfma_runs(t)
    got = bamd.op_mul_mat_batch_seg([(t, Wg, rows), (t, Wu, rows)], K, X, rows + 64, epi=SILU_MUL, norm_w=w, eps=EPS, impl=2, fill=FILL)
    assert bamd.prefill_mfma_runs(t) == before + 2
    assert_bits(got[:, :rows], want, "silu(gate) * up Q6_K T %d" % T)
    assert (got[:, rows:] == FILL).all(), "wrote behind the rows"
