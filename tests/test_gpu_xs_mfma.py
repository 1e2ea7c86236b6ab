"""GPU: the matrix-core prompt mat-mul for IQ4_XS weights (booster_amd/csrc/bamd_prefill2_xs.hip: the policy X2IQ4XS of the eight-wave body, behind set_prefill_xs /
BAMD_PREFILL_XS=1; default off).  Every expectation is the genuine reference's stored output (tests/golden/iq4xs_kats.npz, the *iq4xs*.bgld fixtures) or the numpy
restatement that tests/test_iq4xs_ref.py holds to those (iq4xs_ref.mul_mat); bit equality throughout.  The switch is set through its setter and restored
afterwards; the launch counter prefill_mfma_runs(23) tells the matrix-core kernel from the integer-dot kernel.  (This file collects after test_gpu_iq4xs_ops.py
and test_gpu_sweep_iq4xs.py, which assert that counter at 0.)

Tile edges: a workgroup is 64 rows x 64 tokens, a wave 16 rows x 32 tokens, a record group 8 rows, a step half a super-block.  Rows 8 (one record group: the
row tile's second group is the first one again), 24 (a tile and a half) and 72 (a second row block of 8 rows); tokens both sides of the MFMA tile and of the
workgroup; K = 256 (the prologue's loads only), 512, 768 (an odd super-block count: the loop's tail)."""
import contextlib
import os

import numpy as np
import pytest

import iq4xs_ref as xr
from bitcheck import ADD, EPS, FILL, SILU_MUL, STORE, assert_bits, normed, silu_mul
from booster_amd.gguf import random_iq4_xs_tensor, random_kquant_tensor
from mfma_harness import layer_types, prompt_step, runs, two_stages_on_the_matrix_cores
from refmodel import Family, load_fixture, model_for
from test_iq4xs_ref import stored, stored_case  # noqa: F401  (stored: fixture)

pytestmark = pytest.mark.gpu
XS, Q5_K, Q6_K = xr.IQ4_XS, 13, 14
COUNTED = [XS, Q5_K, Q6_K]
IQ4XS = Family("iq4xs", "")


@contextlib.contextmanager
def xs_switch(bamd, on=True):
    """the switch of this family through its setter; on exit it goes back to the process's default (mfma_harness.prefill_switches does not know it)"""
    bamd.set_prefill_xs(on)
    try:
        yield
    finally:
        bamd.set_prefill_xs(os.environ.get("BAMD_PREFILL_XS", "")[:1] == "1")


def ref_batch(po, W, rows, K, A):
    return np.stack([xr.mul_mat(po, W, rows, K, a) for a in A])


def test_switch_is_off_by_default_and_refuses(bamd, po):
    W = random_iq4_xs_tensor(256, xr.ROWS, np.random.default_rng(2))
    X = np.random.default_rng(3).standard_normal((2, 256)).astype(np.float32)
    before = runs(bamd, COUNTED)
    with xs_switch(bamd, False):
        with pytest.raises(bamd.BamdError, match="MFMA path: unsupported type/shape"):
            bamd.op_mul_mat_batch(XS, W, xr.ROWS, 256, X, impl=2)
        assert runs(bamd, COUNTED) == before
        with xs_switch(bamd):
            got = bamd.op_mul_mat_batch(XS, W, xr.ROWS, 256, X, impl=2)
        after = runs(bamd, COUNTED)
    assert after[XS] == before[XS] + 1 and after[Q5_K] == before[Q5_K] and after[Q6_K] == before[Q6_K]
    assert_bits(got, ref_batch(po, W, xr.ROWS, 256, X), "switch on")


# ---- the reference's own outputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [2, 7, 64])
def test_mul_mat_batch_kats(bamd, stored, T):
    """every stored case — K = 256, 768, 4096, 14336, the edge blocks and the pairs case — with token rows cycling through its vectors; a residual at odd T;
    T = 7: also the first 29 rows only (a ragged last row-group, rows of 29 floats: element-wise stores)"""
    rng = np.random.default_rng(T + XS)
    with xs_switch(bamd):
        for key, blocks, xs, digest, _ in xr.all_cases():
            dots, _, _ = stored_case(stored, key, digest)
            K = xs[0].size
            pick = [i % len(xs) for i in range(T)]
            X = np.stack([xs[i] for i in pick])
            want = np.stack([dots[i] for i in pick])
            res = rng.standard_normal((T, xr.ROWS)).astype(np.float32) if T % 2 else None
            before = bamd.prefill_mfma_runs(XS)
            got = bamd.op_mul_mat_batch(XS, blocks, xr.ROWS, K, X, residual=res, impl=2)
            assert bamd.prefill_mfma_runs(XS) == before + 1
            assert_bits(got, want if res is None else want + res, "%s T %d" % (key, T))
            if T == 7:
                got = bamd.op_mul_mat_batch(XS, blocks[:29 * (K // 256) * xr.BB], 29, K, X, residual=res[:, :29], impl=2)
                assert_bits(got, want[:, :29] + res[:, :29], "%s T %d, 29 rows" % (key, T))


# ---- shapes, expectation from the restatement ------------------------------------------------------------------------------------------------------
SHAPE_ROWS, SHAPE_T = 72, 65
_shape_ref = {}


def shape_ref(po, K, norm):
    """one matrix of 72 rows and 65 token rows per K, and W . x_t of all of them with and without the RMSNorm prologue: the smaller shapes are their first rows / tokens"""
    if K not in _shape_ref:
        rng = np.random.default_rng(1013 * (XS + 1) + K)
        W = random_iq4_xs_tensor(K, SHAPE_ROWS, rng)
        X = (rng.standard_normal((SHAPE_T, K)) * 3).astype(np.float32)
        w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
        res = rng.standard_normal((SHAPE_T, SHAPE_ROWS)).astype(np.float32)
        for a in (W, X, w, res):
            a.setflags(write=False)
        _shape_ref[K] = dict(W=W, X=X, w=w, res=res)
    c = _shape_ref[K]
    if norm not in c:
        c[norm] = ref_batch(po, c["W"], SHAPE_ROWS, K, c["X"] if not norm else [normed(po, x, c["w"]) for x in c["X"]])
        assert np.isfinite(c[norm]).all()
        c[norm].setflags(write=False)
    return c, c[norm]


@pytest.mark.parametrize("K", [256, 512, 768])
@pytest.mark.parametrize("rows", [8, 24, 72])
@pytest.mark.parametrize("T", [1, 16, 17, 64, 65])
def test_mul_mat_batch_shapes(bamd, po, K, rows, T):
    with xs_switch(bamd):
        for norm in (False, True):
            c, want = shape_ref(po, K, norm)
            for with_res in (False, True):
                res = np.ascontiguousarray(c["res"][:T, :rows]) if with_res else None
                before = bamd.prefill_mfma_runs(XS)
                got = bamd.op_mul_mat_batch(XS, c["W"][:rows * (K // 256) * xr.BB], rows, K, c["X"][:T], norm_w=c["w"] if norm else None, eps=EPS, residual=res, impl=2)
                assert bamd.prefill_mfma_runs(XS) == before + 1
                assert_bits(got, want[:T, :rows] + res if with_res else want[:T, :rows], "K %d rows %d T %d norm %d residual %d" % (K, rows, T, norm, with_res))


def test_lane_sums_at_the_bound(bamd, po):
    """every block scale -32 (ls = 0), every nibble 0 (value -127), against constant activation rows (every Q8_K byte +-127): |isum_e| = 32 x 32 x 127 x 127 =
    16 516 096, the largest sum the two chained MFMAs ever hold"""
    rows, K = 8, 256
    blk = random_iq4_xs_tensor(K, rows, np.random.default_rng(5)).reshape(rows, xr.BB).copy()
    blk[:, 2:] = 0
    X = np.stack([np.full(K, 3.0, np.float32), np.full(K, -0.25, np.float32)])
    for x in X:
        q8 = po.quantize_q8_K(x)
        assert set(np.abs(xr.ei.q8_fields(q8)[1]).reshape(-1)) == {127}
        assert np.abs(xr.lane_sums(blk.reshape(-1), q8)).min() == 32 * 32 * 127 * 127
    with xs_switch(bamd):
        got = bamd.op_mul_mat_batch(XS, blk.reshape(-1), rows, K, X, impl=2)
    assert_bits(got, ref_batch(po, blk.reshape(-1), rows, K, X), "bound")


def test_matrix_core_kernel_equals_integer_dot_kernel(bamd):
    """beside the reference expectations above, not instead of them"""
    K, rows, T = 4096, 256, 65
    rng = np.random.default_rng(4096 + XS)
    W = random_iq4_xs_tensor(K, rows, rng)
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    with xs_switch(bamd):
        before = bamd.prefill_mfma_runs(XS)
        a = bamd.op_mul_mat_batch(XS, W, rows, K, X, norm_w=w, eps=EPS, impl=2)
        assert bamd.prefill_mfma_runs(XS) == before + 1
        b = bamd.op_mul_mat_batch(XS, W, rows, K, X, norm_w=w, eps=EPS, impl=0)
        assert bamd.prefill_mfma_runs(XS) == before + 1
    assert np.isfinite(b).all() and np.abs(b).max() > 0
    assert_bits(a, b, "impl 2 vs impl 0")


# ---- routing, as the engine issues the launches -------------------------------------------------------------------------------------------------------
def test_seg_qkv_into_one_matrix(bamd, po):
    """the recipe's IQ4_XS | IQ4_XS | Q5_K QKV as the engine merges it: q | k one IQ4_XS matrix, v on the sixteen-wave kernel — two matrix-core launches into one
    [T][ldo], the fill behind the rows untouched"""
    K, T, rqk, rv = 512, 17, 136 + 64, 72
    rng = np.random.default_rng(808 + XS)
    Wqk, Wv = random_iq4_xs_tensor(K, rqk, rng), random_kquant_tensor(Q5_K, K, rv, rng)
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    A = np.stack([normed(po, x, w) for x in X])
    want = np.concatenate([ref_batch(po, Wqk, rqk, K, A), po.mul_mat_q(Q5_K, Wv, rv, K, A, nthreads=8)], axis=1)
    with xs_switch(bamd):
        before = runs(bamd, COUNTED)
        got = bamd.op_mul_mat_batch_seg([(XS, Wqk, rqk), (Q5_K, Wv, rv)], K, X, rqk + rv + 9, epi=STORE, norm_w=w, eps=EPS, impl=2, fill=FILL)
        after = runs(bamd, COUNTED)
    assert after[XS] == before[XS] + 1 and after[Q5_K] == before[Q5_K] + 1 and after[Q6_K] == before[Q6_K]
    assert_bits(got[:, :rqk + rv], want, "q | k | v")
    assert (got[:, rqk + rv:] == FILL).all(), "wrote behind the rows"


@pytest.mark.parametrize("T", [7, 65])
def test_seg_silu_mul_pair(bamd, po, T):
    """gate, then up with h = silu(gate) * up as its in-place epilogue (res == out): two launches, nothing written behind the rows"""
    K, rows = 512, 200
    rng = np.random.default_rng([50, XS, T])
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    Wg, Wu = random_iq4_xs_tensor(K, rows, rng, amp=4.0), random_iq4_xs_tensor(K, rows, rng, amp=4.0)
    A = np.stack([normed(po, x, w) for x in X])
    g, u = ref_batch(po, Wg, rows, K, A), ref_batch(po, Wu, rows, K, A)
    want = silu_mul(po, g.reshape(-1), u.reshape(-1)).reshape(T, rows)
    with xs_switch(bamd):
        before = bamd.prefill_mfma_runs(XS)
        got = bamd.op_mul_mat_batch_seg([(XS, Wg, rows), (XS, Wu, rows)], K, X, rows + 64, epi=SILU_MUL, norm_w=w, eps=EPS, impl=2, fill=FILL)
        assert bamd.prefill_mfma_runs(XS) == before + 2
    assert_bits(got[:, :rows], want, "silu(gate) * up T %d" % T)
    assert (got[:, rows:] == FILL).all(), "wrote behind the rows"


@pytest.mark.parametrize("T", [7, 65])
@pytest.mark.parametrize("ldo", [832, 835])           # 16-byte stores per lane; rows of a token not 16-byte aligned: element-wise stores
def test_seg_add_with_wide_rows(bamd, po, ldo, T):
    """residual add with ldo > rows: output and residual share the stride, the columns behind the rows stay untouched"""
    K, rows = 256, 760
    rng = np.random.default_rng([60, XS])
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    W = random_iq4_xs_tensor(K, rows, rng)
    res = rng.standard_normal((T, ldo)).astype(np.float32)
    want = ref_batch(po, W, rows, K, X) + res[:, :rows]
    with xs_switch(bamd):
        before = bamd.prefill_mfma_runs(XS)
        got = bamd.op_mul_mat_batch_seg([(XS, W, rows)], K, X, ldo, epi=ADD, residual=res, impl=2, fill=FILL)
        assert bamd.prefill_mfma_runs(XS) == before + 1
    assert_bits(got[:, :rows], want, "add")
    assert (got[:, rows:] == FILL).all(), "wrote behind the rows"


# ---- whole models against the genuine reference's llama_decode ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["tiny_iq4xs", "tiny_iq4xs_imatrix_tied", "8bw_iq4xs"])
def test_whole_model_prompt_on_the_matrix_cores(bamd, cfg, monkeypatch, capfd):
    """the prompt step with the switch on: the reference's logits, side tables built, IQ4_XS launches counted, no note about a missing kernel; with the switch
    off a fresh model of the same file builds no tables"""
    fx = load_fixture(IQ4XS, cfg)
    path = model_for(IQ4XS, cfg, fx)
    monkeypatch.setenv("BAMD_PREFILL_VERBOSE", "1")
    assert XS in layer_types(path, [XS])
    with xs_switch(bamd):
        err, aux, before, after = prompt_step(bamd, path, capfd, COUNTED, {}, fam=IQ4XS, cfg=cfg, fx=fx)
    assert "prompts run without the matrix-core kernels" not in err, err
    assert aux > 0
    assert after[XS] > before[XS]
    with xs_switch(bamd, False):
        m = bamd.Model(path)
        try:
            assert m.prefill_aux_bytes() == 0
        finally:
            m.close()


def test_prompt_through_two_stages_on_the_matrix_cores(bamd):
    """tiny_iq4xs through two layer-split stages (bamd_stage_prefill): the stage path takes the same routing"""
    with xs_switch(bamd):
        two_stages_on_the_matrix_cores(bamd, IQ4XS, "tiny_iq4xs", COUNTED, (XS,), {})
