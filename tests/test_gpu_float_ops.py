"""GPU: the F32 / F16 / BF16 kernels through the C-ABI (include/bamd.h bamd_op_*) against the genuine reference's stored outputs (tests/golden/float_kats.npz)
and, at the shapes the stored cases do not have, against the numpy restatement that tests/test_float_ref.py holds to those outputs (tests/float_ref.py).
Bit equality throughout; every expectation is finite.  Weights travel as the row-major bytes of the GGUF tensor."""
import functools

import numpy as np
import pytest

import float_ref as fr
from bitcheck import assert_bits, bits, EPS, normed, silu_mul
from booster_amd.gguf import random_float_tensor, random_kquant_tensor
from test_float_ref import stored  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
TYPES = list(fr.TYPES)


# ---- the reference's own outputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES)
def test_mul_mat_vec_kats(bamd, stored, t):
    """every stored case — K = 256, 512, 1024, 4096 and the edge matrix x edge vectors (subnormal f16 weights, +-0, the largest f16, f32 subnormal activations,
    products and partial sums below 2^-126)"""
    for key, raw, xs, digest in fr.all_cases(t):
        assert str(stored[key + "_inputs_sha256"]) == digest
        want = stored[key + ("_dots" if t == fr.BF16 else "_sgemm1")]
        K = xs[0].size
        for i, x in enumerate(xs):
            assert_bits(bamd.op_mul_mat_vec(t, raw, fr.ROWS, K, x), want[i], "%s vector %d" % (key, i))


def test_act_bf16_kats(bamd, stored):
    """ggml_fp32_to_bf16_row's own bytes: ties of both parities, f32 subnormals (kept), tiny values"""
    for key, raw, xs, _ in fr.all_cases(fr.BF16):
        for i, x in enumerate(xs):
            assert np.array_equal(bamd.op_act_bf16(x), stored[key + "_act"][i]), "%s vector %d" % (key, i)


@pytest.mark.parametrize("K", [256, 4096])
def test_act_bf16_with_rmsnorm(bamd, po, K):
    rng = np.random.default_rng(K)
    x = (rng.standard_normal(K) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    assert np.array_equal(bamd.op_act_bf16(x, norm_w=w, eps=EPS), fr.bf16_bits(normed(po, x, w)))


@pytest.mark.parametrize("t", TYPES)
def test_get_row(bamd, stored, t):
    """embedding rows: the type's to_float (BF16: bits << 16), first, middle and last row of every stored matrix, every row of the edge matrix"""
    for key, raw, xs, _ in fr.all_cases(t):
        K = xs[0].size
        rows = range(fr.ROWS) if key.endswith("_edge") else fr.DEQ_ROWS
        for i, r in enumerate(rows):
            got = bamd.op_get_row(t, raw, fr.ROWS, K, r)
            assert np.array_equal(bits(got), bits(stored[key + "_to_float"][i])), "%s row %d" % (key, r)


# ---- mat-vec shapes against the restatement ---------------------------------------------------------------------------------------------------------
ROWS_BIG = 4090                    # 512 row-groups, the last one ragged: more units than workgroups, a unit with one row-group only


@functools.lru_cache(maxsize=None)
def shape_case(t, K):
    """one 4090-row matrix, one vector, one norm weight, one residual per (type, K) and the restatement's answers, shared by the tests"""
    rng = np.random.default_rng(9100 * (t + 1) + K)
    W = random_float_tensor(t, K, ROWS_BIG, rng, amp=4.0)
    x = (rng.standard_normal(K) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    res = rng.standard_normal(ROWS_BIG).astype(np.float32)
    for a in (W, x, w, res):
        a.setflags(write=False)
    return W, x, w, res


@functools.lru_cache(maxsize=None)
def shape_want(t, K, rows, norm_key):
    W, x, w, _ = shape_case(t, K)
    a = x if norm_key is None else np.frombuffer(norm_key, np.float32)
    return fr.mul_mat(t, W, rows, K, a)


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("K", [256, 512, 4096, 14336])
def test_mul_mat_vec_shapes(bamd, po, t, K):
    """rows 8, 32 and 4090 (ragged); plain and RMSNorm prologue; with and without residual"""
    W, x, w, res = shape_case(t, K)
    rb = K * fr.ESIZE[t]
    a = normed(po, x, w)
    for rows in (8, 32, ROWS_BIG):
        want_plain = shape_want(t, K, rows, None)
        want_norm = shape_want(t, K, rows, a.tobytes())
        what = "type %d K %d rows %d" % (t, K, rows)
        assert_bits(bamd.op_mul_mat_vec(t, W[:rows * rb], rows, K, x), want_plain, what)
        assert_bits(bamd.op_mul_mat_vec(t, W[:rows * rb], rows, K, x, residual=res[:rows]), want_plain + res[:rows], what + " + residual")
        assert_bits(bamd.op_mul_mat_vec(t, W[:rows * rb], rows, K, x, norm_w=w, eps=EPS), want_norm, what + " norm")
        assert_bits(bamd.op_mul_mat_vec(t, W[:rows * rb], rows, K, x, norm_w=w, eps=EPS, residual=res[:rows]), want_norm + res[:rows], what + " norm + residual")


@pytest.mark.parametrize("t", TYPES)
def test_mul_mat_vec_longest_row(bamd, t):
    """K = 28672 (the 70B ffn_down): the whole activation vector in LDS"""
    K, rows = 28672, 24
    rng = np.random.default_rng(5 + t)
    W = random_float_tensor(t, K, rows, rng, amp=4.0)
    x = rng.standard_normal(K).astype(np.float32)
    assert_bits(bamd.op_mul_mat_vec(t, W, rows, K, x), fr.mul_mat(t, W, rows, K, x), "type %d K %d" % (t, K))


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("K,rows", [(512, 24), (4096, 1792)])
def test_ffn_gate_up(bamd, po, t, K, rows):
    rng = np.random.default_rng(5 * t + K + rows)
    Wg = random_float_tensor(t, K, rows, rng, amp=4.0)
    Wu = random_float_tensor(t, K, rows, rng, amp=4.0)
    x = (rng.standard_normal(K) * 2).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    a = normed(po, x, w)
    want = silu_mul(po, fr.mul_mat(t, Wg, rows, K, a), fr.mul_mat(t, Wu, rows, K, a))
    assert_bits(bamd.op_ffn_gate_up(t, Wg, Wu, rows, K, x, norm_w=w, eps=EPS), want, "ffn gate/up type %d K %d rows %d" % (t, K, rows))


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("E,H,Hkv", [(512, 8, 2), (4096, 32, 8)])
def test_fused_qkv(bamd, po, t, E, H, Hkv):
    """three segments of one type behind one RMSNorm prologue: rows 512 | 128 | 128 and 4096 | 1024 | 1024"""
    rng = np.random.default_rng(31 + t + E)
    rows = [E, E // H * Hkv, E // H * Hkv]
    Ws = [random_float_tensor(t, E, r, rng, amp=2.0) for r in rows]
    x = (rng.standard_normal(E) * 2).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(E)).astype(np.float32)
    a = normed(po, x, w)
    want = np.concatenate([fr.mul_mat(t, W, r, E, a) for W, r in zip(Ws, rows)])
    assert_bits(bamd.op_fused_qkv([(t, W, r) for W, r in zip(Ws, rows)], E, x, w, eps=EPS), want, "fused QKV type %d E %d" % (t, E))


def test_fused_qkv_f32_beside_f16(bamd, po):
    """F32 and F16 segments share the f32 activation form: one launch"""
    E, rows = 512, [64, 24, 16]
    rng = np.random.default_rng(4)
    ts = [fr.F16, fr.F32, fr.F16]
    Ws = [random_float_tensor(t, E, r, rng) for t, r in zip(ts, rows)]
    x = rng.standard_normal(E).astype(np.float32); w = (1 + 0.1 * rng.standard_normal(E)).astype(np.float32)
    a = normed(po, x, w)
    want = np.concatenate([fr.mul_mat(t, W, r, E, a) for t, W, r in zip(ts, Ws, rows)])
    assert_bits(bamd.op_fused_qkv(list(zip(ts, Ws, rows)), E, x, w, eps=EPS), want, "F16 | F32 | F16")


@pytest.mark.parametrize("t", TYPES)
def test_argmax_tie_returns_the_lower_row(bamd, po, t):
    """the lm_head launch with its arg-max epilogue at 32 001 rows x K 512, the largest logit tied between two rows of different workgroups"""
    K, rows = 512, 32001
    rng = np.random.default_rng(60 + t)
    W = random_float_tensor(t, K, rows, rng, amp=4.0).reshape(rows, -1).copy()
    x = (rng.standard_normal(K) * 2).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    a = normed(po, x, w)
    y0 = fr.mul_mat(t, W.reshape(-1), rows, K, a)
    tied = [20011, 31999]
    top, bottom = int(np.argmax(y0)), int(np.argmin(y0))
    best = W[top].copy()
    W[top] = W[bottom]
    W[tied] = best
    want = fr.mul_mat(t, W.reshape(-1), rows, K, a)
    assert np.flatnonzero(want == want.max()).tolist() == tied
    got, row = bamd.op_mul_mat_vec_argmax(t, W.reshape(-1), rows, K, x, norm_w=w, eps=EPS)
    assert_bits(got, want, "lm_head logits")
    assert row == tied[0]


# ---- prompt evaluation: the batched kernels give the bits of the mat-vec path -----------------------------------------------------------------------
BATCH_T = (2, 5, 17, 65)


@pytest.mark.parametrize("t", TYPES)
def test_mul_mat_batch_equals_mat_vec(bamd, t):
    """T = 2, 5, 17, 65 tokens (ragged token tiles) x rows 13 (a padded row-group) and 64, all three epilogues: each equals T calls of the mat-vec op"""
    K = 512
    rng = np.random.default_rng(77 * (t + 1))
    rows = [64, 16, 16]
    Ws = [random_float_tensor(t, K, r, rng, amp=4.0) for r in rows]
    rb = K * fr.ESIZE[t]
    Tmax = max(BATCH_T)
    X = (rng.standard_normal((Tmax, K)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    res = rng.standard_normal((Tmax, 64)).astype(np.float32)
    segs = [(t, W, r) for W, r in zip(Ws, rows)]
    # T calls of the mat-vec ops, once
    mv_add = {r: np.stack([bamd.op_mul_mat_vec(t, Ws[0][:r * rb], r, K, X[i], residual=res[i, :r]) for i in range(Tmax)]) for r in (13, 64)}
    mv_norm = np.stack([bamd.op_mul_mat_vec(t, Ws[0], 64, K, X[i], norm_w=w, eps=EPS) for i in range(Tmax)])
    mv_qkv = np.stack([bamd.op_fused_qkv(segs, K, X[i], w, eps=EPS) for i in range(Tmax)])
    mv_silu = np.stack([bamd.op_ffn_gate_up(t, Ws[1], Ws[2], 16, K, X[i], norm_w=w, eps=EPS) for i in range(Tmax)])
    for a in (mv_add[13], mv_add[64], mv_norm, mv_qkv, mv_silu):
        assert np.isfinite(a).all()
    ldo = sum(rows) + 8
    for T in BATCH_T:
        what = "type %d T %d" % (t, T)
        for r in (13, 64):
            assert_bits(bamd.op_mul_mat_batch(t, Ws[0][:r * rb], r, K, X[:T], residual=res[:T, :r], impl=0), mv_add[r][:T], what + " rows %d + residual" % r)
        assert_bits(bamd.op_mul_mat_batch(t, Ws[0], 64, K, X[:T], norm_w=w, eps=EPS, impl=0), mv_norm[:T], what + " norm")
        got = bamd.op_mul_mat_batch_seg(segs, K, X[:T], ldo, epi=0, norm_w=w, eps=EPS, fill=-7.0)
        want = np.full((T, ldo), -7.0, np.float32); want[:, :sum(rows)] = mv_qkv[:T]
        assert_bits(got, want, what + " q | k | v")
        r1 = np.zeros((T, 64), np.float32); r1[:] = res[:T]
        assert_bits(bamd.op_mul_mat_batch_seg([segs[0]], K, X[:T], 64, epi=1, residual=r1), mv_add[64][:T], what + " one segment + residual")
        assert_bits(bamd.op_mul_mat_batch_seg([segs[1], segs[2]], K, X[:T], 16, epi=2, norm_w=w, eps=EPS), mv_silu[:T], what + " gate / up")


@pytest.mark.parametrize("t", TYPES)
def test_mul_mat_batch_long_rows(bamd, t):
    """K = 14336 (the 8B ffn_down) at T = 5: equal to the mat-vec op"""
    K, rows, T = 14336, 24, 5
    rng = np.random.default_rng(13 + t)
    W = random_float_tensor(t, K, rows, rng, amp=4.0)
    X = rng.standard_normal((T, K)).astype(np.float32)
    want = np.stack([bamd.op_mul_mat_vec(t, W, rows, K, X[i]) for i in range(T)])
    assert_bits(bamd.op_mul_mat_batch(t, W, rows, K, X, impl=0), want, "type %d" % t)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_fused_launch_refuses_mixed_activation_forms(bamd):
    """F16 beside Q4_K (Q8_K activations), F16 beside BF16 (bf16 activations): an error in words, never a run with the wrong form"""
    rng = np.random.default_rng(3)
    E = 512
    f16 = (fr.F16, random_float_tensor(fr.F16, E, 64, rng), 64)
    q4k = (12, random_kquant_tensor(12, E, 64, rng), 64)
    b16 = (fr.BF16, random_float_tensor(fr.BF16, E, 64, rng), 64)
    x = rng.standard_normal(E).astype(np.float32); w = np.ones(E, np.float32)
    for s in ([f16, q4k], [q4k, f16], [f16, b16], [b16, f16]):
        with pytest.raises(bamd.BamdError, match="type without a kernel"):
            bamd.op_fused_qkv(s, E, x, w, eps=EPS)
        with pytest.raises(bamd.BamdError, match="different activation forms"):
            bamd.op_mul_mat_batch_seg(s, E, np.stack([x, x]), 136, epi=0, norm_w=w, eps=EPS)


@pytest.mark.parametrize("t", TYPES)
def test_matrix_core_path_refuses_the_type(bamd, t):
    W = random_float_tensor(t, 256, 32, np.random.default_rng(1))
    x = np.ones((2, 256), np.float32)
    for impl in (1, 2):
        with pytest.raises(bamd.BamdError, match="F32 / F16 / BF16"):
            bamd.op_mul_mat_batch(t, W, 32, 256, x, impl=impl)


def test_the_k_quant_launcher_still_refuses_f16(bamd):
    """bamd_launch_matvec itself (the launcher tests/test_launch_selection.py pins) keeps refusing type 1: the float family is dispatched in front of it"""
    assert bamd.trace_matvec([(1, 6144)], 4096, 1, 0) is None
    assert bamd.trace_matvec([(30, 4096)], 4096, 0, 1) is None
