"""GPU: the Q8_0 / Q4_0 / Q5_0 kernels through the C-ABI (include/bamd.h bamd_op_*) against the genuine reference's stored outputs (tests/golden/legacy_kats.npz)
and, at the shapes the stored cases do not have, against the numpy restatement that tests/test_legacy_ref.py holds to those outputs (tests/legacy_ref.py).
Bit equality throughout; every expectation is finite."""
import functools
import hashlib

import numpy as np
import pytest

import legacy_ref as lg
from bitcheck import assert_bits, EPS, normed, silu_mul
from booster_amd.gguf import random_q0_tensor
from legacy_ref import all_cases
from test_legacy_ref import stored_case, stored  # noqa: F401  (stored: fixture)

pytestmark = pytest.mark.gpu
TYPES = list(lg.TYPES)
MODES = (0, 1, 2)                  # the launcher's choice, one wave per row-group, split-K (no fast-family instances exist for these types)


@functools.lru_cache(maxsize=None)
def shape_case(t, K):
    """one 32-row matrix, one vector, one norm weight and one residual per (type, K), shared by the tests; rows 8 and 13 are its leading rows"""
    rng = np.random.default_rng(9000 * t + K)
    W = random_q0_tensor(t, K, 32, rng)
    x = (rng.standard_normal(K) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    res = rng.standard_normal(32).astype(np.float32)
    for a in (W, x, w, res):
        a.setflags(write=False)
    return W, x, w, res


# ---- the activation quantiser ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [256, 4096])
@pytest.mark.parametrize("norm", [False, True])
def test_quantize_q8_0(bamd, po, K, norm):
    rng = np.random.default_rng(K + norm)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32) if norm else None
    for s in lg.SCALES:
        x = (rng.standard_normal(K) * s).astype(np.float32)
        got = bamd.op_quantize_q8_0(x, norm_w=w, eps=EPS)
        want = lg.quantize_row_q8_0(x if w is None else normed(po, x, w))
        assert np.array_equal(got, want), "Q8_0 bytes, K %d scale %g norm %d: %d bytes differ" % (K, s, norm, int((got != want).sum()))


def test_quantize_q8_0_edge_vectors(bamd, stored):
    """the edge activations (all-zero blocks, negative extrema, exact ties, blocks whose f16 d is subnormal or zero): the reference's own bytes, by digest"""
    for t in TYPES:
        key, blocks, xs, digest, _ = list(all_cases(t))[-1]
        _, q8sha, _ = stored_case(stored, key, digest)
        for i, x in enumerate(xs):
            got = bamd.op_quantize_q8_0(x)
            assert hashlib.sha256(got.tobytes()).hexdigest() == q8sha[i], "%s vector %d" % (key, i)
            assert np.array_equal(got, lg.quantize_row_q8_0(x))


# ---- mat-vec: the reference's own outputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("mode", MODES)
def test_mul_mat_vec_kats(bamd, stored, t, mode):
    """every stored case — K = 256, 512, 4096, 11008 (43 records: the uneven split-K share) and the edge matrix x edge vectors — in every launch mode"""
    for key, blocks, xs, digest, _ in all_cases(t):
        dots, _, _ = stored_case(stored, key, digest)
        K = xs[0].size
        for i, x in enumerate(xs):
            got = bamd.op_mul_mat_vec(t, blocks, lg.ROWS, K, x, mode=mode)
            assert_bits(got, dots[i], "%s vector %d mode %d" % (key, i, mode))


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("K", [256, 512, 4096, 11008, 14336])        # 1, 2, 16, 43, 56 records per row-group
def test_mul_mat_vec_shapes(bamd, po, t, K):
    """rows 8, 13 (a padded row-group) and 32; plain and RMSNorm prologue; with and without residual; every mode"""
    W, x, w, res = shape_case(t, K)
    rb = K // 32 * lg.BB[t]
    want_plain = lg.mul_mat(t, W, 32, K, x)
    want_norm = lg.mul_mat(t, W, 32, K, normed(po, x, w))
    for rows in (8, 13, 32):
        for mode in MODES:
            what = "type %d K %d rows %d mode %d" % (t, K, rows, mode)
            assert_bits(bamd.op_mul_mat_vec(t, W[:rows * rb], rows, K, x, mode=mode), want_plain[:rows], what)
            assert_bits(bamd.op_mul_mat_vec(t, W[:rows * rb], rows, K, x, residual=res[:rows], mode=mode), want_plain[:rows] + res[:rows], what + " + residual")
            assert_bits(bamd.op_mul_mat_vec(t, W[:rows * rb], rows, K, x, norm_w=w, eps=EPS, mode=mode), want_norm[:rows], what + " norm")
            assert_bits(bamd.op_mul_mat_vec(t, W[:rows * rb], rows, K, x, norm_w=w, eps=EPS, residual=res[:rows], mode=mode), want_norm[:rows] + res[:rows], what + " norm + residual")


@pytest.mark.parametrize("t", TYPES)
def test_mul_mat_vec_many_row_groups(bamd, po, t):
    """more row-groups than workgroups: in split-K a workgroup takes several row-groups, so both term buffers are used and the chain wave rotates.  In mode A the
    513 row-groups land on 256 workgroups x 8 waves = 2048 wave slots, so no wave takes a second row-group here: that walk (the next-row-group prefetch, the
    `last` flag of the final refill) is tests/test_gpu_sweep_families.py::test_tall_matrix_more_row_groups_than_wave_slots"""
    K, rows = 4096, 4104                                              # 513 row-groups
    rng = np.random.default_rng(77 + t)
    W = random_q0_tensor(t, K, rows, rng)
    x = (rng.standard_normal(K) * 2).astype(np.float32)
    res = rng.standard_normal(rows).astype(np.float32)
    want = lg.mul_mat(t, W, rows, K, x) + res
    for mode in MODES:
        assert_bits(bamd.op_mul_mat_vec(t, W, rows, K, x, residual=res, mode=mode), want, "type %d mode %d" % (t, mode))


@pytest.mark.parametrize("t", TYPES)
def test_split_k_single_term_buffer_many_row_groups(bamd, t):
    """K = 14336 (56 records: one term buffer, a second barrier per row-group) with more row-groups than workgroups: 2056 rows = 257 row-groups, so that on
    256 CUs one workgroup parks a second row-group into the buffer its chain wave has just read; mode 2 and, for the same bits, mode 1"""
    K, rows = 14336, 2056
    rng = np.random.default_rng(91 + t)
    W = random_q0_tensor(t, K, rows, rng)
    x = (rng.standard_normal(K) * 2).astype(np.float32)
    res = rng.standard_normal(rows).astype(np.float32)
    want = lg.mul_mat(t, W, rows, K, x) + res
    for mode in (2, 1):
        assert_bits(bamd.op_mul_mat_vec(t, W, rows, K, x, residual=res, mode=mode), want, "type %d mode %d" % (t, mode))


@pytest.mark.parametrize("K,mode", [(4096, 0), (512, 0)])
def test_argmax_q8_0(bamd, po, K, mode):
    """the lm_head launch of the Q8_0 recipe with its arg-max epilogue, the largest logit tied between rows of different workgroups: logits and the lowest tied row"""
    t, rows = lg.Q8_0, 4096
    rng = np.random.default_rng(60 + K)
    W = random_q0_tensor(t, K, rows, rng).reshape(rows, -1)
    x = (rng.standard_normal(K) * 2).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    a = normed(po, x, w)
    y0 = lg.mul_mat(t, W.reshape(-1), rows, K, a)
    grid = min(256, rows // 8)
    tied = [8 * (grid - 1) + 5, 8 * grid + 2]
    top, bottom = int(np.argmax(y0)), int(np.argmin(y0))
    best = W[top].copy()
    W[top] = W[bottom]
    W[tied] = best
    want = lg.mul_mat(t, W.reshape(-1), rows, K, a)
    assert np.flatnonzero(want == want.max()).tolist() == tied
    got, row = bamd.op_mul_mat_vec_argmax(t, W.reshape(-1), rows, K, x, norm_w=w, eps=EPS, mode=mode)
    assert_bits(got, want, "lm_head logits")
    assert row == int(np.argmax(want)) == tied[0]


# ---- gate/up, fused QKV, embedding rows --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("K,rows", [(512, 24), (4096, 24), (512, 1792), (4096, 1792)])
def test_ffn_gate_up(bamd, po, t, K, rows):
    rng = np.random.default_rng(5 * t + K + rows)
    Wg = random_q0_tensor(t, K, rows, rng, amp=4.0)
    Wu = random_q0_tensor(t, K, rows, rng, amp=4.0)
    x = (rng.standard_normal(K) * 2).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    a = normed(po, x, w)
    want = silu_mul(po, lg.mul_mat(t, Wg, rows, K, a), lg.mul_mat(t, Wu, rows, K, a))
    got = bamd.op_ffn_gate_up(t, Wg, Wu, rows, K, x, norm_w=w, eps=EPS)
    assert_bits(got, want, "ffn gate/up type %d K %d rows %d" % (t, K, rows))


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("E,H,Hkv", [(512, 8, 2), (4096, 32, 8)])
def test_fused_qkv(bamd, po, t, E, H, Hkv):
    """three segments of one type behind one RMSNorm prologue, in every mode"""
    rng = np.random.default_rng(31 + t + E)
    rows = [E, E // H * Hkv, E // H * Hkv]
    Ws = [random_q0_tensor(t, E, r, rng) for r in rows]
    x = (rng.standard_normal(E) * 2).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(E)).astype(np.float32)
    a = normed(po, x, w)
    want = np.concatenate([lg.mul_mat(t, W, r, E, a) for W, r in zip(Ws, rows)])
    for mode in MODES:
        got = bamd.op_fused_qkv([(t, W, r) for W, r in zip(Ws, rows)], E, x, w, eps=EPS, mode=mode)
        assert_bits(got, want, "fused QKV type %d E %d mode %d" % (t, E, mode))


def test_fused_launch_refuses_mixed_activation_forms(bamd):
    """a K-quant segment beside a Q8_0 one would need both activation forms in one launch: an error, never a run with the wrong form"""
    from booster_amd.gguf import random_kquant_tensor
    rng = np.random.default_rng(3)
    E = 512
    segs = [(12, random_kquant_tensor(12, E, 64, rng), 64), (lg.Q8_0, random_q0_tensor(lg.Q8_0, E, 64, rng), 64)]
    x = rng.standard_normal(E).astype(np.float32); w = np.ones(E, np.float32)
    for s in (segs, segs[::-1]):
        with pytest.raises(bamd.BamdError, match="type without a kernel"):
            bamd.op_fused_qkv(s, E, x, w, eps=EPS)


@pytest.mark.parametrize("t", TYPES)
def test_get_row_kats(bamd, stored, t):
    """embedding rows (dequantize_row_q*_0): first, middle and last row of every stored matrix, every row of the edge matrix"""
    for key, blocks, xs, digest, deq_rows in all_cases(t):
        _, _, deq = stored_case(stored, key, digest)
        K = xs[0].size
        for i, r in enumerate(deq_rows):
            assert_bits(bamd.op_get_row(t, blocks, lg.ROWS, K, r), deq[i], "%s get_row %d" % (key, r))


# ---- prompt evaluation: the integer-dot batched kernel with Q8_0 activation blobs ----------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("K", [256, 4096, 11008])
def test_mul_mat_batch(bamd, po, t, K):
    """T = 1, 2, 5, 33 (ragged token tiles) x rows 13 (a padded row-group) and 64; plain + residual and RMSNorm prologue"""
    rng = np.random.default_rng(77 * t + K)
    W = random_q0_tensor(t, K, 64, rng)
    rb = K // 32 * lg.BB[t]
    X = (rng.standard_normal((33, K)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    want_plain = np.stack([lg.mul_mat(t, W, 64, K, X[i]) for i in range(33)])
    want_norm = np.stack([lg.mul_mat(t, W, 64, K, normed(po, X[i], w)) for i in range(33)])
    for T in (1, 2, 5, 33):
        for rows in (13, 64):
            res = rng.standard_normal((T, rows)).astype(np.float32)
            what = "batch type %d K %d T %d rows %d" % (t, K, T, rows)
            assert_bits(bamd.op_mul_mat_batch(t, W[:rows * rb], rows, K, X[:T], residual=res, impl=0), want_plain[:T, :rows] + res, what + " + residual")
            assert_bits(bamd.op_mul_mat_batch(t, W[:rows * rb], rows, K, X[:T], norm_w=w, eps=EPS, impl=0), want_norm[:T, :rows], what + " norm")


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("K,T", [(256, 5), (4096, 33), (11008, 2)])
def test_mul_mat_batch_seg(bamd, po, t, K, T):
    """the segment form the engine uses: three segments into one [T][ldo] matrix (q | k | v), and gate / up with the SiLU epilogue"""
    rng = np.random.default_rng(99 * t + K + T)
    rows = [64, 16, 16]
    Ws = [random_q0_tensor(t, K, r, rng) for r in rows]
    X = (rng.standard_normal((T, K)) * 2).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    A = [normed(po, X[i], w) for i in range(T)]
    ldo = sum(rows) + 8
    got = bamd.op_mul_mat_batch_seg([(t, W, r) for W, r in zip(Ws, rows)], K, X, ldo, epi=0, norm_w=w, eps=EPS, fill=-7.0)
    want = np.full((T, ldo), -7.0, np.float32)
    for i in range(T):
        want[i, :sum(rows)] = np.concatenate([lg.mul_mat(t, W, r, K, A[i]) for W, r in zip(Ws, rows)])
    assert_bits(got, want, "q | k | v type %d K %d T %d" % (t, K, T))
    got = bamd.op_mul_mat_batch_seg([(t, Ws[1], 16), (t, Ws[2], 16)], K, X, 16, epi=2, norm_w=w, eps=EPS)
    want = np.stack([silu_mul(po, lg.mul_mat(t, Ws[1], 16, K, A[i]), lg.mul_mat(t, Ws[2], 16, K, A[i])) for i in range(T)])
    assert_bits(got, want, "gate / up type %d K %d T %d" % (t, K, T))


@pytest.mark.parametrize("t", TYPES)
def test_matrix_core_path_refuses_the_type(bamd, t):
    """the matrix-core prompt kernels have none of these types: asking for them is an error, never wrong numbers"""
    W, x, _, _ = shape_case(t, 4096)
    with pytest.raises(bamd.BamdError, match="MFMA path: unsupported type/shape"):
        bamd.op_mul_mat_batch(t, W, 32, 4096, np.stack([x, x]), impl=2)


# ---- attention and wo in one launch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [lg.Q8_0, lg.Q4_0, lg.Q5_0])
@pytest.mark.parametrize("H,Hkv,hd,pos,rows", [(32, 8, 128, 37, "4096"), (32, 8, 128, 446, "ragged"), (64, 8, 64, 0, "extra_max"), (16, 2, 256, 255, "extra0")])
def test_attention_wo(bamd, po, t, H, Hkv, hd, pos, rows):
    """the wo role of the co-launched attention + wo kernel with a Q8_0 / Q4_0 / Q5_0 wo, through tests/test_gpu_colaunch.py's run_case (attention role, granules,
    caches, x2) at its head layouts, positions and row kinds; the expectation of the wo rows comes from the restatement"""
    import test_gpu_colaunch as tc
    tc.run_case(bamd, po, t, H, Hkv, hd, 512, pos, rows, lds_ld=512, serial=3, step=pos + 1, il=t, gran_kind="ff" if pos else None,
                ref=lambda po_, t_, W, rows_, x: lg.mul_mat(t_, W, rows_, tc.K, x))
