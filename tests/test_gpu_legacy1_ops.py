"""GPU: the Q4_1 / Q5_1 kernels through the C-ABI (include/bamd.h bamd_op_*) against the genuine reference's stored outputs (tests/golden/legacy1_kats.npz)
and, at the shapes the stored cases do not have, against the numpy restatement that tests/test_legacy1_ref.py holds to those outputs (tests/legacy1_ref.py).
Bit equality throughout; every expectation is finite."""
import functools
import hashlib

import numpy as np
import pytest

import legacy1_ref as l1
from bitcheck import assert_bits, EPS, normed, silu_mul
from booster_amd.gguf import random_kquant_tensor, random_q0_tensor, random_q1_tensor
from legacy1_ref import all_cases
from test_legacy1_ref import stored_case, stored  # noqa: F401  (stored: fixture)

pytestmark = pytest.mark.gpu
TYPES = list(l1.TYPES)
MODES = (0, 1)                     # the launcher's choice and one wave per row-group; split-K (mode 2) does not exist for these types
# the batched kernel takes token tiles of 8 while 8 activation images fit the LDS: 8 * blob bytes(K) <= 160 KB with blob bytes = 292 * K / 256 rounded up to 16
# (bamd_launch_matmul_batch_b32), i.e. up to K = 17920 (70 records); K = 18176 is the first row length that takes tiles of 4
K_TILE4 = 18176
assert 8 * ((292 * (K_TILE4 // 256 - 1) + 15) // 16 * 16) <= 160 * 1024 < 8 * ((292 * (K_TILE4 // 256) + 15) // 16 * 16)


@functools.lru_cache(maxsize=None)
def shape_case(t, K):
    """one 32-row matrix, one vector, one norm weight and one residual per (type, K), shared by the tests; rows 8 and 13 are its leading rows"""
    rng = np.random.default_rng(9100 * t + K)
    W = random_q1_tensor(t, K, 32, rng)
    x = (rng.standard_normal(K) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    res = rng.standard_normal(32).astype(np.float32)
    for a in (W, x, w, res):
        a.setflags(write=False)
    return W, x, w, res


# ---- the activation quantiser ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [256, 4096])
@pytest.mark.parametrize("norm", [False, True])
def test_quantize_q8_1(bamd, po, K, norm):
    rng = np.random.default_rng(K + norm)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32) if norm else None
    for s in l1.SCALES:
        x = (rng.standard_normal(K) * s).astype(np.float32)
        got = bamd.op_quantize_q8_1(x, norm_w=w, eps=EPS)
        want = l1.quantize_row_q8_1(x if w is None else normed(po, x, w))
        assert np.isfinite(l1.q8_1_fields(want)[1]).all()
        assert np.array_equal(got, want), "Q8_1 bytes, K %d scale %g norm %d: %d bytes differ" % (K, s, norm, int((got != want).sum()))


def test_quantize_q8_1_edge_vectors(bamd, stored):
    """the edge activations (all-zero blocks, negative extrema, exact ties, blocks whose f16 d is subnormal or zero, single values, blocks of equal values with
    |sum| = 4064): the reference's own bytes, by digest; and the vector with a block whose s overflows f16 to +-inf"""
    for t in TYPES:
        key, blocks, xs, digest, _ = list(all_cases(t))[-1]
        _, q8sha, _ = stored_case(stored, key, digest)
        for i, x in enumerate(xs):
            got = bamd.op_quantize_q8_1(x)
            assert hashlib.sha256(got.tobytes()).hexdigest() == q8sha[i], "%s vector %d" % (key, i)
            assert np.array_equal(got, l1.quantize_row_q8_1(x))
    x = l1.overflow_vector()
    assert hashlib.sha256(x.tobytes()).hexdigest() == str(stored["overflow_inputs_sha256"])
    got = bamd.op_quantize_q8_1(x)
    assert hashlib.sha256(got.tobytes()).hexdigest() == str(stored["overflow_q8_sha256"]), "the overflow vector"
    s = l1.q8_1_fields(got)[1]
    assert np.isposinf(s[3]) and np.isneginf(s[5])


def test_quantize_q8_1_rounds_the_sum_field_twice(bamd, stored):
    """s = f16(f32(d * sum)): 64 blocks on which rounding the exact product once gives another f16 (a multiply folded into the conversion would); the
    reference's own bytes, by digest"""
    x = l1.double_rounding_vector()
    assert hashlib.sha256(x.tobytes()).hexdigest() == str(stored["round2_inputs_sha256"])
    got = bamd.op_quantize_q8_1(x)
    want = l1.quantize_row_q8_1(x)
    assert np.isfinite(l1.q8_1_fields(want)[1]).all()
    assert np.array_equal(got, want), "%d bytes differ" % int((got != want).sum())
    assert hashlib.sha256(got.tobytes()).hexdigest() == str(stored["round2_q8_sha256"])


# ---- mat-vec: the reference's own outputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("mode", MODES)
def test_mul_mat_vec_kats(bamd, stored, t, mode):
    """every stored case — K = 256, 512, 4096, 11008 (43 records: an odd count, ring depth 1) and the edge matrix x edge vectors — in both launch modes"""
    for key, blocks, xs, digest, _ in all_cases(t):
        dots, _, _ = stored_case(stored, key, digest)
        K = xs[0].size
        for i, x in enumerate(xs):
            got = bamd.op_mul_mat_vec(t, blocks, l1.ROWS, K, x, mode=mode)
            assert_bits(got, dots[i], "%s vector %d mode %d" % (key, i, mode))


@pytest.mark.parametrize("t", TYPES)
def test_split_k_is_refused(bamd, t):
    """mode 2 (split-K) is not built for these types: an error in words, never another kernel's numbers"""
    W, x, _, _ = shape_case(t, 4096)
    with pytest.raises(bamd.BamdError, match="Q4_1 / Q5_1 have no split-K kernel"):
        bamd.op_mul_mat_vec(t, W, 32, 4096, x, mode=2)


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("K", [256, 512, 4096, 11008, 14336])        # 1, 2, 16, 43, 56 records per row-group: ring depths 1, 2, 4, 1, 4
def test_mul_mat_vec_shapes(bamd, po, t, K):
    """rows 8, 13 (a padded row-group) and 32; plain and RMSNorm prologue; with and without residual"""
    W, x, w, res = shape_case(t, K)
    rb = K // 32 * l1.BB[t]
    want_plain = l1.mul_mat(t, W, 32, K, x)
    want_norm = l1.mul_mat(t, W, 32, K, normed(po, x, w))
    for rows in (8, 13, 32):
        for mode in MODES:
            what = "type %d K %d rows %d mode %d" % (t, K, rows, mode)
            assert_bits(bamd.op_mul_mat_vec(t, W[:rows * rb], rows, K, x, mode=mode), want_plain[:rows], what)
            assert_bits(bamd.op_mul_mat_vec(t, W[:rows * rb], rows, K, x, residual=res[:rows], mode=mode), want_plain[:rows] + res[:rows], what + " + residual")
            assert_bits(bamd.op_mul_mat_vec(t, W[:rows * rb], rows, K, x, norm_w=w, eps=EPS, mode=mode), want_norm[:rows], what + " norm")
            assert_bits(bamd.op_mul_mat_vec(t, W[:rows * rb], rows, K, x, norm_w=w, eps=EPS, residual=res[:rows], mode=mode), want_norm[:rows] + res[:rows], what + " norm + residual")


@pytest.mark.parametrize("t", TYPES)
def test_mul_mat_vec_many_row_groups(bamd, po, t):
    """more row-groups than waves in the grid: 20488 rows = 2561 row-groups over 256 workgroups x 8 waves = 2048 wave slots, so 513 waves stream a second
    row-group (K = 512: ring depth 2 with one chunk, residual epilogue).  The other ring depths, a third walk, a ragged last row-group and the gate/up and
    arg-max epilogues of that walk: tests/test_gpu_sweep_families.py::test_tall_matrix_more_row_groups_than_wave_slots"""
    K, rows = 512, 20488
    rng = np.random.default_rng(77 + t)
    W = random_q1_tensor(t, K, rows, rng)
    x = (rng.standard_normal(K) * 2).astype(np.float32)
    res = rng.standard_normal(rows).astype(np.float32)
    want = l1.mul_mat(t, W, rows, K, x) + res
    for mode in MODES:
        assert_bits(bamd.op_mul_mat_vec(t, W, rows, K, x, residual=res, mode=mode), want, "type %d mode %d" % (t, mode))


@pytest.mark.parametrize("t,K", [(l1.Q4_1, 4096), (l1.Q5_1, 512)])
def test_argmax(bamd, po, t, K):
    """the arg-max epilogue, the largest logit tied between rows of different workgroups: logits and the lowest tied row"""
    rows = 4096
    rng = np.random.default_rng(60 + K)
    W = random_q1_tensor(t, K, rows, rng).reshape(rows, -1)
    x = (rng.standard_normal(K) * 2).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    a = normed(po, x, w)
    y0 = l1.mul_mat(t, W.reshape(-1), rows, K, a)
    grid = min(256, rows // 8)
    tied = [8 * (grid - 1) + 5, 8 * grid + 2]
    top, bottom = int(np.argmax(y0)), int(np.argmin(y0))
    best = W[top].copy()
    W[top] = W[bottom]
    W[tied] = best
    want = l1.mul_mat(t, W.reshape(-1), rows, K, a)
    assert np.flatnonzero(want == want.max()).tolist() == tied
    got, row = bamd.op_mul_mat_vec_argmax(t, W.reshape(-1), rows, K, x, norm_w=w, eps=EPS, mode=0)
    assert_bits(got, want, "logits")
    assert row == int(np.argmax(want)) == tied[0]


# ---- gate/up, fused QKV, embedding rows --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("K,rows", [(512, 24), (4096, 24), (512, 1792)])
def test_ffn_gate_up(bamd, po, t, K, rows):
    rng = np.random.default_rng(5 * t + K + rows)
    Wg = random_q1_tensor(t, K, rows, rng, amp=4.0)
    Wu = random_q1_tensor(t, K, rows, rng, amp=4.0)
    x = (rng.standard_normal(K) * 2).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    a = normed(po, x, w)
    want = silu_mul(po, l1.mul_mat(t, Wg, rows, K, a), l1.mul_mat(t, Wu, rows, K, a))
    got = bamd.op_ffn_gate_up(t, Wg, Wu, rows, K, x, norm_w=w, eps=EPS)
    assert_bits(got, want, "ffn gate/up type %d K %d rows %d" % (t, K, rows))


@pytest.mark.parametrize("E,H,Hkv", [(512, 8, 2), (4096, 32, 8)])
def test_fused_qkv_mixed_q4_1_q5_1(bamd, po, E, H, Hkv):
    """Q4_1 | Q4_1 | Q5_1 behind one RMSNorm prologue: segments of both types share a launch (one activation form)"""
    rng = np.random.default_rng(31 + E)
    rows = [E, E // H * Hkv, E // H * Hkv]
    types = [l1.Q4_1, l1.Q4_1, l1.Q5_1]
    Ws = [random_q1_tensor(t, E, r, rng) for t, r in zip(types, rows)]
    x = (rng.standard_normal(E) * 2).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(E)).astype(np.float32)
    a = normed(po, x, w)
    want = np.concatenate([l1.mul_mat(t, W, r, E, a) for t, W, r in zip(types, Ws, rows)])
    for mode in MODES:
        got = bamd.op_fused_qkv([(t, W, r) for t, W, r in zip(types, Ws, rows)], E, x, w, eps=EPS, mode=mode)
        assert_bits(got, want, "fused QKV E %d mode %d" % (E, mode))


def test_fused_launch_refuses_mixed_activation_forms(bamd):
    """a Q4_0 or a Q4_K segment beside a Q4_1 one would need two activation forms in one launch: an error, never a run with the wrong form"""
    rng = np.random.default_rng(3)
    E = 512
    q1 = (l1.Q4_1, random_q1_tensor(l1.Q4_1, E, 64, rng), 64)
    x = rng.standard_normal(E).astype(np.float32); w = np.ones(E, np.float32)
    for other in ((2, random_q0_tensor(2, E, 64, rng), 64), (12, random_kquant_tensor(12, E, 64, rng), 64)):
        for s in ([q1, other], [other, q1]):
            with pytest.raises(bamd.BamdError, match="type without a kernel"):
                bamd.op_fused_qkv(s, E, x, w, eps=EPS)
            with pytest.raises(bamd.BamdError, match="activation forms"):
                bamd.op_mul_mat_batch_seg(s, E, np.stack([x, x]), 128, epi=0, norm_w=w, eps=EPS)


@pytest.mark.parametrize("t", TYPES)
def test_get_row_kats(bamd, stored, t):
    """embedding rows (dequantize_row_q*_1): first, middle and last row of every stored matrix, every row of the edge matrix"""
    for key, blocks, xs, digest, deq_rows in all_cases(t):
        _, _, deq = stored_case(stored, key, digest)
        K = xs[0].size
        for i, r in enumerate(deq_rows):
            assert_bits(bamd.op_get_row(t, blocks, l1.ROWS, K, r), deq[i], "%s get_row %d" % (key, r))


# ---- prompt evaluation: the integer-dot batched kernel with Q8_1 activation blobs ----------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("K", [512, 4096, K_TILE4])
def test_mul_mat_batch(bamd, po, t, K):
    """T = 1, 5, 8, 13 (token tiles of 8 with a ragged tail; of 4 at K_TILE4) x rows 13 (a padded row-group) and 64; plain + residual and RMSNorm prologue;
    the batched result equals the restatement of every token, and the single-token kernel token by token"""
    rng = np.random.default_rng(77 * t + K)
    W = random_q1_tensor(t, K, 64, rng)
    rb = K // 32 * l1.BB[t]
    X = (rng.standard_normal((13, K)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    want_plain = np.stack([l1.mul_mat(t, W, 64, K, X[i]) for i in range(13)])
    want_norm = np.stack([l1.mul_mat(t, W, 64, K, normed(po, X[i], w)) for i in range(13)])
    for i in (0, 12):
        assert_bits(bamd.op_mul_mat_vec(t, W, 64, K, X[i], norm_w=w, eps=EPS), want_norm[i], "token %d through the single-token kernel" % i)
    for T in (1, 5, 8, 13):
        for rows in (13, 64):
            res = rng.standard_normal((T, rows)).astype(np.float32)
            what = "batch type %d K %d T %d rows %d" % (t, K, T, rows)
            assert_bits(bamd.op_mul_mat_batch(t, W[:rows * rb], rows, K, X[:T], residual=res, impl=0), want_plain[:T, :rows] + res, what + " + residual")
            assert_bits(bamd.op_mul_mat_batch(t, W[:rows * rb], rows, K, X[:T], norm_w=w, eps=EPS, impl=0), want_norm[:T, :rows], what + " norm")


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("K,T", [(512, 5), (4096, 13), (K_TILE4, 5)])
def test_mul_mat_batch_seg(bamd, po, t, K, T):
    """the segment form the engine uses: three segments (the last of the other "_1" type) into one [T][ldo] matrix (q | k | v), and gate / up with the SiLU
    epilogue"""
    rng = np.random.default_rng(99 * t + K + T)
    rows = [64, 16, 16]
    other = l1.Q5_1 if t == l1.Q4_1 else l1.Q4_1
    types = [t, t, other]
    Ws = [random_q1_tensor(tt, K, r, rng) for tt, r in zip(types, rows)]
    X = (rng.standard_normal((T, K)) * 2).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    A = [normed(po, X[i], w) for i in range(T)]
    ldo = sum(rows) + 8
    got = bamd.op_mul_mat_batch_seg([(tt, W, r) for tt, W, r in zip(types, Ws, rows)], K, X, ldo, epi=0, norm_w=w, eps=EPS, fill=-7.0)
    want = np.full((T, ldo), -7.0, np.float32)
    for i in range(T):
        want[i, :sum(rows)] = np.concatenate([l1.mul_mat(tt, W, r, K, A[i]) for tt, W, r in zip(types, Ws, rows)])
    assert_bits(got, want, "q | k | v type %d K %d T %d" % (t, K, T))
    Wu = random_q1_tensor(t, K, 16, rng)
    got = bamd.op_mul_mat_batch_seg([(t, Ws[1], 16), (t, Wu, 16)], K, X, 16, epi=2, norm_w=w, eps=EPS)
    want = np.stack([silu_mul(po, l1.mul_mat(t, Ws[1], 16, K, A[i]), l1.mul_mat(t, Wu, 16, K, A[i])) for i in range(T)])
    assert_bits(got, want, "gate / up type %d K %d T %d" % (t, K, T))


@pytest.mark.parametrize("t", TYPES)
def test_matrix_core_path_refuses_the_type(bamd, t):
    """the matrix-core prompt kernels have none of these types: asking for them is an error, never wrong numbers"""
    W, x, _, _ = shape_case(t, 4096)
    with pytest.raises(bamd.BamdError, match="MFMA path: unsupported type/shape"):
        bamd.op_mul_mat_batch(t, W, 32, 4096, np.stack([x, x]), impl=2)


# ---- attention and wo in one launch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("H,Hkv,hd,pos,rows", [(32, 8, 128, 37, "4096"), (32, 8, 128, 446, "ragged"), (64, 8, 64, 0, "extra_max"), (64, 8, 64, 70, "extra0")])
def test_attention_wo(bamd, po, t, H, Hkv, hd, pos, rows):
    """the wo role of the co-launched attention + wo kernel with a Q4_1 / Q5_1 wo at K = 4096, heads of 64 and 128, through tests/test_gpu_colaunch.py's
    run_case (attention role, granules, caches, x2 against the oracle; the give-up counter is 0); the expectation of the wo rows comes from the restatement.
    Then the same output from two launches: the attention output the granules carry through the ordinary mat-vec with the residual"""
    import test_gpu_colaunch as tc
    n = tc.wo_rows(rows, tc.device_cus(bamd), H)
    rng = np.random.default_rng([t, H, pos])
    W = random_q1_tensor(t, tc.K, n, rng)
    r = tc.run_case(bamd, po, t, H, Hkv, hd, 512, pos, rows, lds_ld=512, serial=3, step=pos + 1, il=t, gran_kind="ff" if pos else None, W=W,
                    ref=lambda po_, t_, W_, rows_, x: l1.mul_mat(t_, W_, rows_, tc.K, x))
    assert r["gave_up"] == 0 and not r["declined"]
    att = (r["gran"] & np.uint64(0xffffffff)).astype(np.uint32).view(np.float32)
    res = np.random.default_rng([0, t, H, Hkv, hd, pos, n])          # run_case's generator: replay its draws up to the residual
    tc.attention_inputs(res, H, Hkv, hd, 512)
    residual = res.standard_normal(n).astype(np.float32)
    assert_bits(r["x2"], bamd.op_mul_mat_vec(t, W, n, tc.K, att, residual=residual, mode=1), "co-launch vs two launches")


@pytest.mark.parametrize("t", TYPES)
def test_attention_wo_declines_k8192(bamd, t):
    """K = 8192 has no co-launch for these types: the launcher declines and the caller issues the two launches"""
    z = np.zeros
    H, Hkv, hd, n_ctx, rows = 64, 8, 128, 64, 8192
    rng = np.random.default_rng(t)
    W = random_q1_tensor(t, 8192, rows, rng)
    r = bamd.op_attention_wo(z(H * hd, np.float32), z(Hkv * hd, np.float32), z(Hkv * hd, np.float32), z(n_ctx * Hkv * hd, np.uint16), z(n_ctx * Hkv * hd, np.uint16),
                             z(hd, np.float32), H, Hkv, hd, n_ctx, 0, t, W, rows, z(rows, np.float32))
    assert r["declined"]
