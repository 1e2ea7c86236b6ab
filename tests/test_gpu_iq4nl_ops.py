"""GPU: the IQ4_NL kernels through the C-ABI (include/bamd.h bamd_op_*) against the genuine reference's stored outputs (tests/golden/iq4nl_kats.npz) and, at the
shapes the stored cases do not have, against the numpy restatement that tests/test_iq4nl_ref.py holds to those outputs (tests/iq4nl_ref.py).
Bit equality throughout; every expectation is finite."""
import functools

import numpy as np
import pytest

import iq4nl_ref as nl
import legacy_ref as lg
from bitcheck import assert_bits, EPS, normed, silu_mul
from booster_amd.gguf import random_iq4_nl_tensor, random_q0_tensor
from test_iq4nl_ref import stored_case, stored  # noqa: F401  (stored: fixture)

pytestmark = pytest.mark.gpu
T = nl.IQ4_NL
MODES = (0, 1)                     # the launcher's choice and one wave per row-group: the same kernel (mode 2, split-K, is refused: below)


def ref_mul_mat(t, W, rows, K, x):
    return nl.mul_mat(W, rows, K, x) if t == T else lg.mul_mat(t, W, rows, K, x)


def rand_w(t, K, rows, rng, amp=1.0):
    return random_iq4_nl_tensor(K, rows, rng, amp) if t == T else random_q0_tensor(t, K, rows, rng, amp)


@functools.lru_cache(maxsize=None)
def shape_case(K):
    """one 32-row matrix, one vector, one norm weight and one residual per K, shared by the tests, with its expectations (plain, RMSNorm)"""
    rng = np.random.default_rng(9000 * T + K)
    W = random_iq4_nl_tensor(K, 32, rng)
    x = (rng.standard_normal(K) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    res = rng.standard_normal(32).astype(np.float32)
    for a in (W, x, w, res):
        a.setflags(write=False)
    return W, x, w, res


# ---- mat-vec: the reference's own outputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_mul_mat_vec_kats(bamd, stored, mode):
    """every stored case — K = 256, 512, 4096, 11008 and the edge matrix x edge vectors (all nibbles 0 / 15, d negative / zero / subnormal / large)"""
    for key, blocks, xs, digest, _ in nl.all_cases():
        dots, _, _ = stored_case(stored, key, digest)
        K = xs[0].size
        for i, x in enumerate(xs):
            assert_bits(bamd.op_mul_mat_vec(T, blocks, nl.ROWS, K, x, mode=mode), dots[i], "%s vector %d mode %d" % (key, i, mode))


@pytest.mark.parametrize("K", [256, 512, 4096, 11008, 14336])        # 1, 2, 16, 43, 56 records per row-group: ring depths 1, 2, 4, 1, 4
def test_mul_mat_vec_shapes(bamd, po, K):
    """rows 32 and a ragged count (27 valid of 32); plain and RMSNorm prologue; store and add epilogue"""
    W, x, w, res = shape_case(K)
    rb = K // 32 * nl.BB
    want_plain = nl.mul_mat(W, 32, K, x)
    want_norm = nl.mul_mat(W, 32, K, normed(po, x, w))
    for rows in (27, 32):
        what = "K %d rows %d" % (K, rows)
        assert_bits(bamd.op_mul_mat_vec(T, W[:rows * rb], rows, K, x), want_plain[:rows], what)
        assert_bits(bamd.op_mul_mat_vec(T, W[:rows * rb], rows, K, x, residual=res[:rows]), want_plain[:rows] + res[:rows], what + " + residual")
        assert_bits(bamd.op_mul_mat_vec(T, W[:rows * rb], rows, K, x, norm_w=w, eps=EPS), want_norm[:rows], what + " norm")
        assert_bits(bamd.op_mul_mat_vec(T, W[:rows * rb], rows, K, x, norm_w=w, eps=EPS, residual=res[:rows]), want_norm[:rows] + res[:rows], what + " norm + residual")


def test_mul_mat_vec_many_row_groups(bamd):
    """more row-groups than waves in the grid (2049 row-groups on 256 workgroups x 8 waves = 2048 wave slots): exactly one wave streams a second row-group,
    the ragged last one (K = 512: ring depth 2 with one chunk, residual epilogue).  The other ring depths, a third walk and the gate/up and arg-max
    epilogues of that walk: tests/test_gpu_sweep_families.py::test_tall_matrix_more_row_groups_than_wave_slots"""
    K, rows = 512, 16389                                              # 2049 row-groups, 5 valid rows in the last
    rng = np.random.default_rng(77 + T)
    W = random_iq4_nl_tensor(K, rows, rng)
    x = (rng.standard_normal(K) * 2).astype(np.float32)
    res = rng.standard_normal(rows).astype(np.float32)
    assert_bits(bamd.op_mul_mat_vec(T, W, rows, K, x, residual=res), nl.mul_mat(W, rows, K, x) + res, "many row-groups")


@pytest.mark.parametrize("K", [512, 4096])
def test_argmax(bamd, po, K):
    """the arg-max epilogue, the largest logit tied between rows of different workgroups: logits and the lowest tied row"""
    rows = 4096
    rng = np.random.default_rng(60 + K)
    W = random_iq4_nl_tensor(K, rows, rng).reshape(rows, -1)
    x = (rng.standard_normal(K) * 2).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    a = normed(po, x, w)
    y0 = nl.mul_mat(W.reshape(-1), rows, K, a)
    grid = min(256, rows // 8)
    tied = [8 * (grid - 1) + 5, 8 * grid + 2]
    top, bottom = int(np.argmax(y0)), int(np.argmin(y0))
    best = W[top].copy()
    W[top] = W[bottom]
    W[tied] = best
    want = nl.mul_mat(W.reshape(-1), rows, K, a)
    assert np.flatnonzero(want == want.max()).tolist() == tied
    got, row = bamd.op_mul_mat_vec_argmax(T, W.reshape(-1), rows, K, x, norm_w=w, eps=EPS, mode=0)
    assert_bits(got, want, "logits")
    assert row == int(np.argmax(want)) == tied[0]


@pytest.mark.parametrize("K,rows", [(512, 24), (4096, 1792)])
def test_ffn_gate_up(bamd, po, K, rows):
    rng = np.random.default_rng(5 * T + K + rows)
    Wg = random_iq4_nl_tensor(K, rows, rng, amp=4.0)
    Wu = random_iq4_nl_tensor(K, rows, rng, amp=4.0)
    x = (rng.standard_normal(K) * 2).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    a = normed(po, x, w)
    want = silu_mul(po, nl.mul_mat(Wg, rows, K, a), nl.mul_mat(Wu, rows, K, a))
    assert_bits(bamd.op_ffn_gate_up(T, Wg, Wu, rows, K, x, norm_w=w, eps=EPS), want, "ffn gate/up K %d rows %d" % (K, rows))


@pytest.mark.parametrize("types", [(T, T, T), (T, lg.Q8_0, lg.Q4_0), (lg.Q5_0, T, lg.Q8_0), (lg.Q4_0, lg.Q4_0, T)])
def test_fused_segments_of_one_activation_form(bamd, po, types):
    """three segments behind one RMSNorm prologue in ONE launch: IQ4_NL beside Q8_0 / Q4_0 / Q5_0 segments (the same activation form) takes the kernel that has
    IQ4_NL, whose other type branches run here"""
    E = 512
    rng = np.random.default_rng(31 + sum(types))
    rows = [E, 128, 128]
    Ws = [rand_w(t, E, r, rng) for t, r in zip(types, rows)]
    x = (rng.standard_normal(E) * 2).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(E)).astype(np.float32)
    a = normed(po, x, w)
    want = np.concatenate([ref_mul_mat(t, W, r, E, a) for t, W, r in zip(types, Ws, rows)])
    for mode in MODES:
        got = bamd.op_fused_qkv([(t, W, r) for t, W, r in zip(types, Ws, rows)], E, x, w, eps=EPS, mode=mode)
        assert_bits(got, want, "fused segments %r mode %d" % (types, mode))


def test_launch_with_iq4_nl_goes_to_its_own_kernel(bamd):
    """launch selection: a launch with an IQ4_NL segment takes matvec_b32_nl_kernel; the same launch without one goes where it went before"""
    with_nl = bamd.trace_mv([(T, 4096), (lg.Q8_0, 1024)], 4096, 1, 0)
    last = bamd.trace_mv([(lg.Q8_0, 1024), (T, 4096)], 4096, 1, 0)
    without = bamd.trace_mv([(lg.Q4_0, 4096), (lg.Q8_0, 1024)], 4096, 1, 0)
    assert with_nl is not None and last is not None and without is not None
    assert "matvec_b32_nl_kernel" in with_nl["kernel"] and "matvec_b32_nl_kernel" in last["kernel"]
    assert "matvec_b32_nl_kernel" not in without["kernel"] and "matvec_b32_kernel" in without["kernel"]
    assert bamd.trace_matvec([(T, 4096)], 4096, 1, 0) is None                  # the K-quant launcher itself keeps refusing the type
    wo = bamd.trace_attn_wo(32, 8, 128, 512, 512, T, 4096, 4096)
    assert wo is not None and "attn_wo_b32_kernel" in wo["kernel"]


# ---- refusals, in words ------------------------------------------------------------------------------------------------------------------------
def test_split_k_is_refused(bamd):
    W, x, _, _ = shape_case(4096)
    with pytest.raises(bamd.BamdError, match="IQ4_NL has no split-K kernel"):
        bamd.op_mul_mat_vec(T, W, 32, 4096, x, mode=2)


def test_matrix_core_path_refuses_the_type(bamd):
    """the matrix-core prompt kernels do not have the type: asking for them is an error, never wrong numbers"""
    W, x, _, _ = shape_case(4096)
    with pytest.raises(bamd.BamdError, match="MFMA path: unsupported type/shape"):
        bamd.op_mul_mat_batch(T, W, 32, 4096, np.stack([x, x]), impl=2)


def test_fused_launch_refuses_mixed_activation_forms(bamd):
    """a K-quant segment beside an IQ4_NL one in one op call would need both activation forms in one launch: an error, never a run with the wrong form (the
    engine issues two launches for the one such pair a recipe writes; an op call is one launch)"""
    from booster_amd.gguf import random_kquant_tensor
    rng = np.random.default_rng(3)
    E = 512
    segs = [(13, random_kquant_tensor(13, E, 64, rng), 64), (T, random_iq4_nl_tensor(E, 64, rng), 64)]
    x = rng.standard_normal(E).astype(np.float32); w = np.ones(E, np.float32)
    for s in (segs, segs[::-1]):
        with pytest.raises(bamd.BamdError, match="type without a kernel"):
            bamd.op_fused_qkv(s, E, x, w, eps=EPS)
        with pytest.raises(bamd.BamdError, match="activation forms"):
            bamd.op_mul_mat_batch_seg(s, E, np.stack([x, x]), 128, epi=0, norm_w=w, eps=EPS)


# ---- embedding rows ----------------------------------------------------------------------------------------------------------------------------
def test_get_row_kats(bamd, stored):
    """embedding rows (dequantize_row_iq4_nl): first, middle and last row of every stored matrix, every row of the edge matrix"""
    for key, blocks, xs, digest, deq_rows in nl.all_cases():
        _, _, deq = stored_case(stored, key, digest)
        K = xs[0].size
        for i, r in enumerate(deq_rows):
            assert_bits(bamd.op_get_row(T, blocks, nl.ROWS, K, r), deq[i], "%s get_row %d" % (key, r))


# ---- prompt evaluation: the integer-dot batched kernel with Q8_0 activation blobs ----------------------------------------------------------------
@pytest.mark.parametrize("K,nt", [(256, 5), (4096, 33), (11008, 2)])
def test_mul_mat_batch(bamd, po, K, nt):
    """T tokens at once == the single-token mat-vec of every token, bit for bit (and both == the restatement): one matrix with a residual, then the segment form
    the engine uses — three segments into one [T][ldo] matrix (IQ4_NL | IQ4_NL | Q8_0) and gate / up with the SiLU epilogue"""
    rng = np.random.default_rng(99 * T + K + nt)
    rows = [64, 16, 16]
    types = [T, T, lg.Q8_0]
    Ws = [rand_w(t, K, r, rng) for t, r in zip(types, rows)]
    X = (rng.standard_normal((nt, K)) * 2).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    res = rng.standard_normal((nt, 13)).astype(np.float32)
    rb = K // 32 * nl.BB
    single = np.stack([bamd.op_mul_mat_vec(T, Ws[0][:13 * rb], 13, K, X[i], residual=res[i]) for i in range(nt)])
    assert_bits(single, np.stack([nl.mul_mat(Ws[0][:13 * rb], 13, K, X[i]) + res[i] for i in range(nt)]), "single-token K %d" % K)
    assert_bits(bamd.op_mul_mat_batch(T, Ws[0][:13 * rb], 13, K, X, residual=res, impl=0), single, "batch K %d T %d rows 13 + residual" % (K, nt))
    segs = [(t, W, r) for t, W, r in zip(types, Ws, rows)]
    ldo = sum(rows) + 8
    got = bamd.op_mul_mat_batch_seg(segs, K, X, ldo, epi=0, norm_w=w, eps=EPS, fill=-7.0)
    want = np.full((nt, ldo), -7.0, np.float32)
    for i in range(nt):
        want[i, :sum(rows)] = bamd.op_fused_qkv(segs, K, X[i], w, eps=EPS)
    assert_bits(got, want, "q | k | v K %d T %d" % (K, nt))
    A = [normed(po, X[i], w) for i in range(nt)]
    assert_bits(got[:, :sum(rows)], np.stack([np.concatenate([ref_mul_mat(t, W, r, K, A[i]) for t, W, r in zip(types, Ws, rows)]) for i in range(nt)]), "q | k | v restatement")
    got = bamd.op_mul_mat_batch_seg([(T, Ws[0][:16 * rb], 16), (T, Ws[1], 16)], K, X, 16, epi=2, norm_w=w, eps=EPS)
    want = np.stack([bamd.op_ffn_gate_up(T, Ws[0][:16 * rb], Ws[1], 16, K, X[i], norm_w=w, eps=EPS) for i in range(nt)])
    assert_bits(got, want, "gate / up K %d T %d" % (K, nt))
    assert_bits(got, np.stack([silu_mul(po, nl.mul_mat(Ws[0][:16 * rb], 16, K, A[i]), nl.mul_mat(Ws[1], 16, K, A[i])) for i in range(nt)]), "gate / up restatement")


# ---- attention and wo in one launch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Hkv,hd,pos,rows", [(32, 8, 128, 37, "4096"), (32, 8, 128, 446, "ragged"), (64, 8, 64, 0, "extra_max"), (16, 2, 256, 255, "extra0")])
def test_attention_wo(bamd, po, H, Hkv, hd, pos, rows):
    """the wo role of the co-launched attention + wo kernel with an IQ4_NL wo at K = 4096, through tests/test_gpu_colaunch.py's run_case (attention role,
    granules, caches, x2) at its head layouts, positions and row kinds; the expectation of the wo rows comes from the restatement"""
    import test_gpu_colaunch as tc
    tc.run_case(bamd, po, T, H, Hkv, hd, 512, pos, rows, lds_ld=512, serial=3, step=pos + 1, il=T, gran_kind="ff" if pos else None,
                ref=lambda po_, t_, W, rows_, x: nl.mul_mat(W, rows_, tc.K, x))
