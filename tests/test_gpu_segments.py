"""GPU: launches over more than one weight segment, with the argument blocks of the engine:
  * the fused QKV launch of a decode step over differently typed segments (bamd_op_fused_qkv -> bamd_launch_matvec: the mixed-type split-K kernel where a
    type pair has an instance, one wave per row-group over mixed segments elsewhere), with the split point between the segments moved across the
    workgroup boundaries;
  * the batched prompt mat-muls as enqueue_prefill_batch issues them (bamd_op_mul_mat_batch_seg -> the engine's own routing function): q | k | v into one
    [T][ldo] matrix, ldo > rows, the silu(gate) * up pair on the integer-dot kernel and, in place, on the matrix cores.
Expectation per segment: the oracle's mul_mat_q (Q4_K / Q5_K / Q6_K) or tests/lowbit_ref.py (Q2_K / Q3_K) of the oracle's normalised activations; bit
equality throughout, every expectation finite.  Nothing here depends on BAMD_MIXED_SPLIT or BAMD_MV_GENERIC: those switches select another kernel, not
other bits."""
import numpy as np
import pytest

import edge_inputs as ei
import lowbit_ref as lr
from bitcheck import ADD, assert_bits, EPS, FILL, normed, SILU_MUL, silu_mul, STORE
from booster_amd.gguf import GGML_TYPES, random_kquant_tensor

pytestmark = pytest.mark.gpu
Q2, Q3, Q4, Q5, Q6 = 10, 11, 12, 13, 14
PAIRS = [(Q4, Q6), (Q4, Q5), (Q5, Q6), (Q3, Q4), (Q3, Q5), (Q2, Q4), (Q2, Q3)]      # the type pairs matvec_split_mixed_kernel has instances for


def row_bytes(t, K):
    return K // 256 * GGML_TYPES[t][1]


def ref_mul_mat(po, t, W, rows, K, x):
    """[T][rows] for x [T][K] (or [rows] for x [K])"""
    x = np.ascontiguousarray(x, np.float32)
    if t in (Q2, Q3):
        return lr.mul_mat(po, t, W, rows, K, x) if x.ndim == 1 else np.stack([lr.mul_mat(po, t, W, rows, K, xi) for xi in x])
    y = po.mul_mat_q(t, W, rows, K, x, nthreads=8)
    return y[0] if x.ndim == 1 else y


# ---- the fused QKV launch --------------------------------------------------------------------------------------------------------------------------
_pool = {}


def pool(po, t, K, rows):
    """one random matrix per (type, K), one activation vector per K, and the expectation of every row: a segment of r rows is the first r rows of its
    type's matrix, so that the many split points below share one reference computation per type"""
    if ("x", K) not in _pool:
        rng = np.random.default_rng(K)
        x = (rng.standard_normal(K) * 2).astype(np.float32); w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
        _pool[("x", K)] = (x, w, normed(po, x, w))
    cap = 6144 if K == 4096 else 9216 if t == Q4 else 1024
    assert rows <= cap
    if (t, K) not in _pool:
        W = random_kquant_tensor(t, K, cap, np.random.default_rng(100 * t + K))
        _pool[(t, K)] = (W, ref_mul_mat(po, t, W, cap, K, _pool[("x", K)][2]))
    W, y = _pool[(t, K)]
    return W[:rows * row_bytes(t, K)], y[:rows]


def fused_qkv_case(bamd, po, K, segs, mode=0, what=""):
    """segs: [(type, rows), ...] from the pool"""
    parts = [pool(po, t, K, r) for t, r in segs]
    x, w, _ = _pool[("x", K)]
    got = bamd.op_fused_qkv([(t, W, r) for (t, r), (W, _) in zip(segs, parts)], K, x, w, eps=EPS, mode=mode)
    off = 0
    for i, ((t, r), (_, y)) in enumerate(zip(segs, parts)):
        assert_bits(got[off:off + r], y, "%s K %d segments %r mode %d: segment %d (type %d)" % (what, K, segs, mode, i, t))
        off += r


@pytest.mark.parametrize("nrg0", [512, 513, 640, 767])
@pytest.mark.parametrize("t0,t1", PAIRS)
def test_fused_qkv_mixed_split_points(bamd, po, t0, t1, nrg0):
    """K = 4096, 768 row-groups = three per workgroup on 256 CUs; each workgroup picks its body by whether its LAST row-group (512 + its index) is still in
    segment 0.  512: no workgroup's is; 513: exactly one; 640: the 8B shape; 767: all but one"""
    fused_qkv_case(bamd, po, 4096, [(t0, nrg0 * 8), (t1, 6144 - nrg0 * 8)])


@pytest.mark.parametrize("mode", [1, 2, 16])
@pytest.mark.parametrize("t0,t1", PAIRS)
def test_fused_qkv_mixed_modes(bamd, po, t0, t1, mode):
    """the 8B split on the other kernels: one wave per row-group, the generic split-K kernel streaming its segments one after the other, the generic
    kernels forced (mode 0: test_fused_qkv_mixed_split_points)"""
    fused_qkv_case(bamd, po, 4096, [(t0, 5120), (t1, 1024)], mode=mode)


@pytest.mark.parametrize("t0,t1", [(Q6, Q4), (Q5, Q4), (Q2, Q5)])
def test_fused_qkv_pairs_without_an_instance(bamd, po, t0, t1):
    """no mixed-type instance: the launcher sends these to one wave per row-group over mixed segments"""
    fused_qkv_case(bamd, po, 4096, [(t0, 5120), (t1, 1024)])


def test_fused_qkv_three_types(bamd, po):
    for mode in (0, 1, 2, 16):
        fused_qkv_case(bamd, po, 4096, [(Q4, 4096), (Q5, 1024), (Q6, 1024)], mode=mode)
    fused_qkv_case(bamd, po, 4096, [(Q2, 4096), (Q3, 1024), (Q6, 1024)])


@pytest.mark.parametrize("t0,t1", [(Q4, Q6), (Q3, Q5)])
def test_fused_qkv_total_not_a_multiple_of_the_grid(bamd, po, t0, t1):
    """H 32 with Hkv 4: 4096 + 512 | 512 rows = 640 row-groups on 256 workgroups"""
    fused_qkv_case(bamd, po, 4096, [(t0, 4608), (t1, 512)])


@pytest.mark.parametrize("t1", [Q6, Q5])
def test_fused_qkv_70b_shape(bamd, po, t1):
    """K = 8192, 1024 + 128 | 128 row-groups (five per workgroup), the launcher's default path"""
    fused_qkv_case(bamd, po, 8192, [(Q4, 9216), (t1, 1024)])


@pytest.mark.parametrize("t0,t1", [(Q4, Q6), (Q4, Q5), (Q5, Q6)])
def test_fused_qkv_mixed_edge_values(bamd, po, t0, t1):
    """edge weights (tests/edge_inputs.py) in both segments against edge activations behind the RMSNorm prologue, at the 8B split and with one workgroup's
    last row-group in segment 0"""
    K = 4096
    rng = np.random.default_rng(10 * t0 + t1)
    x, xt = ei.edge_activations(K, rng, huge_max=1e15)
    assert set(xt) == set(ei.ACT_KINDS)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    a = normed(po, x, w)
    assert np.isfinite(a).all()
    for nrg0 in (640, 513):
        r0, r1 = nrg0 * 8, 6144 - nrg0 * 8
        (W0, wt0), (W1, wt1) = ei.edge_kquant_tensor(t0, K, r0, rng), ei.edge_kquant_tensor(t1, K, r1, rng)
        assert set(wt0.reshape(-1)) == set(wt1.reshape(-1)) == set(ei.WEIGHT_KINDS)
        got = bamd.op_fused_qkv([(t0, W0, r0), (t1, W1, r1)], K, x, w, eps=EPS)
        assert_bits(got[:r0], ref_mul_mat(po, t0, W0, r0, K, a), "edge values, split %d: segment 0 (type %d)" % (nrg0, t0))
        assert_bits(got[r0:], ref_mul_mat(po, t1, W1, r1, K, a), "edge values, split %d: segment 1 (type %d)" % (nrg0, t1))


# ---- batched prompt mat-muls as the engine issues them ---------------------------------------------------------------------------------------------------
TS = [1, 7, 64, 65, 129]


def batch_inputs(K, T, seed):
    rng = np.random.default_rng([K, T, seed])
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    return rng, X, w


def qkv_batch_case(bamd, po, t0, t1, T, impls, what, r0=5120, r1=1024):
    """the QKV call of the prompt path (the 8B one by default: 5120 + 1024 rows into [T][6144])"""
    K = 4096
    rng, X, w = batch_inputs(K, T, 10 * t0 + t1)
    W0, W1 = random_kquant_tensor(t0, K, r0, rng), random_kquant_tensor(t1, K, r1, rng)
    A = np.stack([normed(po, x, w) for x in X])
    want = np.concatenate([ref_mul_mat(po, t0, W0, r0, K, A), ref_mul_mat(po, t1, W1, r1, K, A)], axis=1)
    for impl in impls:
        got = bamd.op_mul_mat_batch_seg([(t0, W0, r0), (t1, W1, r1)], K, X, r0 + r1, epi=STORE, norm_w=w, eps=EPS, impl=impl)
        assert_bits(got[:, :r0], want[:, :r0], "%s T %d impl %d: segment 0 (type %d)" % (what, T, impl, t0))
        assert_bits(got[:, r0:], want[:, r0:], "%s T %d impl %d: segment 1 (type %d)" % (what, T, impl, t1))


@pytest.mark.parametrize("T", TS)
def test_batch_qkv_two_segments(bamd, po, T):
    """Q4_K | Q6_K: one integer-dot launch over both segments (impl 0); two matrix-core launches into the one output matrix (impl 2)"""
    qkv_batch_case(bamd, po, Q4, Q6, T, (0, 2), "batched QKV")


@pytest.mark.parametrize("T", [3])                  # (the restatement behind the low-bit expectation takes a second per token at 5120 rows; more tokens: the 256-row case below)
def test_batch_qkv_low_bit_first_segment(bamd, po, T):
    """Q3_K | Q6_K under the matrix-core selector: the Q3_K segment stays on the integer-dot kernel, the Q6_K one takes the matrix cores; both against the
    reference, so also bit-identical to the all-integer-dot run"""
    qkv_batch_case(bamd, po, Q3, Q6, T, (0, 2), "batched QKV, low-bit first segment")


@pytest.mark.parametrize("t0,T", [(Q3, 65), (Q2, 9)])
def test_batch_qkv_low_bit_first_segment_across_token_tiles(bamd, po, t0, T):
    """the same routing over more than one 64-token tile of the matrix-core kernel and nine 8-token tiles of the integer-dot kernel (65 tokens), and over
    a ragged second 8-token tile (9 tokens), with a first segment of 256 rows only, so that the restatement behind its expectation stays affordable"""
    qkv_batch_case(bamd, po, t0, Q6, T, (0, 2), "batched QKV, short low-bit first segment", r0=256, r1=1024)


@pytest.mark.parametrize("t0,t1", [(Q2, Q3)])
def test_batch_qkv_low_bit_pair_falls_to_integer_dot(bamd, po, t0, t1):
    """no segment has a matrix-core kernel: the selector must fall to the integer-dot kernel as the engine does, not refuse"""
    qkv_batch_case(bamd, po, t0, t1, 2, (2,), "batched QKV, low-bit pair")


@pytest.mark.parametrize("t,T", [(Q4, 7), (Q4, 65), (Q6, 7), (Q6, 65), (Q5, 129), (Q3, 3)])
def test_batch_add_with_wide_rows(bamd, po, t, T):
    """residual add with ldo > rows (4096 rows in rows of 4224 floats): output and residual share the stride, the columns behind the rows stay untouched"""
    K, rows, ldo = 4096, 4096, 4224
    rng, X, _ = batch_inputs(K, T, t)
    W = random_kquant_tensor(t, K, rows, rng)
    res = rng.standard_normal((T, ldo)).astype(np.float32)
    want = ref_mul_mat(po, t, W, rows, K, X) + res[:, :rows]
    for impl in (0, 2):
        got = bamd.op_mul_mat_batch_seg([(t, W, rows)], K, X, ldo, epi=ADD, residual=res, impl=impl, fill=FILL)
        assert_bits(got[:, :rows], want, "batched add type %d T %d impl %d" % (t, T, impl))
        assert (got[:, rows:] == FILL).all(), "impl %d wrote behind the rows" % impl


@pytest.mark.parametrize("t,K,rows,Ts", [(t, 4096, 14336, (7, 65)) for t in (Q4, Q5, Q6)] + [(t, 512, 768, tuple(TS)) for t in (Q4, Q5, Q6)] +
                         # Q2_K / Q3_K: the restatement behind the expectation takes seconds per token at 14336 rows
                         [(Q3, 4096, 14336, (1,)), (Q3, 512, 768, (1, 65)), (Q2, 512, 768, (7, 129))])
def test_batch_silu_mul(bamd, po, t, K, rows, Ts):
    """h = silu(gate) * up: one integer-dot launch over the pair (impl 0), or gate then up with the product as the second launch's in-place epilogue (impl 2,
    res == out; Q2_K / Q3_K pairs fall to the integer-dot launch there)"""
    for T in Ts:
        rng, X, w = batch_inputs(K, T, t)
        Wg, Wu = random_kquant_tensor(t, K, rows, rng, amp=4.0), random_kquant_tensor(t, K, rows, rng, amp=4.0)
        A = np.stack([normed(po, x, w) for x in X])
        want = silu_mul(po, ref_mul_mat(po, t, Wg, rows, K, A), ref_mul_mat(po, t, Wu, rows, K, A))
        for impl in (0, 2):
            got = bamd.op_mul_mat_batch_seg([(t, Wg, rows), (t, Wu, rows)], K, X, rows + 64, epi=SILU_MUL, norm_w=w, eps=EPS, impl=impl, fill=FILL)
            assert_bits(got[:, :rows], want, "batched silu(gate) * up type %d K %d T %d impl %d" % (t, K, T, impl))
            assert (got[:, rows:] == FILL).all(), "impl %d wrote behind the rows" % impl
