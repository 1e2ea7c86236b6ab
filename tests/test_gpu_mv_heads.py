"""GPU: the heads of the split-K decode mat-vec launches — activation requests, weight-ring requests, prologue, and every record waiting for its own loads —
at the shapes whose machine code profiles/mv_heads.txt examines: the fused QKV kernels, whose prologue takes the wave count as a constant and no longer
waits for ring loads, and the ffn_down kernels, whose order of requests was examined and left.  Raw bits against the CPU references: the oracle for
Q4_K / Q5_K / Q6_K, and for Q3_K / Q2_K, which the oracle does not have, the numpy restatement that tests/test_lowbit_ref.py holds to the reference's stored
outputs (tests/lowbit_ref.py).

A wait that became too short shows as stale or half-landed data, so every case runs THREE calls in one process, same weights, different activations, and
compares every output element of each.  The second activation vector holds an all-zero 256-block and a block whose largest magnitude is negative.  Every
case first asks booster_amd.trace_matvec which kernel the launch takes (256 CUs), so that it cannot pass on another family:
  test_ffn_down_14_waves    K = 14336 with a residual, matvec_split_fast_kernel on fourteen waves: 64 rows (one row-group per workgroup) and 2107 valid rows of
                            2112 (264 row-groups on 256 CUs: eight workgroups take a second batch through the real refill, the others go through the
                            zero-record descriptor; rows 2107 .. 2111 cross the nvalid edge)
  test_ffn_down_k28672      K = 28672 with a residual, sixteen waves x seven records, compact term buffers: 64 rows
  test_fused_qkv            K = 4096, rows 5120 + 1024, matvec_split_mixed_kernel: three type pairs, and one segment of 6144 rows of a single type
The references of a case are computed once and shared by its three calls."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import lowbit_ref as lr
import booster_amd
from bitcheck import assert_bits
from booster_amd.gguf import random_kquant_tensor

pytestmark = pytest.mark.gpu
EPS = 1e-5
NT = 8
BLOCK_BYTES = {10: 84, 11: 110, 12: 144, 13: 176, 14: 210}
PRO_PLAIN, PRO_NORM, EPI_STORE, EPI_ADD = 0, 1, 0, 1
ZERO_BLOCK, NEG_BLOCK = 3, 6                                 # of the second activation vector


def ref_mv(po, t, W, rows, k, a):
    """W . Q8_K(a) as the reference computes it: float32 [rows]"""
    if t in (lr.Q2_K, lr.Q3_K):                              # lr.vec_dot_rows, its row chunks spread over threads (numpy releases the lock in its kernels)
        rb = k // 256 * BLOCK_BYTES[t]
        q8 = po.quantize_q8_K(np.ascontiguousarray(a, np.float32))
        with ThreadPoolExecutor(NT) as ex:
            return np.concatenate(list(ex.map(lambda r: lr.vec_dot_rows(t, W[r * rb:min(rows, r + 256) * rb], q8), range(0, rows, 256))))
    return po.mul_mat_q(t, W, rows, k, a, nthreads=NT)[0]


def activations(rng, k):
    """three vectors of different scale; the second with an all-zero block and a block whose largest magnitude is a negative element"""
    xs = [(rng.standard_normal(k) * s).astype(np.float32) for s in (2.0, 0.5, 8.0)]
    xs[1][ZERO_BLOCK * 256:(ZERO_BLOCK + 1) * 256] = 0.0
    blk = xs[1][NEG_BLOCK * 256:(NEG_BLOCK + 1) * 256]
    blk[17] = -4.0 * np.abs(blk).max()
    assert blk.max() < -blk.min() and not xs[1][ZERO_BLOCK * 256:(ZERO_BLOCK + 1) * 256].any()
    return xs


_DOWN = {}


def down_case(po, t, k, rows):
    """weights, residual, three activation vectors and the expected outputs of W . Q8_K(x) + residual: built once, never modified"""
    if (t, k, rows) not in _DOWN:
        rng = np.random.default_rng(7 * t + k + rows)
        W = random_kquant_tensor(t, k, rows, rng, amp=4.0)
        res = rng.standard_normal(rows).astype(np.float32)
        xs = activations(rng, k)
        want = [ref_mv(po, t, W, rows, k, x) + res for x in xs]
        for v in (W, res, *xs, *want):
            v.setflags(write=False)
        _DOWN[(t, k, rows)] = dict(W=W, res=res, xs=xs, want=want)
    return _DOWN[(t, k, rows)]


def check_down(bamd, po, t, k, rows, kernel, block, grid):
    tr = booster_amd.trace_matvec([(t, rows)], k, PRO_PLAIN, EPI_ADD)
    assert tr is not None and kernel in tr["kernel"] and tr["block"] == [block, 1, 1] and tr["grid"] == [grid, 1, 1], tr
    c = down_case(po, t, k, rows)
    for i, x in enumerate(c["xs"]):
        got = bamd.op_mul_mat_vec(t, c["W"], rows, k, x, residual=c["res"])
        assert_bits(got, c["want"][i], "ffn_down type %d, K %d, %d rows, call %d" % (t, k, rows, i))


@pytest.mark.parametrize("rows", [64, 2107])
@pytest.mark.parametrize("t", [10, 11, 12, 13, 14])          # Q2_K, Q3_K, Q4_K, Q5_K, Q6_K
def test_ffn_down_14_waves(bamd, po, t, rows):
    check_down(bamd, po, t, 14336, rows, "matvec_split_fast_kernelILi%dELi4ELi1ELi0ELi1ELb0ELi14ELb0EE" % t, 14 * 64, min((rows + 7) // 8, 256))


@pytest.mark.parametrize("t", [12, 13, 14])
def test_ffn_down_k28672(bamd, po, t):
    check_down(bamd, po, t, 28672, 64, "matvec_split_fast_kernelILi%dELi7ELi1ELi0ELi1ELb0ELi16ELb1EE" % t, 16 * 64, 8)


QK_ROWS, V_ROWS, QKV_K = 5120, 1024, 4096
_QKV = {}


def qkv_case(po, ta, tb):
    if (ta, tb) not in _QKV:
        rng = np.random.default_rng(100 * ta + tb)
        W0 = random_kquant_tensor(ta, QKV_K, QK_ROWS, rng, amp=4.0)
        W1 = random_kquant_tensor(tb, QKV_K, V_ROWS, rng, amp=4.0)
        w = (1 + 0.1 * rng.standard_normal(QKV_K)).astype(np.float32)
        xs = activations(rng, QKV_K)
        acts = [(po.rms_norm(x, EPS) * w).astype(np.float32) for x in xs]
        assert not acts[1][ZERO_BLOCK * 256:(ZERO_BLOCK + 1) * 256].any()
        assert acts[1][NEG_BLOCK * 256:(NEG_BLOCK + 1) * 256].max() < -acts[1][NEG_BLOCK * 256:(NEG_BLOCK + 1) * 256].min()
        want = [np.concatenate([ref_mv(po, ta, W0, QK_ROWS, QKV_K, a), ref_mv(po, tb, W1, V_ROWS, QKV_K, a)]) for a in acts]
        for v in (W0, W1, w, *xs, *want):
            v.setflags(write=False)
        _QKV[(ta, tb)] = dict(W0=W0, W1=W1, w=w, xs=xs, want=want)
    return _QKV[(ta, tb)]


@pytest.mark.parametrize("ta,tb", [(12, 14), (12, 13), (13, 14), (12, 12), (14, 14)])
def test_fused_qkv(bamd, po, ta, tb):
    c = qkv_case(po, ta, tb)
    if ta == tb:                                             # wq | wk | wv of one type: the engine launches them as ONE segment
        segs = [(ta, np.concatenate([c["W0"], c["W1"]]), QK_ROWS + V_ROWS)]
    else:
        segs = [(ta, c["W0"], QK_ROWS), (tb, c["W1"], V_ROWS)]
    tr = booster_amd.trace_matvec([(t, r) for t, _, r in segs], QKV_K, PRO_NORM, EPI_STORE)
    assert tr is not None and "matvec_split_mixed_kernelILi%dELi%dELi2ELi2ELb0ELi8EE" % (ta, tb) in tr["kernel"] and tr["grid"] == [256, 1, 1], tr
    for i, x in enumerate(c["xs"]):
        got = bamd.op_fused_qkv(segs, QKV_K, x, c["w"], eps=EPS)
        assert_bits(got, c["want"][i], "fused QKV types (%d, %d), call %d" % (ta, tb, i))
