"""GPU: the mode-A launches whose RMSNorm prologue requests the second half of the weight ring request by request at its stage points (ActPro's staged
`mid`, BAMD_RING_DRIP: bamd_device.h, bamd_matvec_core.h), raw bits against the CPU references: the oracle for Q4_K / Q5_K / Q6_K, the numpy restatement
of tests/lowbit_ref.py for Q3_K / Q2_K.  A request dealt to the wrong ring slot, issued twice or left out puts a wrong record into one slot of one wave's
ring: a wrong row in that wave's rows.  The five types take two (Q4_K), three (Q5_K, Q2_K), four (Q6_K) and six (Q3_K) requests per record, and so every
deal of the requests over the stage points.
  test_gateup7_three_calls      rows 14336, K 4096 (matvec_gateup7_kernel on 256 CUs), five types, three launches with the same weights: every row,
                                reported for the rows of waves 0-3 (whole pairs), of waves 4-6 (short pairs) separately; the helper wave's quarters are
                                the tails of the chains of waves 4-6, so a wrong record there shows in those rows
  test_lm_head_guard_path       Q6_K, K 4096, rows 16392 (2049 row-groups: mode A, one wave slot with a second row-group) through the lm_head op
                                with the arg-max epilogue, on the constructed activation vector whose sum of squares trips the f64-order guard
                                (tests/test_f64_order.py): the rare path with two more barriers between the stage points
  test_gateup14_three_calls     rows 28672, K 8192, Q4_K (matvec_gateup14_kernel: four activation batch slots per wave), three launches
The gate/up references of K 4096 are those of tests/test_gpu_gateup_tail.py (built once per type and shared)."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from bitcheck import EPS, assert_bits, bits
from test_gpu_gateup_tail import NT, ROWS, SHORT0, case

sys.path.insert(0, os.path.join(ROOT, "tools"))
pytestmark = pytest.mark.gpu
TYPES = [10, 11, 12, 13, 14]                                 # Q2_K, Q3_K, Q4_K, Q5_K, Q6_K
K = 4096


@pytest.mark.parametrize("t", TYPES)
def test_gateup7_three_calls(bamd, po, t):
    c = case(po, t)
    assert ROWS == 7 * 8 * 256 and SHORT0 == 4 * 8 * 256     # seven pairs per workgroup on 256 CUs; waves 4-6 own the rows from SHORT0 on
    for i, x in enumerate(c["xs"]):
        got = bamd.op_ffn_gate_up(t, c["Wg"], c["Wu"], ROWS, K, x, norm_w=c["w"], eps=EPS)
        want = po.silu(c["g"][i]) * c["u"][i]
        assert_bits(got[:SHORT0], want[:SHORT0], "gate/up type %d, call %d, rows of waves 0-3" % (t, i))
        assert_bits(got[SHORT0:], want[SHORT0:], "gate/up type %d, call %d, rows of waves 4-6 (last quarters: helper wave)" % (t, i))


def argmax_keys(v):
    """argmax_key of bamd_device.h for rows 0 .. n-1: order-preserving bits of the value above the complemented row (the lowest row wins a tie)"""
    u = bits(v).astype(np.uint64)
    u = np.where(u & 0x80000000, ~u & 0xffffffff, u | 0x80000000)
    return (u << np.uint64(32)) | (np.uint64(0xffffffff) - np.arange(u.size, dtype=np.uint64))


def test_lm_head_guard_path(bamd, po):
    import f64_order_search as fs
    from booster_amd.gguf import random_kquant_tensor
    kat = np.load(os.path.join(GOLDEN, "f64_order_kat.npz"))
    x, eps = kat["x"], float(kat["eps"])
    assert x.size == K and fs.guarded_mean32(fs.terms(x))[1]                # the guard fires: the sequential recomputation runs
    rows = 16392                                                             # 2049 row-groups > 8 waves x 256 workgroups
    rng = np.random.default_rng(14 * K + rows)
    W = random_kquant_tensor(14, K, rows, rng, amp=4.0)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    act = (po.rms_norm(x, eps) * w).astype(np.float32)
    want = po.mul_mat_q(14, W, rows, K, act, nthreads=NT)[0]
    got, row = bamd.op_mul_mat_vec_argmax(14, W, rows, K, x, norm_w=w, eps=eps)
    assert_bits(got, want, "lm_head logits, Q6_K, %d rows, guard path" % rows)
    keys = argmax_keys(want)
    assert row == int(np.argmax(want)) and argmax_keys(got)[row] == keys.max()


def test_gateup14_three_calls(bamd, po):
    from booster_amd.gguf import random_kquant_tensor
    t, k, rows = 12, 8192, 28672                              # fourteen pairs per workgroup on 256 CUs
    rng = np.random.default_rng(5 * t + k)
    Wg = random_kquant_tensor(t, k, rows, rng, amp=4.0)
    Wu = random_kquant_tensor(t, k, rows, rng, amp=4.0)
    w = (1 + 0.1 * rng.standard_normal(k)).astype(np.float32)
    for i, s in enumerate((2.0, 0.5, 8.0)):
        x = (rng.standard_normal(k) * s).astype(np.float32)
        act = (po.rms_norm(x, EPS) * w).astype(np.float32)
        want = po.silu(po.mul_mat_q(t, Wg, rows, k, act, nthreads=NT)[0]) * po.mul_mat_q(t, Wu, rows, k, act, nthreads=NT)[0]
        got = bamd.op_ffn_gate_up(t, Wg, Wu, rows, k, x, norm_w=w, eps=EPS)
        assert_bits(got, want, "gate/up Q4_K, K %d, %d rows, call %d" % (k, rows, i))
