"""GPU: the seven-pair gate/up launch (matvec_gateup7_kernel, stream_pair_short) at the one shape that selects it on a 256-CU device, rows = 14336 and
K = 4096, for all five K-quant types, raw bits against the CPU references: the oracle for Q4_K / Q5_K / Q6_K, and for Q3_K / Q2_K, which the oracle does
not have, the numpy restatement that tests/test_lowbit_ref.py holds to the reference's stored outputs (tests/lowbit_ref.py).

Waves 4-6 of a workgroup finish their own three quarters of a gate/up pair, then replay the last-quarter terms that wave 7 parks in LDS as a per-pair
COUNT of parked records allows, SiLU of the gate value running ahead of the up row's last steps:
  test_three_calls_same_weights   every row of three launches in one process (same weights, different activations): a count that is not re-zeroed, or
                                  read stale, lets a wave replay the terms of the previous call or of a half-written quarter
  test_ragged_rows                14331 valid rows of 14336: the rows of pairs 4-6 of the last workgroups cross the nvalid edge
  test_silu_branches_short_pairs  gate values in every v_expf branch of SiLU in the rows that waves 4-6 own (row-groups b + 256 w, w = 4, 5, 6:
                                  rows 8192 and up), the recipe of tests/test_gpu_edges.py::test_ffn_gate_up_silu_branches
The references of a type are computed once and shared by the three tests."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import lowbit_ref as lr
from bitcheck import EPS, assert_bits
from booster_amd.gguf import random_kquant_tensor

pytestmark = pytest.mark.gpu
TYPES = [10, 11, 12, 13, 14]                                 # Q2_K, Q3_K, Q4_K, Q5_K, Q6_K
K, ROWS, RAGGED = 4096, 14336, 14331
SHORT0 = 4 * 256 * 8                                         # first row of a pair that waves 4-6 stream (256 workgroups x 8 rows per wave slot)
NT = 8
LOG2E = 1.4426950408889634
BLOCK_BYTES = {10: 84, 11: 110, 12: 144, 13: 176, 14: 210}
D_OFFSETS = {10: (80, 82), 11: (108,), 12: (0, 2), 13: (0, 2), 14: (208,)}   # f16 d (and dmin) of a super-block


def ref_mv(po, t, W, rows, a):
    """W . Q8_K(a) as the reference computes it: float32 [rows]"""
    if t in (lr.Q2_K, lr.Q3_K):                              # lr.mul_mat, its row chunks spread over threads (numpy releases the lock in its kernels)
        rb = K // 256 * BLOCK_BYTES[t]
        q8 = po.quantize_q8_K(np.ascontiguousarray(a, np.float32))
        with ThreadPoolExecutor(NT) as ex:
            return np.concatenate(list(ex.map(lambda r: lr.vec_dot_rows(t, W[r * rb:min(rows, r + 256) * rb], q8), range(0, rows, 256))))
    return po.mul_mat_q(t, W, rows, K, a, nthreads=NT)[0]


_CASES = {}


def case(po, t):
    """weights, RMSNorm weight, three activation vectors and the reference's gate and up values for each: built once per type, never modified"""
    if t not in _CASES:
        rng = np.random.default_rng(5 * t + K)
        Wg = random_kquant_tensor(t, K, ROWS, rng, amp=4.0)
        Wu = random_kquant_tensor(t, K, ROWS, rng, amp=4.0)
        w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
        xs = [(rng.standard_normal(K) * s).astype(np.float32) for s in (2.0, 0.5, 8.0)]
        acts = [(po.rms_norm(x, EPS) * w).astype(np.float32) for x in xs]
        g = [ref_mv(po, t, Wg, ROWS, a) for a in acts]
        u = [ref_mv(po, t, Wu, ROWS, a) for a in acts]
        for v in (Wg, Wu, w, *xs, *acts, *g, *u):
            v.setflags(write=False)
        _CASES[t] = dict(Wg=Wg, Wu=Wu, w=w, xs=xs, acts=acts, g=g, u=u)
    return _CASES[t]


def expf_branch(x):
    """the branch of ggml_v_expf an argument takes: 0 main, 1 |n| > 126 (scaled by 2^-+125: inf, or subnormal / 0), 2 |n| > 192"""
    n = np.abs(np.rint(np.asarray(x, np.float64) * LOG2E))
    return np.where(n > 192, 2, np.where(n > 126, 1, 0))


def scale_rows(t, W, rows, f):
    """multiply d (and dmin) of every super-block of row r by f[r], rounded to f16"""
    b = W.reshape(rows, K // 256, BLOCK_BYTES[t]).copy()
    for off in D_OFFSETS[t]:
        d = b[:, :, off:off + 2].copy().view(np.float16).astype(np.float64)
        b[:, :, off:off + 2] = (d * f[:, None, None]).astype(np.float16).view(np.uint8)
    return b.reshape(-1)


def silu_case(po, t):
    """(gate weights, expected output): d of each gate row from SHORT0 on scaled so that its gate value is log-uniform in +-[1e-3, 1e3], with 64 rows in
    each band of SiLU's exp(-g): g in (-133, -87.3), g < -133 (the overflow branch: a huge value or inf), g in (87.3, 133), g > 133 (subnormal or 0), g near 0"""
    c = case(po, t)
    rng = np.random.default_rng(900 + t)
    n = ROWS - SHORT0
    rb = K // 256 * BLOCK_BYTES[t]
    g0 = c["g"][0][SHORT0:].astype(np.float64)
    target = np.where(rng.random(n) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-3, 3, n)
    band = rng.permutation(n)[:320].reshape(5, 64)
    target[band[0]] = -rng.uniform(95, 125, 64)
    target[band[1]] = -rng.uniform(140, 900, 64)
    target[band[2]] = rng.uniform(95, 125, 64)
    target[band[3]] = rng.uniform(140, 900, 64)
    target[band[4]] = np.where(rng.random(64) < 0.5, -1.0, 1.0) * rng.uniform(1e-4, 1e-2, 64)
    f = np.where(np.abs(g0) > 1e-3, target / np.where(g0 == 0, 1.0, g0), 1.0)
    Ws = scale_rows(t, c["Wg"][SHORT0 * rb:], n, f)
    gs = ref_mv(po, t, Ws, n, c["acts"][0])
    assert np.isfinite(gs).all()
    for lo, hi in ((-133.0, -88.0), (-np.inf, -134.0), (88.0, 133.0), (134.0, np.inf), (-1e-2, 1e-2)):
        assert np.count_nonzero((gs > lo) & (gs < hi)) >= 32, "too few gate values in (%g, %g)" % (lo, hi)
    br = expf_branch(-gs)
    assert np.count_nonzero(br == 1) >= 64 and np.count_nonzero(br == 2) >= 64
    g = np.concatenate([c["g"][0][:SHORT0], gs])
    s = po.silu(g)
    assert np.count_nonzero((s[SHORT0:] == 0) & (gs < 0)) >= 64                                 # g / (1 + inf)
    return np.concatenate([c["Wg"][:SHORT0 * rb], Ws]), s * c["u"][0]


@pytest.mark.parametrize("t", TYPES)
def test_three_calls_same_weights(bamd, po, t):
    c = case(po, t)
    for i, x in enumerate(c["xs"]):
        got = bamd.op_ffn_gate_up(t, c["Wg"], c["Wu"], ROWS, K, x, norm_w=c["w"], eps=EPS)
        assert_bits(got, po.silu(c["g"][i]) * c["u"][i], "gate/up type %d, call %d" % (t, i))


@pytest.mark.parametrize("t", TYPES)
def test_ragged_rows(bamd, po, t):
    c = case(po, t)
    rb = K // 256 * BLOCK_BYTES[t]
    got = bamd.op_ffn_gate_up(t, c["Wg"][:RAGGED * rb], c["Wu"][:RAGGED * rb], RAGGED, K, c["xs"][1], norm_w=c["w"], eps=EPS)
    assert_bits(got, (po.silu(c["g"][1]) * c["u"][1])[:RAGGED], "gate/up type %d, %d valid rows" % (t, RAGGED))


@pytest.mark.parametrize("t", TYPES)
def test_silu_branches_short_pairs(bamd, po, t):
    Wg, want = silu_case(po, t)
    c = case(po, t)
    got = bamd.op_ffn_gate_up(t, Wg, c["Wu"], ROWS, K, c["xs"][0], norm_w=c["w"], eps=EPS)
    assert_bits(got, want, "gate/up type %d, SiLU branches in rows %d.." % (t, SHORT0))
