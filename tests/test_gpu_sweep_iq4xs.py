"""GPU: the seeded shape sweep of tests/test_gpu_sweep_families.py for IQ4_XS.  The case lists come from the generators of tests/family_cases.py (seeded per
type: every list is the same on every machine and every case is a pytest id): one draw from every K class — one record, odd record counts, the depth-2 ring
refilling inside a row, depth 4 — and as many uniform draws; gate/up and arg-max at ragged rows; more row-groups than the grid has waves; the batch kernel on
both sides of its token-tile switch.  Every expectation is the numpy restatement that tests/test_iq4xs_ref.py holds to the genuine reference's outputs; bit
equality throughout, every expectation finite and not all zero.  No case is skipped."""
import numpy as np
import pytest

import family_cases as fc
import iq4xs_ref as xr
from bitcheck import EPS, assert_bits, normed, silu_mul
from booster_amd.gguf import random_iq4_xs_tensor
from test_gpu_sweep_families import activation, norm_weight

pytestmark = pytest.mark.gpu
T = xr.IQ4_XS
MODES = (0, 1, 2)                                # split-K exists for the type (the K-quant kernels); a mode-2 request without a split shape falls to mode A
F = fc.Family("IQ4_XS", lambda t, K, rows, rng, amp=1.0: random_iq4_xs_tensor(K, rows, rng, amp), lambda po, t, W, rows, K, x: xr.mul_mat(po, W, rows, K, x), "q8_K", MODES, None)


def ids(cases):
    fmt = (("i", "%d"), ("K", "K%d"), ("rows", "r%d"), ("T", "T%d"), ("epi", "%s"))
    return ["-".join(["IQ4_XS"] + [f % getattr(c, k) for k, f in fmt if hasattr(c, k)]) for c in cases]


def want_of(po, W, rows, K, a):
    y = xr.mul_mat(po, W, rows, K, a)
    assert np.isfinite(y).all() and np.any(y != 0), "the expectation is finite and not all zero"
    return y


def plant_tie(po, W, rows, K, a, tied):
    """test_gpu_sweep_families.plant_tie for this type: the row with the largest logit moved into the rows `tied`; the matrix and its expectation"""
    W = W.reshape(rows, -1).copy()
    want = want_of(po, W.reshape(-1), rows, K, a)
    top = int(np.argmax(want))
    free = np.setdiff1d(np.arange(rows), tied)
    bottom = int(free[np.argmin(want[free])])
    best, peak = W[top].copy(), want[top]
    if top not in tied:
        W[top] = W[bottom]; want[top] = want[bottom]
    W[tied] = best; want[tied] = peak
    assert np.flatnonzero(want == want.max()).tolist() == sorted(tied)
    return W.reshape(-1), want


MATVEC = fc.matvec_cases(T)


@pytest.mark.parametrize("c", MATVEC, ids=ids(MATVEC))
def test_mul_mat_vec_sweep(bamd, po, c):
    rng = np.random.default_rng([7100, c.t, c.i])
    W = F.gen(c.t, c.K, c.rows, rng, float(10 ** rng.uniform(-1, 1)))
    x = activation(rng, c.K, c.i)
    w = norm_weight(rng, c.K) if c.norm else None
    res = rng.standard_normal(c.rows).astype(np.float32) if c.resid else None
    want = want_of(po, W, c.rows, c.K, x if w is None else normed(po, x, w))
    if res is not None:
        want = want + res
    for mode in MODES:
        got = bamd.op_mul_mat_vec(c.t, W, c.rows, c.K, x, norm_w=w, eps=EPS, residual=res, mode=mode)
        assert_bits(got, want, "IQ4_XS K %d rows %d norm %d residual %d mode %d" % (c.K, c.rows, c.norm, c.resid, mode))


GATEUP = fc.gateup_cases(T)
ARGMAX = fc.argmax_cases(T)


@pytest.mark.parametrize("c", GATEUP, ids=ids(GATEUP))
def test_ffn_gate_up_sweep(bamd, po, c):
    rng = np.random.default_rng([7200, c.t, c.i])
    Wg = F.gen(c.t, c.K, c.rows, rng, 4.0)
    Wu = F.gen(c.t, c.K, c.rows, rng, 4.0)
    x = (rng.standard_normal(c.K) * 2).astype(np.float32)
    w = norm_weight(rng, c.K)
    a = normed(po, x, w)
    want = silu_mul(po, want_of(po, Wg, c.rows, c.K, a), want_of(po, Wu, c.rows, c.K, a))
    assert_bits(bamd.op_ffn_gate_up(c.t, Wg, Wu, c.rows, c.K, x, norm_w=w, eps=EPS), want, "gate/up IQ4_XS K %d rows %d" % (c.K, c.rows))


@pytest.mark.parametrize("c", ARGMAX, ids=ids(ARGMAX))
def test_argmax_sweep(bamd, po, c):
    rng = np.random.default_rng([7300, c.t, c.i])
    W = F.gen(c.t, c.K, c.rows, rng, 4.0)
    x = (rng.standard_normal(c.K) * 2).astype(np.float32)
    w = norm_weight(rng, c.K)
    nrg = (c.rows + 7) // 8
    tied = [8 * (nrg // 3) + 5, c.rows - 1]
    assert (tied[0] // 8) % min(fc.GRID, nrg) != (tied[1] // 8) % min(fc.GRID, nrg), "the tied rows belong to different workgroups"
    W, want = plant_tie(po, W, c.rows, c.K, normed(po, x, w), tied)
    got, row = bamd.op_mul_mat_vec_argmax(c.t, W, c.rows, c.K, x, norm_w=w, eps=EPS, mode=0)
    assert_bits(got, want, "arg-max logits IQ4_XS K %d rows %d" % (c.K, c.rows))
    assert row == tied[0], "the lower of the tied rows"


TALL = fc.tall_cases(T)


@pytest.mark.parametrize("c", TALL, ids=ids(TALL))
def test_tall_matrix_more_row_groups_than_wave_slots(bamd, po, c):
    """2049 and 4099 row-groups on 2048 wave slots: a wave's second and third row-group in mode A — residual add, gate/up, arg-max with the top tied between a
    row that only a second walk reaches and the last valid row"""
    rng = np.random.default_rng([7500, c.t, c.K])
    x = (rng.standard_normal(c.K) * 2).astype(np.float32)
    what = "tall IQ4_XS K %d row-groups %d %s" % (c.K, c.nrg, c.epi)
    if c.epi == "add":
        W = F.gen(c.t, c.K, c.rows, rng)
        res = rng.standard_normal(c.rows).astype(np.float32)
        assert_bits(bamd.op_mul_mat_vec(c.t, W, c.rows, c.K, x, residual=res, mode=1), want_of(po, W, c.rows, c.K, x) + res, what)
    elif c.epi == "gateup":
        w = norm_weight(rng, c.K)
        a = normed(po, x, w)
        Wg = F.gen(c.t, c.K, c.rows, rng, 4.0)
        Wu = F.gen(c.t, c.K, c.rows, rng, 4.0)
        want = silu_mul(po, want_of(po, Wg, c.rows, c.K, a), want_of(po, Wu, c.rows, c.K, a))
        assert_bits(bamd.op_ffn_gate_up(c.t, Wg, Wu, c.rows, c.K, x, norm_w=w, eps=EPS), want, what)
    else:
        w = norm_weight(rng, c.K)
        tied = [8 * fc.WAVE_SLOTS + 1, c.rows - 1]
        W, want = plant_tie(po, F.gen(c.t, c.K, c.rows, rng, 4.0), c.rows, c.K, normed(po, x, w), tied)
        got, row = bamd.op_mul_mat_vec_argmax(c.t, W, c.rows, c.K, x, norm_w=w, eps=EPS, mode=1)
        assert_bits(got, want, what)
        assert row == tied[0], what + ": the lower of the tied rows"


BATCH = fc.batch_cases(T)


@pytest.mark.parametrize("c", BATCH, ids=ids(BATCH))
def test_mul_mat_batch_sweep(bamd, po, c):
    """the integer-dot batch kernel against the restatement for the first, the middle and the last token; the type has no matrix-core kernel: impl 2 is refused"""
    rng = np.random.default_rng([7600, c.t, c.i])
    W = F.gen(c.t, c.K, c.rows, rng, float(10 ** rng.uniform(-1, 1)))
    X = (rng.standard_normal((c.T, c.K)) * 10 ** rng.uniform(-1, 1)).astype(np.float32)
    w = norm_weight(rng, c.K) if c.norm else None
    res = rng.standard_normal((c.T, c.rows)).astype(np.float32) if c.resid else None
    what = "batch IQ4_XS K %d rows %d T %d norm %d residual %d" % (c.K, c.rows, c.T, c.norm, c.resid)
    plain = bamd.op_mul_mat_batch(c.t, W, c.rows, c.K, X, norm_w=w, eps=EPS, residual=res, impl=0)
    for tok in sorted({0, c.T // 2, c.T - 1}):
        want = want_of(po, W, c.rows, c.K, X[tok] if w is None else normed(po, X[tok], w))
        assert_bits(plain[tok], want if res is None else want + res[tok], what + " token %d" % tok)
    with pytest.raises(bamd.BamdError, match="MFMA path: unsupported type/shape"):
        bamd.op_mul_mat_batch(c.t, W, c.rows, c.K, X, norm_w=w, eps=EPS, residual=res, impl=2)
