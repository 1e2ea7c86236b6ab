"""The decomposition the F32 / F16 matrix-core prompt kernel (booster_amd/csrc/bamd_prefill2_flt.hip) computes, written in numpy with the exact f32 fma that
tests/float_ref.py uses, against the genuine reference's stored answers (tests/golden/float_kats.npz, the *_sgemm1 keys) and the restatement float_ref.mul_mat.
No GPU: this pins the index arithmetic of the mapping.

  an output tile is EIGHT accumulator tiles, one per lane j of the reference's 8-lane accumulator;
  MFMA step s of tile j is the four-link chain  C <- fma(a3, b3, fma(a2, b2, fma(a1, b1, fma(a0, b0, C))))  with link kk at k = 32 s + 8 kk + j, chained through
  C in the order of s (no split over K);
  after the last step the eight tiles are summed element-wise in the tree of hsum(__m256): t[m] = c[m] + c[m + 4], (t0 + t2) + (t1 + t3)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float_ref as fr  # noqa: E402
from lowbit_ref import fma32  # noqa: E402
from test_float_ref import bits, cases, stored  # noqa: E402,F401  (stored: fixture)


def mfma_16x16x4(a, b, c):
    """v_mfma_f32_16x16x4_f32 on whole operand blocks: a [rows][4], b [4][tokens], c [rows][tokens] -> the sequential chain over kk = 0..3"""
    for kk in range(4):
        c = fma32(a[:, kk, None], b[None, kk, :], c)
    return c


def mfma_mul_mat(t, raw, rows, K, X):
    """Y [tokens][rows] of W . x_t by the kernel's decomposition"""
    w = fr.to_f32(t, np.asarray(raw, np.uint8)[:rows * K * fr.ESIZE[t]]).reshape(rows, K)      # F16: widened exactly
    X = np.ascontiguousarray(X, np.float32)                                                     # activations: never rounded
    T = X.shape[0]
    tiles = [np.zeros((rows, T), np.float32) for _ in range(8)]
    for s in range(K // 32):
        for j in range(8):
            k = 32 * s + 8 * np.arange(4) + j
            tiles[j] = mfma_16x16x4(w[:, k], X[:, k].T, tiles[j])
    with np.errstate(all="ignore"):
        tt = [tiles[m] + tiles[m + 4] for m in range(4)]
        y = ((tt[0] + tt[2]) + (tt[1] + tt[3])).astype(np.float32)
    return y.T


@pytest.mark.parametrize("t", fr.SGEMM_TYPES)
def test_decomposition_equals_the_stored_outputs(stored, t):
    """every stored F16 / F32 case, the edge matrix x edge vectors included (subnormal weights and activations, products and partial sums below 2^-126)"""
    for key, raw, xs, digest in cases(t):
        assert str(stored[key + "_inputs_sha256"]) == digest
        want = stored[key + "_sgemm1"]
        assert np.isfinite(want).all()
        got = mfma_mul_mat(t, raw, fr.ROWS, xs[0].size, np.stack(xs))
        assert np.array_equal(bits(got), bits(want)), key


@pytest.mark.parametrize("t", fr.SGEMM_TYPES)
@pytest.mark.parametrize("K", [256, 768, 14336])
def test_decomposition_equals_the_restatement(t, K):
    """one record, an odd record count, the 8B ffn_down (448 chained steps per tile)"""
    from booster_amd.gguf import random_float_tensor
    rows, T = 8, 3
    rng = np.random.default_rng(31 * K + t)
    W = random_float_tensor(t, K, rows, rng, amp=4.0)
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    want = np.stack([fr.mul_mat(t, W, rows, K, x) for x in X])
    assert np.isfinite(want).all() and np.abs(want).max() > 0
    assert np.array_equal(bits(mfma_mul_mat(t, W, rows, K, X)), bits(want))


def test_a_split_over_k_would_move_bits():
    """two half-chains added at the end are not the chain: the decomposition above must stay unsplit"""
    from booster_amd.gguf import random_float_tensor
    K, rows = 512, 8
    rng = np.random.default_rng(5)
    W = random_float_tensor(fr.F32, K, rows, rng, amp=4.0)
    x = (rng.standard_normal((1, K)) * 3).astype(np.float32)
    w = fr.to_f32(fr.F32, W).reshape(rows, K)
    whole = mfma_mul_mat(fr.F32, W, rows, K, x)
    halves = mfma_mul_mat(fr.F32, fr.encode(fr.F32, w[:, :256]), rows, 256, x[:, :256]) + mfma_mul_mat(fr.F32, fr.encode(fr.F32, w[:, 256:]), rows, 256, x[:, 256:])
    assert not np.array_equal(bits(whole), bits(halves))
