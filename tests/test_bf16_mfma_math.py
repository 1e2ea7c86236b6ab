"""The decomposition the BF16 matrix-core prompt kernel (booster_amd/csrc/bamd_prefill2_bf16.hip) computes and the guard it runs behind, written in numpy
with the exact f32 fma that tests/float_ref.py uses, against the genuine reference's stored answers (tests/golden/float_kats.npz, the bf16_*_dots keys) and the
restatement float_ref.mul_mat.  No GPU: this pins the index arithmetic of the mapping and the arithmetic of the guard.

  an output tile is 32 accumulator tiles, one per chain lane c = 8 a + j of ggml_vec_dot_bf16's four 8-lane accumulators;
  MFMA step s of tile c is the four-link chain  C <- fma(a3, b3, fma(a2, b2, fma(a1, b1, fma(a0, b0, C))))  with link kk at k = 32 (4 s + kk) + c, chained
  through C in the order of s (no split over K);
  after the last step the tiles are combined element-wise: (c1 + c3) + (c2 + c4) over a, then the tree of hsum(__m256) over j.

The reference's chain is add(mul(w, x), c), two roundings.  The fma chain equals it wherever every product is exact in f32; the guard proves that from exponent
ranges: with E = (h >> 7) & 0xff and e = max(E, 1) - 127 of a bf16 pattern h, a value is an integer of fewer than 8 bits times 2^(e - 7), a product an integer of
at most 16 bits times 2^(e_w + e_x - 14) — exact iff that unit is >= 2^-149 and the magnitude stays under 2^128."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float_ref as fr  # noqa: E402
from lowbit_ref import fma32  # noqa: E402
from test_float_ref import bits, stored  # noqa: E402,F401  (stored: fixture)

BF16 = fr.BF16


def guard(w_bits, x_bits):
    """sufficient for "every product of a weight and an activation is exact in f32": emin_w + emin_x >= -135 over the nonzero values, emax_w + emax_x <= 126,
    no E == 255 on either side; a side without a nonzero value is safe"""
    def rng(h):
        h = np.asarray(h, np.uint16).astype(np.int64).reshape(-1)
        E = (h >> 7) & 0xff
        if (E == 255).any():
            return None
        e = np.maximum(E, 1)[(h & 0x7fff) != 0] - 127
        return (int(e.min()), int(e.max())) if e.size else ()
    w, x = rng(w_bits), rng(x_bits)
    if w is None or x is None:
        return False
    if w == () or x == ():
        return True
    return w[0] + x[0] >= -135 and w[1] + x[1] <= 126


def mfma_16x16x4(a, b, c):
    """v_mfma_f32_16x16x4_f32 on whole operand blocks: a [rows][4], b [4][tokens], c [rows][tokens] -> the sequential chain over kk = 0..3"""
    for kk in range(4):
        c = fma32(a[:, kk, None], b[None, kk, :], c)
    return c


def mfma_mul_mat(raw, rows, K, X):
    """Y [tokens][rows] of W . bf16(x_t) by the kernel's decomposition, fma throughout"""
    w = fr.to_f32(BF16, np.asarray(raw, np.uint8)[:rows * K * 2]).reshape(rows, K)
    xb = np.stack([fr.bf16_to_f32(fr.bf16_bits(x)) for x in np.ascontiguousarray(X, np.float32)])
    T = xb.shape[0]
    tiles = [np.zeros((rows, T), np.float32) for _ in range(32)]
    with np.errstate(all="ignore"):
        for s in range(K // 128):
            for c in range(32):
                k = 32 * (4 * s + np.arange(4)) + c
                tiles[c] = mfma_16x16x4(w[:, k], xb[:, k].T, tiles[c])
        lane = [(tiles[j] + tiles[16 + j]) + (tiles[8 + j] + tiles[24 + j]) for j in range(8)]
        tt = [lane[m] + lane[m + 4] for m in range(4)]
        y = ((tt[0] + tt[2]) + (tt[1] + tt[3])).astype(np.float32)
    return y.T


def bf16_cases():
    return list(fr.all_cases(BF16))


def test_decomposition_equals_the_stored_outputs_where_the_guard_passes(stored):
    """the twelve bf16_K* vectors: all pass the guard, and the fma decomposition gives the genuine reference's bits"""
    n = 0
    for key, raw, xs, digest in bf16_cases():
        if key == "bf16_edge":
            continue
        assert str(stored[key + "_inputs_sha256"]) == digest
        want = stored[key + "_dots"]
        assert np.isfinite(want).all()
        for x in xs:
            assert guard(raw.view(np.uint16), fr.bf16_bits(x)), key
            n += 1
        assert np.array_equal(bits(mfma_mul_mat(raw, fr.ROWS, xs[0].size, np.stack(xs))), bits(want)), key
    assert n == 12


def test_edge_vectors_fail_the_guard_and_the_fused_chain_misses_them(stored):
    """the six bf16_edge vectors all fail the guard, and for at least one of them the fma decomposition is NOT the stored answer: a kernel without the guard
    cannot pass them (the two-rounding restatement does: tests/test_float_ref.py)"""
    (key, raw, xs, digest), = [c for c in bf16_cases() if c[0] == "bf16_edge"]
    assert str(stored[key + "_inputs_sha256"]) == digest
    want = stored[key + "_dots"]
    assert np.isfinite(want).all() and len(xs) == 6
    for x in xs:
        assert not guard(raw.view(np.uint16), fr.bf16_bits(x))
    got = mfma_mul_mat(raw, fr.ROWS, fr.EDGE_K, np.stack(xs))
    differ = [i for i in range(6) if not np.array_equal(bits(got[i]), bits(want[i]))]
    assert differ, "the fused chain gives the stored answers of every edge vector: the edge case has no teeth"
    unfused = np.stack([fr.mul_mat(BF16, raw, fr.ROWS, fr.EDGE_K, x) for x in xs])
    assert np.array_equal(bits(unfused), bits(want))


@pytest.mark.parametrize("K", [256, 768, 14336])
def test_decomposition_equals_the_restatement(K):
    """one record, an odd record count, the 8B ffn_down (112 chained steps per tile)"""
    from booster_amd.gguf import random_float_tensor
    rows, T = 8, 3
    rng = np.random.default_rng(31 * K + BF16)
    W = random_float_tensor(BF16, K, rows, rng, amp=4.0)
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    assert all(guard(W.view(np.uint16), fr.bf16_bits(x)) for x in X)
    want = np.stack([fr.mul_mat(BF16, W, rows, K, x) for x in X])
    assert np.isfinite(want).all() and np.abs(want).max() > 0
    assert np.array_equal(bits(mfma_mul_mat(W, rows, K, X)), bits(want))


# ---- the boundaries of the guard ------------------------------------------------------------------------------------------------------------------
def _val(m, e):
    """the bf16 value m * 2^(e - 7) (128 <= m < 256: a normal pattern with e = E - 127), as f32 and as its pattern"""
    v = np.float32(m) * np.float32(2.0) ** np.float32(e - 7)
    h = fr.bf16_bits(np.array([v], np.float32))
    assert fr.bf16_to_f32(h)[0] == v and ((int(h[0]) >> 7) & 0xff) - 127 == e
    return v, h


def _both(w, x, acc):
    with np.errstate(all="ignore"):
        unfused = (np.float32(w) * np.float32(x)).astype(np.float32) + np.float32(acc)
    return bits(fma32(np.array([w], np.float32), np.array([x], np.float32), np.array([acc], np.float32)))[0], bits(np.array([unfused], np.float32))[0]


def test_guard_boundary_at_the_bottom():
    """e_w + e_x = -135 with an odd product integer: the unit is 2^-149, the product exact, fused and unfused agree for any accumulator.  One lower, the
    product is an odd multiple of 2^-150 — a tie — and an accumulator of 2^-149 flips which neighbour is even: the bits differ"""
    ulp = np.float32(2.0) ** np.float32(-149)
    w, hw = _val(129, -75)
    x, hx = _val(131, -60)
    assert (129 * 131) & 1 and guard(hw, hx)
    for acc in (0.0, ulp, -ulp, 3 * ulp, np.float32(1e-40), np.float32(-1.5e-38), np.float32(1.0)):
        f, u = _both(w, x, acc)
        assert f == u, acc
    w, hw = _val(129, -76)
    assert not guard(hw, hx)
    f, u = _both(w, x, ulp)
    assert f != u
    # (and subnormal patterns count with e = -126: the smallest subnormal weight against 2^-9 is the same boundary)
    sub = np.array([1], np.uint16)
    assert guard(sub, _val(128, -9)[1]) and not guard(sub, _val(128, -10)[1])


def test_guard_boundary_at_the_top():
    """emax_w + emax_x = 126: the largest such product, 255 * 255 * 2^112, is finite and exact — equal bits; one higher and the guard refuses (the product of
    the largest patterns would pass 2^128)"""
    w, hw = _val(255, 63)
    x, hx = _val(255, 63)
    assert guard(hw, hx)
    for acc in (0.0, np.float32(-3e38), np.float32(1e30)):
        f, u = _both(w, x, acc)
        assert f == u and np.isfinite(np.array([f], np.uint32).view(np.float32)[0])
    assert not guard(hw, _val(255, 64)[1])
    inf = fr.bf16_bits(np.array([np.inf], np.float32))
    assert not guard(inf, hx) and not guard(hw, inf) and not guard(inf, np.zeros(4, np.uint16))
    assert guard(np.zeros(4, np.uint16), _val(255, 127)[1]) and guard(_val(255, 127)[1], np.array([0, 0x8000], np.uint16))      # a side without a nonzero value


def test_a_split_over_k_would_move_bits():
    """two half-chains added at the end are not the chain: the decomposition above must stay unsplit"""
    from booster_amd.gguf import random_float_tensor
    K, rows = 512, 8
    rng = np.random.default_rng(5)
    W = random_float_tensor(BF16, K, rows, rng, amp=4.0)
    x = (rng.standard_normal((1, K)) * 3).astype(np.float32)
    w = W.view(np.uint16).reshape(rows, K)
    whole = mfma_mul_mat(W, rows, K, x)
    halves = mfma_mul_mat(np.ascontiguousarray(w[:, :256]).view(np.uint8).reshape(-1), rows, 256, x[:, :256]) + \
        mfma_mul_mat(np.ascontiguousarray(w[:, 256:]).view(np.uint8).reshape(-1), rows, 256, x[:, 256:])
    assert not np.array_equal(bits(whole), bits(halves))
