"""CPU: the arithmetic of the matrix-core prompt mat-mul for Q4_1 / Q5_1 weights (booster_amd/csrc/bamd_prefill2_b32.hip), checked before a GPU is involved.
As tests/test_legacy_mfma_math.py for the Q8_0 family: per 32-weight block l and SIMD lane e of the reference the kernel multiplies the f16 images of four
UNSIGNED weights (no offset: (0x6400 | u) - 1024 = u) and four int8 activations on the matrix cores and sums the four f32 products in whatever order the
instruction takes; the scale product, the eight chains in block order and the tree follow on the vector ALUs, and next to them ONE more chain per output,
summs = summs + f32(m_w) * f32(s_x) in block order, added to the tree at the end.  The operand images, the products, the four-term sums and the formulation as a
whole — with the summs step once as a multiply and an add and once as an fma — are held to the genuine reference's stored outputs
(tests/golden/legacy1_kats.npz), bit for bit.  The last test asks for the public switch of the feature in the built library and the header."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import legacy1_ref as l1
from lowbit_ref import fma32
from test_legacy1_ref import stored, stored_case  # noqa: F401  (stored: fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_every_operand_is_an_exact_float16():
    u = np.arange(32, dtype=np.uint16)                                           # Q4_1: 0..15, Q5_1: 0..31
    img = (np.uint16(0x6400) | u).view(np.float16)                              # the v_perm image: 1024 + u
    assert np.array_equal(img.astype(np.int64), 1024 + u.astype(np.int64))
    w = (img + np.float16(-1024.0)).astype(np.float16)                          # no further offset: the weights are unsigned
    assert np.array_equal(w.astype(np.int64), u.astype(np.int64))
    assert max(l1.QMAX.values()) == 31
    a = np.arange(-127, 128)
    assert np.array_equal(a.astype(np.float16).astype(np.int64), a)


def test_every_product_and_every_four_term_sum_is_exact_in_f32():
    w, x = np.meshgrid(np.arange(0, 32, dtype=np.int64), np.arange(-127, 128, dtype=np.int64), indexing="ij")          # all 32 x 255 operand pairs
    p = (w.astype(np.float16).astype(np.float32) * x.astype(np.float16).astype(np.float32)).astype(np.float32)
    assert p.shape == (32, 255) and np.array_equal(p.astype(np.int64), w * x)
    assert 4 * 31 * 127 < 2 ** 24
    # the extreme four-term sums, every order of the additions: partial sums are integers of magnitude <= 4 * 31 * 127, so nothing rounds
    ext = [np.float32(v) for v in (31 * 127, -31 * 127, 15 * 127, -15 * 127, 1, -1, 0)]
    for terms in itertools.product(ext, repeat=4):
        exact = int(sum(int(v) for v in terms))
        for order in itertools.permutations(range(4)):
            s = np.float32(0)
            for k in order:
                s = np.float32(s + terms[k])
            assert int(s) == exact
        assert int(np.float32(np.float32(terms[0] + terms[1]) + np.float32(terms[2] + terms[3]))) == exact


def mfma_formulation(t, raw, q8, rng, contracted):
    """float32 [rows]: the kernel's arithmetic in numpy — f16 operands, the four f32 products of a (block, e) link summed in a shuffled order, the f32 scale
    product, the eight chains in block order, the summs chain in block order (contracted: an fma; else a multiply, then an add), the tree plus summs"""
    yd, ys, qa = l1.q8_1_fields(q8)
    nb = yd.size
    wd, wm, wq = l1.unpack(t, raw)
    rows = wd.size // nb
    assert wq.min() >= 0 and wq.max() <= l1.QMAX[t]
    w16 = ((np.uint16(0x6400) | wq.astype(np.uint16)).view(np.float16) + np.float16(-1024.0)).astype(np.float16)
    assert np.array_equal(w16.astype(np.int64), wq)
    A = w16.astype(np.float32).reshape(rows, nb, 8, 4)
    B = qa.astype(np.float16).astype(np.float32).reshape(1, nb, 8, 4)
    prod = (A * B).astype(np.float32)
    dot4 = np.zeros((rows, nb, 8), np.float32)
    for k in rng.permutation(4):
        dot4 = (dot4 + prod[..., k]).astype(np.float32)
    wd = wd.reshape(rows, nb); wm = wm.reshape(rows, nb)
    acc = np.zeros((rows, 8), np.float32)
    summs = np.zeros(rows, np.float32)
    with np.errstate(all="ignore"):
        for l in range(nb):
            s = (wd[:, l] * yd[l]).astype(np.float32)
            acc = fma32(s[:, None], dot4[:, l], acc)
            if contracted:
                summs = fma32(wm[:, l], np.full(rows, ys[l], np.float32), summs).astype(np.float32)
            else:
                summs = (summs + (wm[:, l] * ys[l]).astype(np.float32)).astype(np.float32)
        tree = (((acc[:, 0] + acc[:, 4]) + (acc[:, 2] + acc[:, 6])) + ((acc[:, 1] + acc[:, 5]) + (acc[:, 3] + acc[:, 7]))).astype(np.float32)
        return (tree + summs).astype(np.float32)


@pytest.mark.parametrize("contracted", [False, True], ids=["mul_add", "fma"])
@pytest.mark.parametrize("t", l1.TYPES)
def test_formulation_reproduces_the_reference_on_the_edge_case(stored, t, contracted):
    blocks, xs, digest, wtags, xtags = l1.edge_case(t)
    assert {"neg_d", "zero_d", "subnormal_d", "big_d", "zero_m", "neg_m", "big_m", "quants_min", "quants_max"} <= set(wtags.reshape(-1))
    assert t == l1.Q4_1 or {"qh_0", "qh_1"} <= set(wtags.reshape(-1))
    assert {"zero", "ties", "tiny", "equal"} <= set(xtags.reshape(-1))
    dots, _, _ = stored_case(stored, "%s_edge" % l1.NAME[t], digest)
    assert np.isfinite(dots).all()
    rng = np.random.default_rng(17 + t)
    for i, x in enumerate(xs):
        got = mfma_formulation(t, blocks, l1.quantize_row_q8_1(x), rng, contracted)
        assert np.array_equal(bits(got), bits(dots[i])), "vector %d: differs from the reference's stored dots" % i


@pytest.mark.parametrize("contracted", [False, True], ids=["mul_add", "fma"])
@pytest.mark.parametrize("t", l1.TYPES)
def test_formulation_reproduces_the_reference_on_a_stored_random_case(stored, t, contracted):
    blocks, xs, digest = l1.rand_case(t, 512)
    dots, _, _ = stored_case(stored, "%s_K512" % l1.NAME[t], digest)
    assert np.isfinite(dots).all()
    rng = np.random.default_rng(29 + t)
    for i, x in enumerate(xs):
        got = mfma_formulation(t, blocks, l1.quantize_row_q8_1(x), rng, contracted)
        assert np.array_equal(bits(got), bits(dots[i])), "vector %d" % i


def test_the_switch_is_public():
    """the built library exports bamd_set_prefill_q1, include/bamd.h declares it, the Python package has the setter (no device needed)"""
    import booster_amd as bamd
    from booster_amd import build
    L = ctypes.CDLL(build.build())
    assert hasattr(L, "bamd_set_prefill_q1")
    header = open(os.path.join(ROOT, "include", "bamd.h")).read()
    assert re.search(r"^void bamd_set_prefill_q1\(int on\);", header, re.M)
    assert callable(bamd.set_prefill_q1)
