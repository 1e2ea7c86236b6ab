"""CPU: the arithmetic of the matrix-core prompt mat-mul for Q8_0 / Q4_0 / Q5_0 weights (booster_amd/csrc/bamd_prefill2_b32.hip), checked before a GPU is
involved.  Per 32-weight block l and SIMD lane e of the reference the kernel multiplies the f16 images of four weights and four int8 activations on the matrix
cores and sums the four f32 products in whatever order the instruction takes; the scale product f32(d_w) * f32(d_x), the chain acc_e = fma(scale, dot4_e, acc_e)
in block order and the hsum tree follow on the vector ALUs.  That is the reference's dot product only if every operand is an exact float16, every four-term sum
is exact in f32 in any order and the scale product is exact; all three are asserted here, and the whole formulation is held to the genuine reference's stored
outputs (tests/golden/legacy_kats.npz), bit for bit.  The last test asks for the public switch of the feature in the built library and the header."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import legacy_ref as lg
from lowbit_ref import fma32
from test_legacy_ref import stored, stored_case  # noqa: F401  (stored: fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFFSET = {lg.Q8_0: 128, lg.Q4_0: 8, lg.Q5_0: 16}     # u = weight + offset is the unsigned byte the kernel widens: byte ^ 0x80, nibble, nibble | bit 4


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_every_operand_is_an_exact_float16():
    for t, off in OFFSET.items():
        u = np.arange(2 * off, dtype=np.uint16)                                  # 0 .. 255 / 15 / 31
        img = (np.uint16(0x6400) | u).view(np.float16)                          # the v_perm image: 1024 + u
        assert np.array_equal(img.astype(np.int64), 1024 + u.astype(np.int64))
        kz = np.float16(-(1024 + off))
        assert int(kz) == -(1024 + off)
        w = (img + kz).astype(np.float16)
        assert np.array_equal(w.astype(np.int64), u.astype(np.int64) - off), "type %d" % t
    a = np.arange(-127, 128)
    assert np.array_equal(a.astype(np.float16).astype(np.int64), a)


def test_every_product_and_every_four_term_sum_is_exact_in_f32():
    w, x = np.meshgrid(np.arange(-128, 128, dtype=np.int64), np.arange(-127, 128, dtype=np.int64), indexing="ij")      # all 256 x 255 byte pairs
    p = (w.astype(np.float16).astype(np.float32) * x.astype(np.float16).astype(np.float32)).astype(np.float32)
    assert p.shape == (256, 255) and np.array_equal(p.astype(np.int64), w * x)
    assert 4 * 128 * 127 < 2 ** 24
    # the extreme four-term sums, every order of the additions: partial sums are integers of magnitude <= 4 * 128 * 127, so nothing rounds
    ext = [np.float32(v) for v in (-128 * 127, 128 * 127, 127 * 127, -127 * 127, 1, -1, 0)]
    for terms in itertools.product(ext, repeat=4):
        exact = int(sum(int(v) for v in terms))
        for order in ((0, 1, 2, 3), (3, 2, 1, 0), (0, 2, 1, 3)):
            s = np.float32(0)
            for k in order:
                s = np.float32(s + terms[k])
            assert int(s) == exact
        assert int(np.float32(np.float32(terms[0] + terms[1]) + np.float32(terms[2] + terms[3]))) == exact


def test_the_product_of_two_widened_f16_scales_is_exact():
    """f32(a) * f32(b) == the float64 product for every pair of f16 exponents with the extreme significands, subnormals and 65504 included"""
    vals = []
    for e in range(0, 31):                                                       # biased exponent 0 = subnormals (and zero)
        for m in (0, 1, 0x200, 0x3fe, 0x3ff):
            vals.append((e << 10) | m)
    h = np.array(vals + [v | 0x8000 for v in vals], np.uint16).view(np.float16)
    assert np.float16(65504) in h and np.float16(2.0 ** -24) in h
    a = h.astype(np.float32)
    with np.errstate(all="ignore"):
        p32 = (a[:, None] * a[None, :]).astype(np.float32)
    p64 = a.astype(np.float64)[:, None] * a.astype(np.float64)[None, :]
    assert np.isfinite(p32).all() and np.array_equal(p32.astype(np.float64), p64)
    nz = p64[p64 != 0]
    assert np.abs(nz).min() == 2.0 ** -48                                       # the smallest non-zero product: a normal f32


def mfma_formulation(t, raw, q8, rng):
    """float32 [rows]: the kernel's arithmetic in numpy — f16 operands, the four f32 products of a (block, e) link summed in a shuffled order, the f32 scale
    product, the chains in block order, the tree"""
    yd, qa = lg.q8_0_fields(q8)
    nb = yd.size
    wd, wq = lg.unpack(t, raw)
    rows = wd.size // nb
    u16 = (wq + OFFSET[t]).astype(np.uint16)
    w16 = ((np.uint16(0x6400) | u16).view(np.float16) + np.float16(-(1024 + OFFSET[t]))).astype(np.float16)
    assert np.array_equal(w16.astype(np.int64), wq)
    A = w16.astype(np.float32).reshape(rows, nb, 8, 4)
    B = qa.astype(np.float16).astype(np.float32).reshape(1, nb, 8, 4)
    prod = (A * B).astype(np.float32)
    dot4 = np.zeros((rows, nb, 8), np.float32)
    for k in rng.permutation(4):
        dot4 = (dot4 + prod[..., k]).astype(np.float32)
    wd = wd.reshape(rows, nb)
    acc = np.zeros((rows, 8), np.float32)
    with np.errstate(all="ignore"):
        for l in range(nb):
            s = (wd[:, l] * yd[l]).astype(np.float32)
            acc = fma32(s[:, None], dot4[:, l], acc)
        return (((acc[:, 0] + acc[:, 4]) + (acc[:, 2] + acc[:, 6])) + ((acc[:, 1] + acc[:, 5]) + (acc[:, 3] + acc[:, 7]))).astype(np.float32)


@pytest.mark.parametrize("t", lg.TYPES)
def test_formulation_reproduces_the_reference_on_the_edge_cases(stored, t):
    blocks, xs, digest, wtags, xtags = lg.edge_case(t)
    assert {"zero_d", "subnormal_d", "quants_min", "quants_max"} <= set(wtags.reshape(-1)) and {"zero", "ties", "tiny"} <= set(xtags.reshape(-1))
    dots, _, _ = stored_case(stored, "%s_edge" % lg.NAME[t], digest)
    rng = np.random.default_rng(17 + t)
    for i, x in enumerate(xs):
        assert np.array_equal(bits(mfma_formulation(t, blocks, lg.quantize_row_q8_0(x), rng)), bits(dots[i])), "vector %d: differs from the reference's stored dots" % i


@pytest.mark.parametrize("t", lg.TYPES)
def test_formulation_reproduces_the_reference_on_a_stored_random_case(stored, t):
    blocks, xs, digest = lg.rand_case(t, 512)
    dots, _, _ = stored_case(stored, "%s_K512" % lg.NAME[t], digest)
    rng = np.random.default_rng(29 + t)
    for i, x in enumerate(xs):
        assert np.array_equal(bits(mfma_formulation(t, blocks, lg.quantize_row_q8_0(x), rng)), bits(dots[i])), "vector %d" % i


def test_the_switch_is_public():
    """the built library exports bamd_set_prefill_q0, include/bamd.h declares it, the Python package has the setter (no device needed)"""
    import booster_amd as bamd
    from booster_amd import build
    L = ctypes.CDLL(build.build())
    assert hasattr(L, "bamd_set_prefill_q0")
    header = open(os.path.join(ROOT, "include", "bamd.h")).read()
    assert re.search(r"^void bamd_set_prefill_q0\(int on\);", header, re.M)
    assert callable(bamd.set_prefill_q0)
