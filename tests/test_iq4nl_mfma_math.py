"""CPU: the arithmetic of the matrix-core prompt mat-mul for IQ4_NL weights (matmul_mfma_b32_kernel<IQ4_NL, EPI>, booster_amd/csrc/bamd_prefill2_b32.hip), checked before a GPU is involved.
As tests/test_legacy1_mfma_math.py for the Q4_1 family: per 32-weight block l and SIMD lane e of the reference the kernel multiplies the f16 images of four table
values ((0x6400 | (value + 128)) - 1152 = value) and four int8 activations on the matrix cores and sums the four f32 products in whatever order the instruction
takes; the scale product, TWO sets of eight chains (the even blocks into one, the odd blocks into the other, each in block order), their lane-wise sum and the
tree follow on the vector ALUs.  The operand images, the products, the four-term sums and the formulation as a whole are held to the genuine reference's stored
outputs (tests/golden/iq4nl_kats.npz), bit for bit; the same formulation with ONE accumulator set must miss them at K = 4096, or the comparison shows nothing.
The last test asks for the public switch of the feature in the built library and the header."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import iq4nl_ref as nl
import legacy_ref as lg
from lowbit_ref import fma32
from test_iq4nl_ref import stored, stored_case  # noqa: F401  (stored: fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def image(values):
    """the kernel's f16 weight operand of table values (int): u = value + 128 as a byte, the v_perm image 0x6400 | u = 1024 + u, minus 1152"""
    u = (np.asarray(values, np.int64) + 128).astype(np.uint16)
    assert u.min() >= 1 and u.max() <= 241
    return ((np.uint16(0x6400) | u).view(np.float16) + np.float16(-1152.0)).astype(np.float16)


def test_every_operand_is_an_exact_float16():
    u = (nl.KVALUES.astype(np.int64) + 128).astype(np.uint16)
    assert u.min() == 1 and u.max() == 241                                       # the byte after ^ 0x80
    img = (np.uint16(0x6400) | u).view(np.float16)
    assert np.array_equal(img.astype(np.int64), 1024 + u.astype(np.int64))       # exact: 1024 .. 2047 are integers in f16
    assert np.array_equal(image(nl.KVALUES).astype(np.int64), nl.KVALUES.astype(np.int64))
    a = np.arange(-127, 128)
    assert np.array_equal(a.astype(np.float16).astype(np.int64), a)


def test_every_product_and_every_four_term_sum_is_exact_in_f32():
    w, x = np.meshgrid(nl.KVALUES.astype(np.int64), np.arange(-127, 128, dtype=np.int64), indexing="ij")              # all 16 x 255 operand pairs
    p = (image(w).astype(np.float32) * x.astype(np.float16).astype(np.float32)).astype(np.float32)
    assert p.shape == (16, 255) and np.array_equal(p.astype(np.int64), w * x)
    assert 4 * 127 * 127 == 64516 < 2 ** 24
    # the extreme four-term sums, every order of the additions: partial sums are integers of magnitude <= 64 516, so nothing rounds
    ext = [np.float32(v) for v in (127 * 127, -127 * 127, 113 * 127, -113 * 127, 1, -1, 0)]
    for terms in itertools.product(ext, repeat=4):
        exact = int(sum(int(v) for v in terms))
        for order in itertools.permutations(range(4)):
            s = np.float32(0)
            for k in order:
                s = np.float32(s + terms[k])
            assert int(s) == exact
        assert int(np.float32(np.float32(terms[0] + terms[1]) + np.float32(terms[2] + terms[3]))) == exact


def mfma_formulation(raw, q8, rng, sets=2):
    """float32 [rows]: the kernel's arithmetic in numpy — f16 operands, the four f32 products of a (block, e) link summed in a shuffled order, the f32 scale
    product, `sets` accumulator sets of eight chains (2: block l into set l & 1, the kernel; 1: every block into one set, the Q4_0 chain), each in block order,
    the lane-wise sum of the sets and the tree"""
    yd, qa = lg.q8_0_fields(q8)
    nb = yd.size
    wd, _, wq = nl.unpack(raw)
    rows = wd.size // nb
    w16 = image(wq)
    assert np.array_equal(w16.astype(np.int64), wq)
    A = w16.astype(np.float32).reshape(rows, nb, 8, 4)
    B = qa.astype(np.float16).astype(np.float32).reshape(1, nb, 8, 4)
    prod = (A * B).astype(np.float32)
    dot4 = np.zeros((rows, nb, 8), np.float32)
    for k in rng.permutation(4):
        dot4 = (dot4 + prod[..., k]).astype(np.float32)
    wd = wd.reshape(rows, nb)
    acc = [np.zeros((rows, 8), np.float32) for _ in range(sets)]
    with np.errstate(all="ignore"):
        for l in range(nb):
            s = (wd[:, l] * yd[l]).astype(np.float32)
            acc[l % sets] = fma32(s[:, None], dot4[:, l], acc[l % sets])
        a = acc[0] if sets == 1 else (acc[0] + acc[1]).astype(np.float32)
        return (((a[:, 0] + a[:, 4]) + (a[:, 2] + a[:, 6])) + ((a[:, 1] + a[:, 5]) + (a[:, 3] + a[:, 7]))).astype(np.float32)


def test_formulation_reproduces_the_reference_on_the_edge_case(stored):
    blocks, xs, digest, wtags, xtags = nl.edge_case()
    assert {"neg_d", "zero_d", "subnormal_d", "big_d", "quants_min", "quants_max"} <= set(wtags.reshape(-1))
    assert {"zero", "neg_max", "ties", "tiny", "single"} <= set(xtags.reshape(-1))
    dots, _, _ = stored_case(stored, "iq4_nl_edge", digest)
    assert np.isfinite(dots).all()
    rng = np.random.default_rng(17 + nl.IQ4_NL)
    for i, x in enumerate(xs):
        got = mfma_formulation(blocks, lg.quantize_row_q8_0(x), rng)
        assert np.array_equal(bits(got), bits(dots[i])), "vector %d: differs from the reference's stored dots" % i


@pytest.mark.parametrize("K", [512, 4096])
def test_formulation_reproduces_the_reference_on_a_stored_random_case(stored, K):
    blocks, xs, digest = nl.rand_case(K)
    dots, _, _ = stored_case(stored, "iq4_nl_K%d" % K, digest)
    assert np.isfinite(dots).all()
    rng = np.random.default_rng(29 + K)
    for i, x in enumerate(xs):
        got = mfma_formulation(blocks, lg.quantize_row_q8_0(x), rng)
        assert np.array_equal(bits(got), bits(dots[i])), "K %d vector %d" % (K, i)


def test_one_accumulator_set_misses_the_reference(stored):
    """the guard of the two tests above: with one accumulator set the same code gives other bits at K = 4096, for every activation magnitude"""
    blocks, xs, digest = nl.rand_case(4096)
    dots, _, _ = stored_case(stored, "iq4_nl_K4096", digest)
    rng = np.random.default_rng(31)
    for i, x in enumerate(xs):
        one = mfma_formulation(blocks, lg.quantize_row_q8_0(x), rng, sets=1)
        assert (bits(one) != bits(dots[i])).any(), "magnitude %g: one accumulator set gives the reference's bits, the comparison checks nothing" % nl.SCALES[i]


def test_the_switch_is_public():
    """the built library exports bamd_set_prefill_nl, include/bamd.h declares it, the Python package has the setter (no device needed)"""
    import booster_amd as bamd
    from booster_amd import build
    L = ctypes.CDLL(build.build())
    assert hasattr(L, "bamd_set_prefill_nl")
    header = open(os.path.join(ROOT, "include", "bamd.h")).read()
    assert re.search(r"^void bamd_set_prefill_nl\(int on\);", header, re.M)
    assert callable(bamd.set_prefill_nl)
