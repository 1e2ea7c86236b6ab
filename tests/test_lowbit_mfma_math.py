"""CPU: the arithmetic of the matrix-core prompt mat-muls for Q3_K / Q2_K weights (booster_amd/csrc/bamd_prefill2.hip, matmul_mfma2_kernel with the X2LowBit policies), checked
before a GPU is involved.  Per SIMD lane e of the reference and super-block the kernel forms an f16 fragment scale x quant, multiplies it with the f16 image of
the 32 int8 activations of lane e and sums the products in f32 in whatever order the matrix core takes; then come the reference's f32 chains.  That is only
the reference's dot product if every operand is an exact float16 and the f32 sum is exact in any order; both are asserted here, and the whole formulation is
held to tests/lowbit_ref.py and to the genuine reference's stored outputs (tests/golden/lowbit_kats.npz) on the edge matrices, bit for bit."""
import numpy as np
import pytest

import lowbit_ref as lr
from test_lowbit_ref import stored, stored_case  # noqa: F401  (stored: fixture)

TYPES = [lr.Q2_K, lr.Q3_K]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_every_operand_is_an_exact_float16():
    for lo, hi, qlo, qhi in ((-32, 31, -4, 3), (0, 15, 0, 3)):             # Q3_K: (sc - 32) x (low2 + 4 hbit - 4); Q2_K: sc x q
        sc, q = np.meshgrid(np.arange(lo, hi + 1), np.arange(qlo, qhi + 1))
        p = (sc * q).reshape(-1)
        assert np.array_equal(p.astype(np.float16).astype(np.int64), p)
        # the builders' route to it: the f16 image 0x6400 | u of u = q - qlo is 1024 + u; (1024 + u) - (1024 - qlo) and the product with the f16 scale round nowhere
        u = (q - qlo).reshape(-1).astype(np.uint16)
        img = (np.uint16(0x6400) | u).view(np.float16)
        assert np.array_equal(img.astype(np.int64), 1024 + u)
        v = (img + np.float16(-(1024 - qlo))).astype(np.float16)
        assert np.array_equal(v.astype(np.int64), q.reshape(-1))
        assert np.array_equal((v * sc.reshape(-1).astype(np.float16)).astype(np.float16).astype(np.int64), p)
    b = np.arange(-2048, 2033)                                              # sums of sixteen int8
    assert np.array_equal(b.astype(np.float16).astype(np.int64), b)
    m = np.arange(16)
    assert np.array_equal(m.astype(np.float16).astype(np.int64), m)
    a = np.arange(-128, 128)
    assert np.array_equal(a.astype(np.float16).astype(np.int64), a)
    # bounds of the sums: 32 slots of |scale x quant| x |activation|, two min products — integers below 2^24, so every partial f32 sum is exact
    assert 32 * 128 * 128 < 2 ** 24 and 32 * 45 * 128 < 2 ** 24 and 2 * 15 * 2048 < 2 ** 24


def mfma_formulation(t, raw, q8, rng):
    """float32 [rows]: the kernel's arithmetic in numpy — f16 operands, f32 products summed over the 32 slots of (e, super-block) in a shuffled order, the chains"""
    yd, qa, bsums = lr.q8_fields(q8)
    nb = yd.size
    f = lr.unpack(t, raw)
    rows = f["q"].shape[0] // nb
    el = np.arange(256)
    frag = (f["scale"][:, el >> 4] * f["q"]).astype(np.float16)                                   # [rows * nb][256]
    assert np.array_equal(frag.astype(np.int64), f["scale"][:, el >> 4].astype(np.int64) * f["q"])
    act = qa.astype(np.float16)                                                                   # [nb][256]
    # element n = 32 c + 4 e + u belongs to lane e: [.., c, e, u] -> [.., e, (c, u)]
    A = frag.astype(np.float32).reshape(rows, nb, 8, 8, 4).transpose(0, 1, 3, 2, 4).reshape(rows, nb, 8, 32)
    B = act.astype(np.float32).reshape(nb, 8, 8, 4).transpose(0, 2, 1, 3).reshape(nb, 8, 32)
    prod = A * B[None]                                                                            # f32 products of f16 values: exact
    isum = np.zeros((rows, nb, 8), np.float32)
    for k in rng.permutation(32):
        isum = (isum + prod[..., k]).astype(np.float32)                                           # f32 adds, one slot at a time, shuffled
    if t == lr.Q2_K:
        mn16 = f["mn"].astype(np.float16).astype(np.float32).reshape(rows, nb, 8, 2)
        bs16 = bsums.astype(np.float16).astype(np.float32).reshape(1, nb, 8, 2)
        pm = (mn16[..., 0] * bs16[..., 0] + mn16[..., 1] * bs16[..., 1]).astype(np.float32)      # v_dot2_f32_f16: exact integers
    xd, xm = f["d"].reshape(rows, nb), f["dmin"].reshape(rows, nb)
    acc = np.zeros((rows, 8), np.float32)
    with np.errstate(all="ignore"):
        for i in range(nb):
            d = (yd[i] * xd[:, i]).astype(np.float32)
            if t == lr.Q2_K:
                dmin = ((-yd[i]) * xm[:, i]).astype(np.float32)
                acc = lr.fma32(dmin[:, None], pm[:, i], acc)
            acc = lr.fma32(d[:, None], isum[:, i], acc)
        r = acc[:, 0:4] + acc[:, 4:8]
        r = r[:, 0:2] + r[:, 2:4]
        return (r[:, 0] + r[:, 1]).astype(np.float32)


@pytest.mark.parametrize("t", TYPES)
def test_formulation_reproduces_the_reference_on_the_edge_cases(po, stored, t):
    blocks, xs, digest, wtags, xtags = lr.edge_case(t)
    want_kinds = {"scales_lo", "scales_hi", "quants_min", "quants_max"} | ({"hmask_0", "hmask_1"} if t == lr.Q3_K else set())
    assert want_kinds <= set(wtags.reshape(-1)) and "opposite_max" in set(xtags.reshape(-1))
    dots, _, _ = stored_case(stored, "%s_edge" % lr.NAME[t], digest)
    rng = np.random.default_rng(17 + t)
    for i, x in enumerate(xs):
        q8 = po.quantize_q8_K(x)
        got = mfma_formulation(t, blocks, q8, rng)
        assert np.array_equal(bits(got), bits(lr.vec_dot_rows(t, blocks, q8))), "vector %d: differs from the restatement" % i
        assert np.array_equal(bits(got), bits(dots[i])), "vector %d: differs from the reference's stored dots" % i


@pytest.mark.parametrize("t", TYPES)
def test_formulation_reproduces_the_reference_on_a_stored_random_case(po, stored, t):
    blocks, xs, digest = lr.rand_case(t, 1024)
    dots, _, _ = stored_case(stored, "%s_K1024" % lr.NAME[t], digest)
    rng = np.random.default_rng(29 + t)
    for i, x in enumerate(xs):
        assert np.array_equal(bits(mfma_formulation(t, blocks, po.quantize_q8_K(x), rng)), bits(dots[i])), "vector %d" % i
