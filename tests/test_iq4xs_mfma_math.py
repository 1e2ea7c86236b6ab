"""CPU: the arithmetic of the matrix-core prompt mat-mul for IQ4_XS weights (booster_amd/csrc/bamd_prefill2_xs.hip: the policy X2IQ4XS of matmul_mfma2_kernel),
checked before a GPU is involved.  Per SIMD lane e and super-block the kernel splits the block scale s = ls - 32 into sa = s & ~15 and sl = s & 15, forms the
f16 fragments sa x value and sl x value, multiplies both with the f16 image of the 32 int8 activations of lane e and sums the products in f32 — two MFMAs chained
through the accumulator, in whatever order the matrix core takes.  That is the reference's integer lane sum only if every operand is an exact float16 and every
partial f32 sum is exact; both are asserted here against tests/iq4xs_ref.py on every stored case.  And the switch of the family, beside the recorded answers
of the other types (tests/golden/prefill_reasons.json)."""
import ctypes as C
import json
import os

import numpy as np

import iq4xs_ref as xr
from test_prefill_family import GOLDEN, TYPES, _key

SENTENCE = ("the model holds an IQ4_XS matrix: these have no matrix-core kernel, and side tables are all-or-nothing per model, so every prompt mat-mul runs on the "
            "integer-dot kernel (token by token where K > 35840)")

OTHERS = ("lowbit", "q0", "q1", "nl", "flt", "bf16")


def split(s):
    return s & ~15, s & 15


def test_both_halves_of_the_split_scale_give_exact_float16_products():
    s, v = np.meshgrid(np.arange(-32, 32), xr.KVALUES)
    sa, sl = split(s)
    assert np.array_equal(sa + sl, s) and set(sa.reshape(-1)) == {-32, -16, 0, 16} and sl.min() == 0 and sl.max() == 15
    v16 = v.astype(np.float16)
    assert np.array_equal((sa.astype(np.float16) * v16).astype(np.float16).astype(np.int64), sa * v)
    assert np.array_equal((sl.astype(np.float16) * v16).astype(np.float16).astype(np.int64), sl * v)
    assert not np.array_equal((s.astype(np.float16) * v16).astype(np.float16).astype(np.int64), s * v)      # why it is split: 31 x 113 is no float16
    # the builders' route to the value: the byte u = value + 128 under 0x64 is the f16 1024 + u, and - 1152 leaves the value
    u = (xr.KVALUES + 128).astype(np.uint16)
    assert u.min() == 1 and u.max() == 241
    assert np.array_equal(((np.uint16(0x6400) | u).view(np.float16) + np.float16(-1152)).astype(np.int64), xr.KVALUES)


def test_chained_f16_products_rebuild_the_lane_sums_in_either_order(po):
    """S = A_l.B + (A_a.B + 0) slot by slot in f32, forwards and backwards, on every stored case: the restatement's integer lane sums, below 2^24"""
    top = 0
    for key, blocks, xs, _, _ in xr.all_cases():
        _, ls, _, val = xr.unpack(blocks)
        for x in xs:
            q8 = po.quantize_q8_K(x)
            yd, qa, _ = xr.ei.q8_fields(q8)
            nb = yd.size
            rows = val.shape[0] // nb
            want = xr.lane_sums(blocks, q8)
            sa, sl = split(np.repeat(ls, 32, axis=1))
            v16 = val.astype(np.float16)
            act = qa.astype(np.float16).astype(np.float32).reshape(1, nb, 8, 8, 4).transpose(0, 1, 3, 2, 4).reshape(1, nb, 8, 32)
            # element 32 ib + 4 e + u belongs to lane e: [.., ib, e, u] -> [.., e, (ib, u)]
            lanes = lambda f: (f.astype(np.float16) * v16).astype(np.float16).astype(np.float32).reshape(rows, nb, 8, 8, 4).transpose(0, 1, 3, 2, 4).reshape(rows, nb, 8, 32)
            Aa, Al = lanes(sa), lanes(sl)
            for order in (range(32), range(31, -1, -1)):
                S = np.zeros((rows, nb, 8), np.float32)
                for A in (Aa, Al):
                    for k in order:
                        S = (S + A[..., k] * act[..., k]).astype(np.float32)
                        top = max(top, int(np.abs(S).max()))
                assert np.array_equal(S.astype(np.int64), want), key
    assert 0 < top <= 32 * 32 * 127 * 127 < 2 ** 24


def test_the_switch_moves_iq4_xs_and_nothing_else():
    import booster_amd
    f = booster_amd.lib().bamd_prefill_reason_test
    f.argtypes = [C.c_int]; f.restype = C.c_char_p
    with open(GOLDEN) as g:
        gold = json.load(g)
    all_off = {n: gold["strings"][i] for n, i in zip(gold["types"], gold["cases"][_key(0)])}
    default = os.environ.get("BAMD_PREFILL_XS", "")[:1] == "1"
    try:
        booster_amd.set_prefill_xs(False)
        assert f(xr.IQ4_XS).decode() == SENTENCE
        booster_amd.set_prefill_xs(True)
        assert f(xr.IQ4_XS).decode() == "tables"
        for s in OTHERS:                                                   # the recorded row is the one with the other switches off
            getattr(booster_amd, "set_prefill_" + s)(False)
        assert {n: f(t).decode() for n, t in TYPES.items()} == all_off
    finally:
        booster_amd.set_prefill_xs(default)
        for s in OTHERS:
            getattr(booster_amd, "set_prefill_" + s)(os.environ.get("BAMD_PREFILL_" + s.upper(), "")[:1] == "1")
