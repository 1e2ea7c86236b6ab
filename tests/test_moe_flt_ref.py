"""CPU: the restatement of an F16 / F32 / BF16 expert row (tests/moe_flt_ref.py) against the genuine reference's recorded answers: tests/golden/moe_flt_kats.npz
(from_float + the vec_dot of the type traits, as mul_mat_id calls them) for F32 and F16, the vec_dot answers of tests/golden/float_kats.npz for BF16.  This pins the
chain order (four 8-lane accumulators) and the tail (neighbouring pairs first) the expert kernels restate."""
import os

import numpy as np
import pytest

import float_ref as fr
import moe_flt_ref as mr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KATS = np.load(os.path.join(GOLDEN, "moe_flt_kats.npz"))
FLOAT_KATS = np.load(os.path.join(GOLDEN, "float_kats.npz"))
CASES = [(t, key) for t in fr.TYPES for key in ["%s_K%d" % (fr.NAME[t], K) for K in fr.KS] + ["%s_edge" % fr.NAME[t]]]


@pytest.mark.parametrize("t,key", CASES, ids=[c[1] for c in CASES])
def test_expert_row_matches_reference(t, key):
    kats = FLOAT_KATS if t == fr.BF16 else KATS
    raw, xs, digest = next((r, x, d) for k, r, x, d in fr.all_cases(t) if k == key)
    assert str(kats[key + "_inputs_sha256"]) == digest, "the stored answers belong to other inputs"
    for i, x in enumerate(xs):
        if t == fr.F16:
            with np.errstate(all="ignore"):
                assert np.array_equal(x.astype(np.float16).view(np.uint16), kats[key + "_act"][i]), "f16 activations of vector %d" % i
        got = mr.mul_mat_id_rows(t, raw, fr.ROWS, x.size, x)
        assert np.array_equal(got.view(np.uint32), kats[key + "_dots"][i].view(np.uint32)), "vector %d" % i
