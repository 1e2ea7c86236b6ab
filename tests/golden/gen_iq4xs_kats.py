"""Generates tests/golden/iq4xs_kats.npz: the genuine reference's outputs (oracle/_ref/libggml_ref.so, built by `make -C oracle ref`) for the seeded IQ4_XS
inputs of tests/iq4xs_ref.py — the random cases (K in iq4xs_ref.KS, 32 rows, three activation magnitudes), the edge case (edge weight blocks x edge
activation blocks) and the pairs case (every nibble against every activation byte): the ggml_vec_dot_iq4_xs_q8_K result of every (vector, row); the
dequantize_row_iq4_xs output (rows 0, 15, 31 of the random cases, every row of the other two); a SHA-256 of the reference's quantize_row_q8_K bytes per
vector; and a SHA-256 of the inputs they all belong to.  For the cases of iq4xs_ref.M128_KEYS also <key>_dots_m128: the same rows against HAND-MADE Q8_K
vectors that hold the byte -128 (iq4xs_ref.m128_q8), which quantize_row_q8_K never writes (iscale = -127 / max).  Data only.  Run where the reference is
built; the .npz is the committed fixture.

The fixture must have teeth (checked here, and again from the committed file by tests/test_iq4xs_ref.py):
  (a) the plain signed dot, without the -128 rule, differs from the stored outputs in at least one of the 32 rows at K = 4096 for EVERY activation magnitude —
      on the hand-made vectors, where the rule acts; on the quantised vectors the two are the same function, and that is asserted too (no byte is -128);
  (b) the single-rounding form of the dequantiser differs from the stored rows in at least one element;
  (c) the Q4_K lane mapping differs from the stored outputs in at least one of the 32 rows at K = 4096 (for every magnitude).
If a magnitude does not discriminate, pick another iq4xs_ref.SEED.

    python tests/golden/gen_iq4xs_kats.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
import iq4xs_ref as xr  # noqa: E402
from oracle import pyoracle as po  # noqa: E402

L = xr.load_ref()
if L is None:
    sys.exit("oracle/_ref/libggml_ref.so is not built (make -C oracle ref)")
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
out = {}
for key, blocks, xs, digest, deq_rows in xr.all_cases():
    out[key + "_inputs_sha256"] = np.array(digest)
    q8s = []
    dots, q8sha, deq = xr.reference_outputs(L, blocks, xs, deq_rows, q8s)
    for q in q8s:
        assert not (xr.ei.q8_fields(q)[1] == -128).any(), key + ": quantize_row_q8_K wrote a byte of -128"
    K = xs[0].size
    if key in xr.M128_KEYS:
        hand = xr.m128_q8(key, q8s)
        assert all((xr.ei.q8_fields(q)[1] == -128).any() for q in hand)
        m128 = np.stack([xr.reference_dots(L, blocks, K, q) for q in hand])
        assert np.isfinite(m128).all(), key
        out[key + "_dots_m128"] = m128
    assert np.isfinite(dots).all() and np.isfinite(deq).all(), key
    out[key + "_dots"] = dots
    out[key + "_q8_sha256"] = np.array(q8sha)
    out[key + "_dequant"] = deq
    rb = xs[0].size // 256 * xr.BB
    if key == "iq4_xs_K4096":
        for i, x in enumerate(xs):
            q8 = po.quantize_q8_K(x)
            assert np.array_equal(q8, q8s[i])
            na = int((bits(xr.vec_dot_rows(blocks, hand[i], rule=False)) != bits(m128[i])).sum())
            assert np.array_equal(bits(xr.vec_dot_rows(blocks, q8, rule=False)), bits(xr.vec_dot_rows(blocks, q8)))
            nc = int((bits(xr.vec_dot_rows(blocks, q8, q4k_lanes=True)) != bits(dots[i])).sum())
            print("K = 4096, magnitude %g: on the hand-made -128 vectors %d of %d rows differ without the -128 rule; under the Q4_K lane mapping %d" % (xr.SCALES[i], na, xr.ROWS, nc))
            assert na >= 1, "magnitude %g does not show the -128 rule: pick another iq4xs_ref.SEED" % xr.SCALES[i]
            assert nc >= 1, "magnitude %g does not tell the lane mappings apart: pick another iq4xs_ref.SEED" % xr.SCALES[i]
        nb = sum(int((bits(xr.dequantize(blocks[r * rb:(r + 1) * rb], fused=True)) != bits(deq[j])).sum()) for j, r in enumerate(deq_rows))
        print("K = 4096: the single-rounding dequantiser differs in %d elements of the stored rows" % nb)
        assert nb >= 1, "the stored rows do not show the two roundings: pick another iq4xs_ref.SEED"
np.savez_compressed(os.path.join(HERE, "iq4xs_kats.npz"), **out)
print("wrote", os.path.join(HERE, "iq4xs_kats.npz"), len(out), "arrays", os.path.getsize(os.path.join(HERE, "iq4xs_kats.npz")), "bytes")
