"""Generates tests/golden/iq4nl_kats.npz: the genuine reference's outputs (oracle/_ref/libggml_ref.so, built by `make -C oracle ref`) for the seeded IQ4_NL
inputs of tests/iq4nl_ref.py — the random cases (K in iq4nl_ref.KS, 32 rows, three activation magnitudes) and the edge case (edge weight blocks x edge
activations): the ggml_vec_dot_iq4_nl_q8_0 result of every (vector, row); the dequantize_row_iq4_nl output (rows 0, 15, 31 of the random cases, every row of
the edge case); a SHA-256 of the reference's quantize_row_q8_0 bytes per vector; and a SHA-256 of the inputs they all belong to.  Data only.  Run where the
reference is built; the .npz is the committed fixture.

The fixture must tell the reference's two-accumulator chain from the one-accumulator order of Q4_0: at K = 4096 the latter has to differ from the stored
outputs in at least one of the 32 rows for EVERY activation magnitude.  Checked here; if a magnitude does not discriminate, pick another iq4nl_ref.SEED.

    python tests/golden/gen_iq4nl_kats.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
import iq4nl_ref as nl  # noqa: E402
import legacy_ref as lg  # noqa: E402

L = nl.load_ref()
if L is None:
    sys.exit("oracle/_ref/libggml_ref.so is not built (make -C oracle ref)")
out = {}
for key, blocks, xs, digest, deq_rows in nl.all_cases():
    out[key + "_inputs_sha256"] = np.array(digest)
    dots, q8sha, deq = nl.reference_outputs(L, blocks, xs, deq_rows)
    assert np.isfinite(dots).all() and np.isfinite(deq).all(), key
    out[key + "_dots"] = dots
    out[key + "_q8_sha256"] = np.array(q8sha)
    out[key + "_dequant"] = deq
    if key == "iq4_nl_K4096":
        for i, x in enumerate(xs):
            one = nl.vec_dot_rows(blocks, lg.quantize_row_q8_0(x), one_accumulator=True)
            n = int((one.view(np.uint32) != dots[i].view(np.uint32)).sum())
            print("K = 4096, magnitude %g: the one-accumulator order differs in %d of %d rows" % (nl.SCALES[i], n, nl.ROWS))
            assert n >= 1, "magnitude %g does not tell the two chain shapes apart: pick another iq4nl_ref.SEED" % nl.SCALES[i]
np.savez_compressed(os.path.join(HERE, "iq4nl_kats.npz"), **out)
print("wrote", os.path.join(HERE, "iq4nl_kats.npz"), len(out), "arrays")
