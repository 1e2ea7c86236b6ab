"""Generates tests/golden/legacy_kats.npz: the genuine reference's outputs (oracle/_ref/libggml_ref.so, built by `make -C oracle ref`) for the seeded
Q8_0 / Q4_0 / Q5_0 inputs of tests/legacy_ref.py — per type the random cases (K in legacy_ref.KS, 32 rows, three activation magnitudes) and the edge case
(edge weight blocks x edge activations): the ggml_vec_dot_q*_0_q8_0 result of every (vector, row); for Q8_0 and Q4_0 also the llamafile_sgemm results at n = 1
and n = 5 (what ggml_compute_forward_mul_mat calls for them); the dequantize_row_q*_0 output (rows 0, 15, 31 of the random cases, every row of the edge case);
a SHA-256 of the reference's quantize_row_q8_0 bytes per vector; and a SHA-256 of the inputs they all belong to.  Data only.  Run where the reference is
built; the .npz is the committed fixture.

    python tests/golden/gen_legacy_kats.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
import legacy_ref as lg  # noqa: E402

L = lg.load_ref()
if L is None:
    sys.exit("oracle/_ref/libggml_ref.so is not built (make -C oracle ref)")
out = {}
for qt in lg.TYPES:
    for key, blocks, xs, digest, deq_rows in lg.all_cases(qt):
        out[key + "_inputs_sha256"] = np.array(digest)
        dots, q8sha, deq, sg1, sg5 = lg.reference_outputs(L, qt, blocks, xs, deq_rows)
        assert np.isfinite(dots).all() and np.isfinite(deq).all(), key
        out[key + "_dots"] = dots
        out[key + "_q8_sha256"] = np.array(q8sha)
        out[key + "_dequant"] = deq
        if sg1 is not None:
            assert np.isfinite(sg1).all() and np.isfinite(sg5).all(), key
            out[key + "_sgemm1"] = sg1
            out[key + "_sgemm5"] = sg5
np.savez_compressed(os.path.join(HERE, "legacy_kats.npz"), **out)
print("wrote", os.path.join(HERE, "legacy_kats.npz"), len(out), "arrays")
