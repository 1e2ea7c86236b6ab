"""Generates tests/golden/lowbit_kats.npz: the genuine reference's outputs (oracle/_ref/libggml_ref.so, built by `make -C oracle ref`) for the
seeded Q2_K / Q3_K inputs of tests/lowbit_ref.py — per type the random cases (K in lowbit_ref.KS, 32 rows, three activation magnitudes) and the
edge case (edge weight blocks x edge activations): the ggml_vec_dot_q*_K_q8_K result of every (vector, row), the dequantize_row_q*_K output of the
matrix (rows 0, 15, 31 of the random cases, every row of the edge case), a SHA-256 of the reference's quantize_row_q8_K bytes per vector, and a
SHA-256 of the inputs they all belong to.  Data only.  Run where the reference is built; the .npz is the committed fixture.

    python tests/golden/gen_lowbit_kats.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
import lowbit_ref as lr  # noqa: E402

L = lr.load_ref()
if L is None:
    sys.exit("oracle/_ref/libggml_ref.so is not built (make -C oracle ref)")
out = {}
for qt in (lr.Q2_K, lr.Q3_K):
    for key, blocks, xs, digest, deq_rows in lr.all_cases(qt):
        out[key + "_inputs_sha256"] = np.array(digest)
        dots, q8sha, deq = lr.reference_outputs(L, qt, blocks, xs, deq_rows)
        assert np.isfinite(dots).all() and np.isfinite(deq).all(), key
        out[key + "_dots"] = dots
        out[key + "_q8_sha256"] = np.array(q8sha)
        out[key + "_dequant"] = deq
np.savez_compressed(os.path.join(HERE, "lowbit_kats.npz"), **out)
print("wrote", os.path.join(HERE, "lowbit_kats.npz"), len(out), "arrays")
