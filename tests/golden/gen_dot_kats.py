"""Generates tests/golden/dot_kats.npz: the genuine reference's outputs (oracle/_ref/libggml_ref.so, built by `make -C oracle ref`) for the
inputs of tests/test_oracle_vs_ref.py — per K-quant type and row length K, for each activation vector its quantize_row_q8_K bytes and the
ggml_vec_dot_q*_K_q8_K result of every row, with a SHA-256 of the inputs they belong to.  Run where the reference is built; the .npz is the
committed fixture.

    python tests/golden/gen_dot_kats.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
import test_oracle_vs_ref as t  # noqa: E402

L = t.load_ref()
if L is None:
    sys.exit("oracle/_ref/libggml_ref.so is not built (make -C oracle ref)")
out = {}
for qt, bb, fn in t.CASES:
    for K in t.KS:
        blocks, xs, digest = t.case_inputs(qt, K)
        key = "%s_K%d" % (fn, K)
        out[key + "_inputs_sha256"] = np.array(digest)
        for i, (q8r, want) in enumerate(t.reference_outputs(L, bb, fn, K, blocks, xs)):
            out["%s_q8_%d" % (key, i)] = q8r
            out["%s_dot_%d" % (key, i)] = want
np.savez_compressed(os.path.join(HERE, "dot_kats.npz"), **out)
print("wrote", os.path.join(HERE, "dot_kats.npz"), len(out), "arrays")
