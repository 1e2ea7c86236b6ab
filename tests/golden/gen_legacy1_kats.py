"""Generates tests/golden/legacy1_kats.npz: the genuine reference's outputs (oracle/_ref/libggml_ref.so, built by `make -C oracle ref`) for the seeded
Q4_1 / Q5_1 inputs of tests/legacy1_ref.py — per type the random cases (K in legacy1_ref.KS, 32 rows, three activation magnitudes) and the edge case
(edge weight blocks x edge activations): the ggml_vec_dot_q*_1_q8_1 result of every (vector, row); the dequantize_row_q*_1 output (rows 0, 15, 31 of the
random cases, every row of the edge case); a SHA-256 of the reference's quantize_row_q8_1 bytes per vector; a SHA-256 of the inputs they all belong to.
Two more vectors are stored by their quantiser digests only: legacy1_ref.overflow_vector (a block whose s overflows f16) and
legacy1_ref.double_rounding_vector (blocks whose s depends on the product being rounded to f32 before it is rounded to f16).  Data only.  Run where the reference is
built; the .npz is the committed fixture.

    python tests/golden/gen_legacy1_kats.py
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
import legacy1_ref as l1  # noqa: E402

L = l1.load_ref()
if L is None:
    sys.exit("oracle/_ref/libggml_ref.so is not built (make -C oracle ref)")
out = {}
for qt in l1.TYPES:
    for key, blocks, xs, digest, deq_rows in l1.all_cases(qt):
        out[key + "_inputs_sha256"] = np.array(digest)
        dots, q8sha, deq = l1.reference_outputs(L, qt, blocks, xs, deq_rows)
        assert np.isfinite(dots).all() and np.isfinite(deq).all(), key
        out[key + "_dots"] = dots
        out[key + "_q8_sha256"] = np.array(q8sha)
        out[key + "_dequant"] = deq
xo = l1.overflow_vector()
q8 = l1.reference_q8_1(L, xo)
s16 = np.ascontiguousarray(q8.reshape(-1, 36)[:, 2:4]).view(np.float16).reshape(-1)
assert np.isposinf(s16[3]) and np.isneginf(s16[5]) and np.isfinite(np.delete(s16, [3, 5])).all()
out["overflow_inputs_sha256"] = np.array(hashlib.sha256(xo.tobytes()).hexdigest())
out["overflow_q8_sha256"] = np.array(hashlib.sha256(q8.tobytes()).hexdigest())
xr = l1.double_rounding_vector()
out["round2_inputs_sha256"] = np.array(hashlib.sha256(xr.tobytes()).hexdigest())
out["round2_q8_sha256"] = np.array(hashlib.sha256(l1.reference_q8_1(L, xr).tobytes()).hexdigest())
np.savez_compressed(os.path.join(HERE, "legacy1_kats.npz"), **out)
print("wrote", os.path.join(HERE, "legacy1_kats.npz"), len(out), "arrays")
