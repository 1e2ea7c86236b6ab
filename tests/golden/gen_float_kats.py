"""Generates tests/golden/float_kats.npz: the genuine reference's outputs (oracle/_ref/libggml_ref.so, built by `make -C oracle ref`) for the seeded
F32 / F16 / BF16 inputs of tests/float_ref.py — per type the random cases (K in float_ref.KS, 32 rows, three activation magnitudes) and the edge case (edge
weights x edge activations): for F32 and F16 the llamafile_sgemm results at n = 1 and n = 5 (what ggml_compute_forward_mul_mat calls for them); for BF16 the
bytes of ggml_fp32_to_bf16_row and the vec_dot of the type traits over them; the to_float rows (rows 0, 15, 31 of the random cases, every row of the edge
case); and a SHA-256 of the inputs they all belong to.  Data only.  Run where the reference is built; the .npz is the committed fixture.

    python tests/golden/gen_float_kats.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
import float_ref as fr  # noqa: E402

L = fr.load_ref()
if L is None:
    sys.exit("oracle/_ref/libggml_ref.so is not built (make -C oracle ref)")
out = {}
for t in fr.TYPES:
    for key, raw, xs, digest in fr.all_cases(t):
        out[key + "_inputs_sha256"] = np.array(digest)
        ref = fr.reference_outputs(L, t, raw, xs)
        for name in ("sgemm1", "sgemm5", "dots"):
            if name in ref:
                assert np.isfinite(ref[name]).all(), (key, name)
                out[key + "_" + name] = ref[name]
        if "act" in ref:
            out[key + "_act"] = ref["act"]
        out[key + "_to_float"] = ref["to_float"] if key.endswith("_edge") else ref["to_float"][list(fr.DEQ_ROWS)]
np.savez_compressed(os.path.join(HERE, "float_kats.npz"), **out)
print("wrote", os.path.join(HERE, "float_kats.npz"), len(out), "arrays")
