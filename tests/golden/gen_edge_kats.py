"""Generates tests/golden/edge_kats.npz: the genuine reference's outputs (oracle/_ref/libggml_ref.so, built by `make -C oracle ref`) for the
edge inputs of tests/test_oracle_edges.py — quantize_row_q8_K bytes and ggml_vec_dot_q*_K_q8_K results, ggml_silu, ggml_soft_max_ext and
ggml_rms_norm through the graph API — with a SHA-256 of the inputs they belong to.  Run where the reference is built; the .npz is the
committed fixture.  The archive is written with fixed member order and time stamps, so that a second run reproduces it byte for byte.

    python tests/golden/gen_edge_kats.py
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
import test_oracle_edges as t  # noqa: E402

L = t.load_ref()
if L is None:
    sys.exit("oracle/_ref/libggml_ref.so is not built (make -C oracle ref)")
out = t.reference_outputs(L)
path = os.path.join(HERE, "edge_kats.npz")
with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
    for k in sorted(out):
        buf = io.BytesIO()
        np.lib.format.write_array(buf, np.asanyarray(out[k]), allow_pickle=False)
        zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
        zi.compress_type = zipfile.ZIP_DEFLATED
        z.writestr(zi, buf.getvalue())
print("wrote", path, len(out), "arrays")
