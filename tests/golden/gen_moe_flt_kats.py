"""Generates tests/golden/moe_flt_kats.npz: what the genuine reference (oracle/_ref/libggml_ref.so, built by `make -C oracle ref`) computes for a row of an F32 or
F16 EXPERT matrix, the way ggml_compute_forward_mul_mat_id calls it: from_float of the type's vec_dot_type over the activation row (F16: the f16 bits are stored),
then the vec_dot of the type traits, row by row.  Inputs: float_ref.all_cases (K 256 .. 4096, 32 rows, three magnitudes, and the edge case).  BF16 experts take the
dot float_kats.npz already holds.  Data only.  Run where the reference is built; the .npz is the committed fixture.

    python tests/golden/gen_moe_flt_kats.py
"""
import ctypes as C
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
p = lambda a: a.ctypes.data_as(C.c_void_p)
out = {}
for t in (fr.F32, fr.F16):
    tr = L.ggml_internal_get_type_traits(t)
    assert tr.vec_dot_type == t
    vec_dot = C.CFUNCTYPE(None, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int)(tr.vec_dot)
    from_float = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int64)(tr.from_float) if t == fr.F16 else None
    for key, raw, xs, digest in fr.all_cases(t):
        K = xs[0].size
        raw = np.ascontiguousarray(raw, np.uint8)
        dots = np.zeros((len(xs), fr.ROWS), np.float32)
        acts = np.zeros((len(xs), K), np.uint16)
        for i, x in enumerate(xs):
            a = np.ascontiguousarray(x, np.float32)
            if from_float:
                from_float(p(a), p(acts[i]), K)
                a = acts[i]
            for r in range(fr.ROWS):
                s = C.c_float(0)
                vec_dot(K, C.byref(s), 0, C.c_void_p(raw.ctypes.data + r * K * fr.ESIZE[t]), 0, p(a), 0, 1)
                dots[i, r] = s.value
        out[key + "_inputs_sha256"] = np.array(digest)
        out[key + "_dots"] = dots
        if from_float:
            out[key + "_act"] = acts
np.savez_compressed(os.path.join(HERE, "moe_flt_kats.npz"), **out)
print("wrote", os.path.join(HERE, "moe_flt_kats.npz"), len(out), "arrays")
