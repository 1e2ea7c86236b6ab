#!/usr/bin/env python3
"""tests/golden/f64_order_kats.npz and f64_softmax_kats.npz: constructed inputs, one per length, on which f32_rounding_safe (bamd_device.h) must send
the double-precision sum down the reference's sequential order WHATEVER tree a kernel uses: the sequential value (the f64 mean of the squares;
1 / the softmax denominator) sits within 8 units of an f32 rounding boundary, any other order of the same n terms within 2 n units of that,
the guard's band is 2 n + 8 (tools/f64_order_search.py construct_near, tools/f64_softmax_search.py construct_row).  Only the inputs and the
expected sequential f32 are stored; what a kernel has to give comes from the oracle at test time (tests/test_gpu_f64_guard.py).  CPU only,
a few minutes, fixed seeds.

  both                   differs_<name>: the restated orders that round to another f32 than the sequential one on this input (may be empty)
  f64_order_kats.npz     x_<name> [K] f32, mean_<name> f32 (sequential), eps;  names K256 K768 K3072 K4096 K4096b K8192
                         (K4096 is the vector of f64_order_kat.npz when it meets the margin: it does)
  f64_softmax_kats.npz   s_<name> [padded] f32 scores (f16-representable, s_0 = 0 the maximum, -inf = masked), scale_<name> f32 (kq_scale),
                         inv_<name> f32 = (float) (1 / sequential sum);  names v<valid>_p<padded>_hd<head dim>[_holes]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
import f64_order_search as fs  # noqa: E402
import f64_softmax_search as ss  # noqa: E402
from oracle import pyoracle as po  # noqa: E402

SCALE = {64: np.float32(0.125), 128: np.float32(1.0) / np.sqrt(np.float32(128.0)), 256: np.float32(0.0625)}     # 1 / sqrtf(hd), llama.cpp:8829
ROWS = [(64, 64, 64), (96, 96, 64), (576, 576, 64), (4128, 4128, 64), (8224, 8224, 64),
        (64, 64, 128), (96, 96, 128), (80, 96, 128), (576, 576, 128), (64, 64, 256)]
LATER = [(448, 448, 128)]                                                 # added behind the holes row, so that the seeds of the rows above stay what they were: the longest row whose micro-batch the matrix-core kernel keeps in LDS (<= 512 positions)
HOLES = (17, 18, 40, 41, 42, 63)                                          # the cells case: masked entries inside the row (v96_p96_hd64_holes)


def differing(f32s):
    """the restated orders (tools/) that round to ANOTHER f32 than the sequential one on this input: where the search found such an input it was kept"""
    return np.array(sorted(n for n, v in f32s.items() if v.view(np.uint32) != f32s["seq"].view(np.uint32)), dtype="U16")


def order_kats():
    out = dict(eps=np.float32(1e-5))
    old = np.load(os.path.join(HERE, "f64_order_kat.npz"))["x"]
    for i, (name, K) in enumerate([("K256", 256), ("K768", 768), ("K3072", 3072), ("K4096", 4096), ("K4096b", 4096), ("K8192", 8192)]):
        rng = np.random.default_rng(20261019 + i)
        if name == "K4096" and int(fs.dist_units(fs.mean64(fs.sum_seq(fs.terms(old)), K))) <= fs.NEAR_UNITS:
            x = old
        else:
            x = fs.construct_near(K, rng)
        assert x is not None, name
        o = fs.sum_orders(fs.terms(x))
        print(name, {n: (int(fs.dist_units(fs.mean64(v, K))), "%08x" % np.float32(fs.mean64(v, K)).view(np.uint32)) for n, v in o.items()}, flush=True)
        out["x_" + name] = x
        out["mean_" + name] = np.float32(fs.mean64(o["seq"], K))
        out["differs_" + name] = differing({n: np.float32(fs.mean64(v, K)) for n, v in o.items()})
    np.savez_compressed(os.path.join(HERE, "f64_order_kats.npz"), **out)


def softmax_kats():
    out = {}
    for i, (valid, padded, hd) in enumerate(ROWS + [(96, 96, 64)] + LATER):
        holes = HOLES if i == len(ROWS) else ()
        name = "v%d_p%d_hd%d%s" % (valid, padded, hd, "_holes" if holes else "")
        rng = np.random.default_rng(20261100 + i)
        s = ss.construct_row(po, rng, valid, padded, SCALE[hd], holes)
        assert s is not None, name
        den = ss.row_denominators(ss.row_exps(po, s, SCALE[hd]))
        print(name, {n: (int(ss.dist(np.array([1.0 / t]))[0]), "%08x" % np.float32(1.0 / t).view(np.uint32)) for n, t in den.items()}, flush=True)
        out["s_" + name] = s
        out["scale_" + name] = SCALE[hd]
        out["inv_" + name] = np.float32(1.0 / den["seq"])
        out["differs_" + name] = differing({n: np.float32(1.0 / t) for n, t in den.items()})
    np.savez_compressed(os.path.join(HERE, "f64_softmax_kats.npz"), **out)


if __name__ == "__main__":
    order_kats()
    softmax_kats()
