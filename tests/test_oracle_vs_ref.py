"""CPU: the oracle against the genuine reference (oracle/_ref/libggml_ref.so, compiled in place by `make -C oracle ref`).
Where that library is built, the reference runs live and must also reproduce the stored outputs; elsewhere its outputs come from
tests/golden/dot_kats.npz (tests/golden/gen_dot_kats.py), so the oracle is held to the same bits on every machine."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

REF = os.path.join(ROOT, "oracle", "_ref", "libggml_ref.so")
KATS = os.path.join(GOLDEN, "dot_kats.npz")
CASES = [(12, 144, "ggml_vec_dot_q4_K_q8_K"), (13, 176, "ggml_vec_dot_q5_K_q8_K"), (14, 210, "ggml_vec_dot_q6_K_q8_K")]
KS = [256, 1024, 14336]
SCALES = (1e-3, 1.0, 50.0)
ROWS = 32


def load_ref():
    """the reference library, or None where it is not built or cannot be loaded"""
    if not os.path.exists(REF):
        return None
    try:
        L = C.CDLL(REF)
    except OSError:
        return None
    class _InitParams(C.Structure):
        _fields_ = [("mem_size", C.c_size_t), ("mem_buffer", C.c_void_p), ("no_alloc", C.c_bool)]
    # ggml_init fills the f16->f32 lookup table that GGML_FP16_TO_FP32 reads on x86
    L.ggml_init.restype = C.c_void_p
    L.ggml_init.argtypes = [_InitParams]
    L.ggml_init(_InitParams(1 << 20, None, False))
    L.ggml_quantize_chunk.restype = C.c_size_t
    L.ggml_quantize_chunk.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]
    L.quantize_row_q8_K.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    for n in ("ggml_vec_dot_q4_K_q8_K", "ggml_vec_dot_q5_K_q8_K", "ggml_vec_dot_q6_K_q8_K"):
        getattr(L, n).argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]
    return L


@pytest.fixture(scope="module")
def ref():
    return load_ref()


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def case_inputs(t, K):
    """Random raw blocks (every bit pattern of scales/quants), random activations, several magnitudes; and a digest of them"""
    from booster_amd.gguf import random_kquant_tensor
    rng = np.random.default_rng(K + t)
    blocks = random_kquant_tensor(t, K, ROWS, rng)
    xs = [(rng.standard_normal(K) * scale).astype(np.float32) for scale in SCALES]
    h = hashlib.sha256(np.ascontiguousarray(blocks).tobytes())
    for x in xs:
        h.update(x.tobytes())
    return blocks, xs, h.hexdigest()


def reference_outputs(L, bb, fn, K, blocks, xs):
    """per activation vector: the reference's Q8_K bytes of it and its dot product with every row"""
    out = []
    rb = K // 256 * bb
    for x in xs:
        q8r = np.zeros(K // 256 * 292, np.uint8)
        L.quantize_row_q8_K(p(x), p(q8r), K)
        want = np.zeros(ROWS, np.float32)
        for r in range(ROWS):
            s = C.c_float(0)
            getattr(L, fn)(K, C.byref(s), 0, C.c_void_p(blocks.ctypes.data + r * rb), 0, p(q8r), 0, 1)
            want[r] = s.value
        out.append((q8r, want))
    return out


def stored_outputs(fn, K, digest):
    kats = np.load(KATS)
    key = "%s_K%d" % (fn, K)
    assert str(kats[key + "_inputs_sha256"]) == digest, "the inputs of %s differ from those the stored outputs were made from" % key
    return [(kats["%s_q8_%d" % (key, i)], kats["%s_dot_%d" % (key, i)]) for i in range(len(SCALES))]


@pytest.mark.parametrize("t,bb,fn", CASES)
@pytest.mark.parametrize("K", KS)
def test_dot_random_bytes(po, ref, t, bb, fn, K):
    blocks, xs, digest = case_inputs(t, K)
    stored = stored_outputs(fn, K, digest)
    if ref is not None:
        live = reference_outputs(ref, bb, fn, K, blocks, xs)
        for (q8s, ws), (q8l, wl) in zip(stored, live):
            assert np.array_equal(q8s, q8l) and np.array_equal(ws.view(np.uint32), wl.view(np.uint32)), "tests/golden/dot_kats.npz differs from the live reference"
    for x, (q8r, want) in zip(xs, stored):
        assert np.array_equal(po.quantize_q8_K(x), q8r)
        got = po.mul_mat_q(t, blocks, ROWS, K, x)[0]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
