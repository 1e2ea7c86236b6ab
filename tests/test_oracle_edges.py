"""CPU: the oracle against the genuine reference at the value edges of tests/edge_inputs.py.  The reference's outputs are stored in
tests/golden/edge_kats.npz (tests/golden/gen_edge_kats.py) with a SHA-256 of the inputs they belong to; where oracle/_ref/libggml_ref.so is
built (`make -C oracle ref`) the reference also runs live and must reproduce them, as in tests/test_oracle_vs_ref.py.  Pinned here:
  quantize_row_q8_K + ggml_vec_dot_q{4,5,6}_K_q8_K   every weight kind x every activation kind, K = 256 / 1024 / 14336
  ggml_silu (bo_v_silu, bo_v_expf)                   a dense sweep of [-140, 140], concentrated at +-87.3, +-88.7, +-103.9, +-133.1, every f32
                                                     around the two branch points of v_expf, +-0, f32 subnormals, +-1e4
  ggml_soft_max_ext (mask, scale) (bo_soft_max)      rows whose scaled scores reach past -150
  ggml_rms_norm (bo_rms_norm)                        zero, tiny, vanishing, huge and overflowing rows
"""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import edge_inputs as E
from conftest import GOLDEN
from test_oracle_vs_ref import load_ref

KATS = os.path.join(GOLDEN, "edge_kats.npz")
DOTS = [(12, "ggml_vec_dot_q4_K_q8_K"), (13, "ggml_vec_dot_q5_K_q8_K"), (14, "ggml_vec_dot_q6_K_q8_K")]
KS = [256, 1024, 14336]
ROWS = 16
SM_N, SM_ROWS, SM_SCALE = 256, 16, 0.125
RMS_N, RMS_EPS = 4096, 1e-5
LOG2E = 1.4426950408889634
FLT_MIN = 2.0 ** -126


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


# ---- inputs ------------------------------------------------------------------------------------------------
def dot_inputs(t, K):
    """ROWS edge rows and enough edge activation vectors to reach every activation kind"""
    rng = np.random.default_rng(9000 + 10 * t + K // 256)
    W, _, X, _ = E.edge_matvec_inputs(t, K, ROWS, rng, n_vec=-(-len(E.ACT_KINDS) // (K // 256)))
    return W, X


def silu_inputs():
    parts = [np.linspace(-140, 140, 8192)]
    parts += [np.linspace(s * c - 0.6, s * c + 0.6, 1024) for c in (87.3, 88.7, 103.9, 133.1) for s in (1, -1)]
    for b in (126.5, 192.5):                                      # |n| = rint(|x| log2 e) crosses 126 / 192 here
        u = np.float32(b / LOG2E).view(np.uint32) + np.arange(-64, 64, dtype=np.int64)
        v = u.astype(np.uint32).view(np.float32)
        parts += [v, -v]
    parts.append([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, FLT_MIN, -FLT_MIN, 1e4, -1e4, 87.0, -87.0])
    x = np.concatenate([np.asarray(p, np.float32) for p in parts])
    return np.concatenate([x, np.zeros(-x.size % 8, np.float32)])          # the reference's AVX2 loop covers whole rows of 8


def soft_max_inputs():
    rng = np.random.default_rng(77)
    s = (rng.standard_normal((SM_ROWS, SM_N)) * 400).astype(np.float32)
    mask = np.zeros((SM_ROWS, SM_N), np.float32)
    for r in range(SM_ROWS):
        mask[r, 1 + int(rng.integers(0, SM_N)) if r else SM_N:] = -np.inf   # row 0 unmasked; row r keeps a random prefix
    mask[1, 1:] = -np.inf                                          # one score left
    return s, mask


def rms_inputs():
    g = np.random.default_rng(78).standard_normal(RMS_N)
    rows = [np.where(g < 0, -0.0, 0.0), g * 1e-21, g * 1e-30, g * 1e17, g * 1e20, g]
    return np.stack(rows).astype(np.float32)


# ---- the reference ---------------------------------------------------------------------------------------------
class _InitParams(C.Structure):
    _fields_ = [("mem_size", C.c_size_t), ("mem_buffer", C.c_void_p), ("no_alloc", C.c_bool)]


def _graph_api(L):
    vp = C.c_void_p
    L.ggml_init.restype = vp; L.ggml_init.argtypes = [_InitParams]
    L.ggml_free.argtypes = [vp]
    L.ggml_new_tensor_2d.restype = vp; L.ggml_new_tensor_2d.argtypes = [vp, C.c_int, C.c_int64, C.c_int64]
    L.ggml_get_data.restype = vp; L.ggml_get_data.argtypes = [vp]
    L.ggml_silu.restype = vp; L.ggml_silu.argtypes = [vp, vp]
    L.ggml_rms_norm.restype = vp; L.ggml_rms_norm.argtypes = [vp, vp, C.c_float]
    L.ggml_soft_max_ext.restype = vp; L.ggml_soft_max_ext.argtypes = [vp, vp, vp, C.c_float, C.c_float]
    L.ggml_new_graph.restype = vp; L.ggml_new_graph.argtypes = [vp]
    L.ggml_build_forward_expand.argtypes = [vp, vp]
    L.ggml_graph_compute_with_ctx.argtypes = [vp, vp, C.c_int]


def _run_graph(L, op, x, *more):
    """op(ctx, tensor of x, tensors of more) through ggml_graph_compute_with_ctx (f32 [rows][n] in, f32 out of x's shape)"""
    ctx = L.ggml_init(_InitParams(256 << 20, None, False))
    try:
        ts = []
        for a in (x,) + more:
            a = np.ascontiguousarray(a, np.float32).reshape(-1, a.shape[-1])
            t = L.ggml_new_tensor_2d(ctx, 0, a.shape[1], a.shape[0])
            C.memmove(L.ggml_get_data(t), a.ctypes.data, a.nbytes)
            ts.append(t)
        out = op(ctx, *ts)
        gf = L.ggml_new_graph(ctx)
        L.ggml_build_forward_expand(gf, out)
        assert L.ggml_graph_compute_with_ctx(ctx, gf, 1) == 0
        y = np.empty(x.shape, np.float32)
        C.memmove(y.ctypes.data, L.ggml_get_data(out), y.nbytes)
        return y
    finally:
        L.ggml_free(ctx)


def reference_outputs(L):
    """every stored array of edge_kats.npz, computed by the reference library L"""
    _graph_api(L)
    out = {}
    for t, fn in DOTS:
        for K in KS:
            W, X = dot_inputs(t, K)
            key = "%s_K%d" % (fn, K)
            rb = K // 256 * E.BLOCK_BYTES[t]
            q8 = np.zeros((len(X), K // 256 * 292), np.uint8)
            dots = np.zeros((len(X), ROWS), np.float32)
            for i, x in enumerate(X):
                L.quantize_row_q8_K(_p(x), _p(q8[i]), K)
                for r in range(ROWS):
                    s = C.c_float(0)
                    getattr(L, fn)(K, C.byref(s), 0, C.c_void_p(W.ctypes.data + r * rb), 0, _p(q8[i]), 0, 1)
                    dots[i, r] = s.value
            out[key + "_sha256"] = np.array(digest(W, X))
            out[key + "_q8"], out[key + "_dot"] = q8, dots
    x = silu_inputs()
    out["silu_sha256"] = np.array(digest(x))
    out["silu_y"] = _run_graph(L, L.ggml_silu, x[None])[0]
    s, mask = soft_max_inputs()
    out["soft_max_sha256"] = np.array(digest(s, mask))
    out["soft_max_p"] = _run_graph(L, lambda ctx, a, m: L.ggml_soft_max_ext(ctx, a, m, SM_SCALE, 0.0), s, mask)
    x = rms_inputs()
    out["rms_norm_sha256"] = np.array(digest(x))
    out["rms_norm_y"] = _run_graph(L, lambda ctx, a: L.ggml_rms_norm(ctx, a, RMS_EPS), x)
    return out


# ---- the tests ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stored():
    return dict(np.load(KATS))


@pytest.fixture(scope="module")
def live():
    """the reference's outputs where it is built (None elsewhere)"""
    L = load_ref()
    return None if L is None else reference_outputs(L)


def check_stored(stored, live, *keys):
    for k in keys:
        if live is not None:
            assert np.array_equal(stored[k], live[k]), "tests/golden/edge_kats.npz differs from the live reference at " + k


@pytest.mark.parametrize("t,fn", DOTS)
@pytest.mark.parametrize("K", KS)
def test_dot_edges(po, stored, live, t, fn, K):
    W, X = dot_inputs(t, K)
    key = "%s_K%d" % (fn, K)
    assert str(stored[key + "_sha256"]) == digest(W, X), "the inputs of %s differ from those the stored outputs were made from" % key
    check_stored(stored, live, key + "_q8", key + "_dot")
    q8s, dots = stored[key + "_q8"], stored[key + "_dot"]
    assert np.isfinite(dots).all()
    assert sum(E.odd_pair_sums_above_2048(q) for q in q8s) >= 8                                 # the S_h / S_l split
    d = np.concatenate([E.q8_fields(q)[0] for q in q8s])
    assert (d == 0).sum() >= 2 and (d > 0).any() and (d < 0).any()                              # zero and overflowing-iscale blocks: d = +-0
    for i, x in enumerate(X):
        assert np.array_equal(po.quantize_q8_K(x), q8s[i]), "%s vector %d: Q8_K bytes" % (key, i)
        assert bits_equal(po.mul_mat_q(t, W, ROWS, K, x)[0], dots[i]), "%s vector %d: dot products" % (key, i)


def test_silu_edges(po, stored, live):
    x = silu_inputs()
    assert str(stored["silu_sha256"]) == digest(x)
    check_stored(stored, live, "silu_y")
    want = stored["silu_y"]
    n = np.abs(np.rint(-x.astype(np.float64) * LOG2E))
    assert np.count_nonzero((n > 126) & (n <= 192)) >= 500 and np.count_nonzero(n > 192) >= 500            # both branches of v_expf
    assert np.count_nonzero((want == 0) & (x < 0)) >= 500 and np.count_nonzero((np.abs(x) < FLT_MIN) & (x != 0)) >= 4
    assert np.isfinite(want).all()
    assert bits_equal(po.silu(x), want)
    assert bits_equal(np.array([po.lib().bo_v_silu(float(v)) for v in x[::97]], np.float32), want[::97])


def test_soft_max_edges(po, stored, live):
    s, mask = soft_max_inputs()
    assert str(stored["soft_max_sha256"]) == digest(s, mask)
    check_stored(stored, live, "soft_max_p")
    want = stored["soft_max_p"]
    assert np.isfinite(want).all()
    w = s * np.float32(SM_SCALE) + mask
    rel = w - w.max(axis=1, keepdims=True)
    assert (rel[np.isfinite(rel)] < -150).sum() >= SM_ROWS * 8
    assert np.count_nonzero((want > 0) & (want < FLT_MIN)) >= 8 and np.count_nonzero((want == 0) & np.isfinite(mask)) >= 100
    assert want[1, 0] == 1.0
    for r in range(SM_ROWS):
        assert bits_equal(po.soft_max(s[r], mask[r], SM_SCALE), want[r]), "soft_max row %d" % r


def test_rms_norm_edges(po, stored, live):
    x = rms_inputs()
    assert str(stored["rms_norm_sha256"]) == digest(x)
    check_stored(stored, live, "rms_norm_y")
    want = stored["rms_norm_y"]
    assert np.isfinite(want).all()
    with np.errstate(over="ignore", under="ignore"):
        sq = x * x
    assert np.isinf(sq[4]).any() and not want[4].any()                                         # sum of squares inf: scale 0
    assert ((sq[1] > 0) & (sq[1] < FLT_MIN)).sum() > RMS_N // 2 and not sq[2].any()
    for r in range(len(x)):
        assert bits_equal(po.rms_norm(x[r], RMS_EPS), want[r]), "rms_norm row %d" % r
