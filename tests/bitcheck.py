"""The primitives of the op-level GPU tests: bit comparison of f32 results, the oracle's RMSNorm prologue and silu(gate) * up epilogue, and the epilogue codes
and fill value of bamd_op_mul_mat_batch_seg.  A plain helper module (as goldenio.py)."""
import numpy as np

EPS = 1e-5
STORE, ADD, SILU_MUL = 0, 1, 2
FILL = np.float32(-7.25)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits(a, b, what=""):
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    assert np.isfinite(b).all(), what + ": the expectation is not finite"
    assert a.shape == b.shape, what
    bad = np.flatnonzero(bits(a) != bits(b))
    assert bad.size == 0, "%s: %d/%d elements differ, first at %d: %r vs %r" % (what, bad.size, a.size, bad[0], a.flat[bad[0]], b.flat[bad[0]])


def normed(po, x, w):
    return (po.rms_norm(x, EPS) * w).astype(np.float32)


def silu_mul(po, g, u):
    return po.silu(np.ascontiguousarray(g, np.float32).reshape(-1)).reshape(np.shape(g)) * u
