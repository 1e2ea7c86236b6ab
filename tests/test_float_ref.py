"""The numpy restatement of the F32 / F16 / BF16 chains (tests/float_ref.py) against the genuine reference's stored answers (tests/golden/float_kats.npz,
recorded by tests/golden/gen_float_kats.py from oracle/_ref/libggml_ref.so).  Equal bits everywhere; no tolerance."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float_ref as fr  # noqa: E402

KATS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "float_kats.npz")


@pytest.fixture(scope="module")
def stored():
    return np.load(KATS)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def cases(t):
    return list(fr.all_cases(t))


@pytest.mark.parametrize("t", fr.TYPES)
def test_inputs_are_the_recorded_ones(stored, t):
    for key, raw, xs, digest in cases(t):
        assert str(stored[key + "_inputs_sha256"]) == digest, key


@pytest.mark.parametrize("t", fr.SGEMM_TYPES)
def test_sgemm_chain(stored, t):
    """the 8-lane fma chain with f32 activations equals llamafile_sgemm at n = 1, for every vector and row"""
    for key, raw, xs, _ in cases(t):
        K = xs[0].size
        got = np.stack([fr.mul_mat(t, raw, fr.ROWS, K, x) for x in xs])
        assert np.array_equal(bits(got), bits(stored[key + "_sgemm1"])), key


@pytest.mark.parametrize("t", fr.SGEMM_TYPES)
def test_batching_moves_no_bits(stored, t):
    """llamafile_sgemm at n = 5 gives, column by column, what n = 1 gave for the same vectors: the chain of an output does not depend on the tile it is in"""
    for key, raw, xs, _ in cases(t):
        cols = fr.SGEMM_COLS(len(xs))
        assert np.array_equal(bits(stored[key + "_sgemm5"]), bits(stored[key + "_sgemm1"][cols])), key


def test_f16_activations_are_not_rounded(stored):
    """a restatement that rounds the activations to f16 (ggml_vec_dot_f16's operands) does not reproduce the recorded answers"""
    key, raw, xs, _ = cases(fr.F16)[3]
    K = xs[0].size
    with np.errstate(all="ignore"):
        wrong = np.stack([fr.mul_mat(fr.F16, raw, fr.ROWS, K, x.astype(np.float16).astype(np.float32)) for x in xs])
    assert not np.array_equal(bits(wrong), bits(stored[key + "_sgemm1"]))


def test_bf16_rounding(stored):
    """integer round-to-nearest-even: ties of both parities, f32 subnormals kept, NaN quieted"""
    for key, raw, xs, _ in cases(fr.BF16):
        for i, x in enumerate(xs):
            assert np.array_equal(fr.bf16_bits(x), stored[key + "_act"][i]), (key, i)
    special = np.array([0x7fc00001, 0x7f800001, 0xff800001, 0x7f800000, 0x00008000, 0x00018000, 0x7f7fffff, 0x80000001], np.uint32).view(np.float32)
    assert fr.bf16_bits(special).tolist() == [0x7fc0, 0x7fc0, 0xffc0, 0x7f80, 0x0000, 0x0002, 0x7f80, 0x8000]


def test_bf16_chain(stored):
    for key, raw, xs, _ in cases(fr.BF16):
        K = xs[0].size
        got = np.stack([fr.mul_mat(fr.BF16, raw, fr.ROWS, K, x) for x in xs])
        assert np.array_equal(bits(got), bits(stored[key + "_dots"])), key


def test_bf16_products_are_not_fused(stored):
    """the edge vectors hold bf16 x bf16 products below 2^-126: there a fused multiply-add differs from add(mul(w, x), c), and the recorded answers are the
    latter's (what the kernels write with __fmul_rn / __fadd_rn)"""
    assert fr.BF16_FUSED is False
    raw, xs, _, _, _ = fr.edge_case(fr.BF16)
    w = fr.to_f32(fr.BF16, raw).reshape(fr.ROWS, fr.EDGE_K)
    fused = np.stack([fr.vec_dot_bf16_rows(w, fr.bf16_bits(x), fused=True) for x in xs])
    assert not np.array_equal(bits(fused), bits(stored["bf16_edge_dots"]))


@pytest.mark.parametrize("t", fr.TYPES)
def test_edge_case_reaches_the_subnormal_range(stored, t):
    """the recorded edge answers hold non-zero results below 2^-126 (products and partial sums in the subnormal range are the result there)"""
    a = stored["%s_edge_%s" % (fr.NAME[t], "dots" if t == fr.BF16 else "sgemm1")]
    assert ((np.abs(a) < 2.0 ** -126) & (a != 0)).sum() >= 4


@pytest.mark.parametrize("t", fr.TYPES)
def test_to_float(stored, t):
    for key, raw, xs, _ in cases(t):
        K = xs[0].size
        w = fr.to_f32(t, raw).reshape(fr.ROWS, K)
        want = stored[key + "_to_float"]
        got = w if key.endswith("_edge") else w[list(fr.DEQ_ROWS)]
        assert np.array_equal(bits(got), bits(want)), key


def test_gguf_helpers():
    """booster_amd.gguf's bf16 conversion is the same rounding; the seeded float tensors are finite and of the asked size"""
    from booster_amd import gguf
    x = np.concatenate([c[2][0] for c in cases(fr.BF16)])
    assert np.array_equal(gguf.f32_to_bf16(x), fr.bf16_bits(x))
    rng = np.random.default_rng(1)
    for t in fr.TYPES:
        raw = gguf.random_float_tensor(t, 256, 8, rng)
        assert raw.dtype == np.uint8 and raw.size == gguf.tensor_nbytes(t, [256, 8])
        assert np.isfinite(fr.to_f32(t, raw)).all()
    assert gguf.f16_type("attn_q", 0, 2) == gguf.F16 and gguf.bf16_type("output", 0, 2) == gguf.BF16 and gguf.f32_type("ffn_up", 1, 2) == gguf.F32
