"""CPU: Q4_1 / Q5_1 with Q8_1 activations.  The numpy restatement of quantize_row_q8_1, the two chains and the dequantisers (tests/legacy1_ref.py) must
reproduce, bit for bit, every stored output of the genuine reference (tests/golden/legacy1_kats.npz, written by tests/golden/gen_legacy1_kats.py) — with the
scalar statements `summs += a * b` and `x * d + m` as a separate multiply and add AND as fused ones: their products are exact in f32, so the stored answers
cannot tell the two forms apart and need not (legacy1_ref's module text).  Also: the stored outputs belong to
today's seeded inputs, Q8_1 shares d and bytes with Q8_0, the edge case reaches its edges, and the Python GGUF side knows the two types' sizes and the four
recipes that produce them."""
import hashlib
import os

import numpy as np
import pytest

import legacy1_ref as l1
import legacy_ref as lg
from conftest import GOLDEN

KATS = os.path.join(GOLDEN, "legacy1_kats.npz")
TYPES = list(l1.TYPES)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def stored():
    return np.load(KATS)


def stored_case(stored, key, digest):
    assert str(stored[key + "_inputs_sha256"]) == digest, "%s: the stored outputs belong to other inputs (regenerate with tests/golden/gen_legacy1_kats.py)" % key
    return stored[key + "_dots"], [str(s) for s in stored[key + "_q8_sha256"]], stored[key + "_dequant"]


def test_fixture_is_no_larger_than_its_sibling():
    assert os.path.getsize(KATS) <= os.path.getsize(os.path.join(GOLDEN, "legacy_kats.npz"))


@pytest.mark.parametrize("contracted", [False, True], ids=["mul_add", "fma"])
@pytest.mark.parametrize("t", TYPES)
def test_restatement_reproduces_the_reference(stored, t, contracted):
    for key, blocks, xs, digest, deq_rows in l1.all_cases(t):
        dots, q8sha, deq = stored_case(stored, key, digest)
        assert np.isfinite(dots).all() and np.isfinite(deq).all(), key
        K = xs[0].size
        rb = K // 32 * l1.BB[t]
        for i, x in enumerate(xs):
            q8 = l1.quantize_row_q8_1(x)
            assert hashlib.sha256(np.ascontiguousarray(q8).tobytes()).hexdigest() == q8sha[i], "%s vector %d: Q8_1 bytes differ from the reference's" % (key, i)
            assert np.array_equal(l1.q8_1_as_q8_0(q8), lg.quantize_row_q8_0(x)), "%s vector %d: Q8_1 d / bytes differ from Q8_0's" % (key, i)
            got = l1.vec_dot_rows(t, blocks, q8, contracted=contracted)
            bad = np.flatnonzero(bits(got) != bits(dots[i]))
            assert bad.size == 0, "%s vector %d: %d rows differ, first %d: %r vs %r" % (key, i, bad.size, bad[0], got[bad[0]], dots[i][bad[0]])
        for i, r in enumerate(deq_rows):
            got = l1.dequantize(t, blocks[r * rb:(r + 1) * rb], contracted=contracted)
            assert np.array_equal(bits(got), bits(deq[i])), "%s: dequantised row %d differs" % (key, r)


@pytest.mark.parametrize("t", TYPES)
def test_scalar_products_are_exact_in_f32(t):
    """why the two forms agree: m_w * s_x (two widened f16) and q * d (an integer below 32 times a widened f16) are exact in f32 on the edge case too"""
    blocks, xs, _, _, _ = l1.edge_case(t)
    d, m, q = l1.unpack(t, blocks)
    for x in xs:
        _, s, _ = l1.q8_1_fields(l1.quantize_row_q8_1(x))
        p64 = m.astype(np.float64)[:, None] * s.astype(np.float64)[None, :]
        assert np.array_equal(p64, (m[:, None] * s[None, :]).astype(np.float32).astype(np.float64))
    p64 = q.astype(np.float64) * d.astype(np.float64)[:, None]
    assert np.array_equal(p64, (q.astype(np.float32) * d[:, None]).astype(np.float32).astype(np.float64))


def test_overflow_vector(stored):
    """a block of 32 equal values of +-4096: s = f16(32 * 4096) = +-inf, in the reference and in the restatement; stored by digest, used in no dot"""
    x = l1.overflow_vector()
    assert hashlib.sha256(x.tobytes()).hexdigest() == str(stored["overflow_inputs_sha256"])
    q8 = l1.quantize_row_q8_1(x)
    assert hashlib.sha256(q8.tobytes()).hexdigest() == str(stored["overflow_q8_sha256"])
    _, s, q = l1.q8_1_fields(q8)
    assert np.isposinf(s[3]) and np.isneginf(s[5]) and (q[3] == 127).all() and (q[5] == -127).all()
    assert np.array_equal(l1.q8_1_as_q8_0(q8), lg.quantize_row_q8_0(x))


def test_double_rounding_vector(stored):
    """s = f16(f32(d * sum)): two roundings.  Every block of this vector gives another f16 when the exact product is rounded once; the reference's bytes (by
    digest) are the restatement's"""
    x = l1.double_rounding_vector()
    assert x.size == l1.ROUND2_K and hashlib.sha256(x.tobytes()).hexdigest() == str(stored["round2_inputs_sha256"])
    q8 = l1.quantize_row_q8_1(x)
    assert hashlib.sha256(q8.tobytes()).hexdigest() == str(stored["round2_q8_sha256"])
    _, s, q = l1.q8_1_fields(q8)
    d32 = (np.abs(x.reshape(-1, 32)).max(axis=1) / np.float32(127.0)).astype(np.float32)
    once = (d32.astype(np.float64) * q.sum(axis=1)).astype(np.float16).astype(np.float32)
    assert np.isfinite(s).all() and (once != s).all()


@pytest.mark.parametrize("t", TYPES)
def test_edge_case_reaches_its_edges(t):
    """every weight kind and every activation kind occurs; the quants reach both ends; d is negative, zero, subnormal and large somewhere, m is zero,
    negative and large somewhere; the activation blocks include all-zero ones, negative extrema, exact ties, blocks whose f16 d is subnormal or zero under
    non-zero quants, single values, and blocks of equal values with |sum| = 4064"""
    blocks, xs, digest, wtags, xtags = l1.edge_case(t)
    assert set(wtags.reshape(-1)) == set(l1.EDGE_WKINDS[t]) and set(xtags.reshape(-1)) == set(l1.EDGE_AKINDS)
    d, m, q = l1.unpack(t, blocks)
    assert (q == 0).all(axis=1).any() and (q == l1.QMAX[t]).all(axis=1).any()
    raw = blocks.reshape(-1, l1.BB[t])
    d16 = np.ascontiguousarray(raw[:, 0:2]).view(np.uint16).reshape(-1)
    m16 = np.ascontiguousarray(raw[:, 2:4]).view(np.uint16).reshape(-1)
    assert (((d16 & 0x7c00) == 0) & ((d16 & 0x3ff) != 0)).any() and ((d16 & 0x7fff) == 0).any() and (d16 & 0x8000).any() and (np.abs(d) >= 100).any()
    assert ((m16 & 0x7fff) == 0).any() and (m < 0).any() and (m > 0).any() and (np.abs(m) >= 100).any()
    assert np.isfinite(d).all() and np.isfinite(m).all()
    if t == l1.Q5_1:
        qh = np.ascontiguousarray(raw[:, 4:8]).view(np.uint32).reshape(-1)
        assert (qh == 0).any() and (qh == 0xffffffff).any()
    seen = dict(zero=False, neg=False, tie=False, tiny=False, single=False, equal=False)
    for x in xs:
        yd, ys, qa = l1.q8_1_fields(l1.quantize_row_q8_1(x))
        assert np.isfinite(ys).all()
        xb = x.reshape(-1, 32)
        amax = np.abs(xb).max(axis=1)
        seen["zero"] |= bool(((amax == 0) & (yd == 0) & (ys == 0) & (qa == 0).all(axis=1)).any())
        seen["neg"] |= bool((xb.min(axis=1) == -amax)[amax > 0].any())
        sc = xb * np.where(amax != 0, np.float32(127.0) / np.where(amax != 0, amax, 1), 0).astype(np.float32)[:, None]
        seen["tie"] |= bool((np.abs(sc - np.trunc(sc)) == 0.5).any())
        seen["tiny"] |= bool(((yd < 6.2e-5) & (np.abs(qa).max(axis=1) == 127)).any())
        seen["single"] |= bool(((xb != 0).sum(axis=1) == 1).any())
        seen["equal"] |= bool((np.abs(qa.sum(axis=1)) == 4064).any())
    assert all(seen.values()), seen


# ---- the Python GGUF side ------------------------------------------------------------------------------------------------------------------------
def test_type_table_and_tensor_sizes():
    from booster_amd import gguf
    assert (gguf.Q4_1, gguf.Q5_1) == (3, 7)
    assert [gguf.TYPE_NAMES[t] for t in (3, 7)] == ["Q4_1", "Q5_1"]
    for t, bb in ((gguf.Q4_1, 20), (gguf.Q5_1, 24)):
        assert gguf.GGML_TYPES[t] == (32, bb)
        assert gguf.tensor_nbytes(t, [4096, 13]) == 13 * 128 * bb
        w = gguf.random_q1_tensor(t, 512, 5, np.random.default_rng(1))
        assert w.dtype == np.uint8 and w.size == gguf.tensor_nbytes(t, [512, 5])
        dm = np.ascontiguousarray(w.reshape(-1, bb)[:, 0:4]).view(np.float16).astype(np.float32)
        assert np.isfinite(dm).all() and (dm[:, 0] > 0).any() and (dm[:, 0] < 0).any() and (dm[:, 1] > 0).any() and (dm[:, 1] < 0).any()
        big = gguf.random_q1_tensor(t, 4096, 64, np.random.default_rng(2)).reshape(-1, bb)
        assert len(np.unique(big[:, 4:])) == 256                                  # every byte pattern in qs / qh
        # the dequantised values are of the Q4_0 / Q5_0 tensors' magnitude: zero-mean-ish, standard deviation ~ 1 / sqrt(row_len)
        v = l1.dequantize(t, big.reshape(-1))
        assert 0.5 / 64 < v.std() < 2.0 / 64 and abs(v.mean()) < 0.25 / 64


def test_recipes():
    """llama_tensor_get_type: Q4_1 / Q5_1 everywhere but output.weight, which is Q6_K; with an importance matrix the Q4_0 / Q5_0 recipes write ffn_down of
    the first n_layer / 8 layers as Q4_1 / Q5_1 (llama.cpp:15618-15624) and are the plain recipes otherwise"""
    from booster_amd import gguf
    names = ("token_embd", "output", "attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down")
    for n_layer in (2, 8, 32):
        for il in range(n_layer):
            for n in names:
                assert gguf.q4_1_type(n, il, n_layer) == (gguf.Q6_K if n == "output" else gguf.Q4_1)
                assert gguf.q5_1_type(n, il, n_layer) == (gguf.Q6_K if n == "output" else gguf.Q5_1)
                first = n == "ffn_down" and il < n_layer // 8
                assert gguf.q4_0_imatrix_type(n, il, n_layer) == (gguf.Q4_1 if first else gguf.q4_0_type(n, il, n_layer))
                assert gguf.q5_0_imatrix_type(n, il, n_layer) == (gguf.Q5_1 if first else gguf.q5_0_type(n, il, n_layer))
    assert [il for il in range(32) if gguf.q4_0_imatrix_type("ffn_down", il, 32) == gguf.Q4_1] == [0, 1, 2, 3]
    assert [il for il in range(8) if gguf.q5_0_imatrix_type("ffn_down", il, 8) == gguf.Q5_1] == [0]
    assert all(gguf.q4_0_imatrix_type("ffn_down", il, 2) == gguf.Q4_0 for il in range(2))


@pytest.mark.parametrize("recipe", ["q4_1", "q5_1", "q4_0_imatrix", "q5_0_imatrix"])
def test_tiny_file_round_trips(tmp_path, recipe):
    from booster_amd import gguf
    E, H, Hkv, Lyr, F, V = 256, 4, 1, 8, 512, 64
    rf = getattr(gguf, recipe + "_type")
    embd = rf("token_embd", 0, Lyr)
    path = str(tmp_path / (recipe + ".gguf"))
    gguf.write_synthetic_llama(path, E, H, Hkv, Lyr, F, V, type_fn=lambda n, il: rf(n, il, Lyr), embd_type=embd, seed=11)
    r = gguf.GGUFReader(path)
    for il in range(Lyr):
        for nm in ("attn_q", "attn_v", "attn_output", "ffn_up", "ffn_down"):
            ti = r.tensors["blk.%d.%s.weight" % (il, nm)]
            want = rf(nm, il, Lyr)
            assert ti["type"] == want, (il, nm, ti["type"])
            assert ti["data"].size == int(np.prod(ti["shape"])) // 32 * gguf.GGML_TYPES[want][1]
    assert r.tensors["token_embd.weight"]["type"] == embd and r.tensors["output.weight"]["type"] == gguf.Q6_K
    down0 = r.tensors["blk.0.ffn_down.weight"]["type"]
    assert down0 == {"q4_1": gguf.Q4_1, "q5_1": gguf.Q5_1, "q4_0_imatrix": gguf.Q4_1, "q5_0_imatrix": gguf.Q5_1}[recipe]
