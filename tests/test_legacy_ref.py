"""CPU: Q8_0 / Q4_0 / Q5_0.  The numpy restatement of quantize_row_q8_0, the eight-lane chain and the dequantisers (tests/legacy_ref.py) must reproduce, bit
for bit, every stored output of the genuine reference (tests/golden/legacy_kats.npz, written by tests/golden/gen_legacy_kats.py); the two reference entry
points stored for Q8_0 / Q4_0 (ggml_vec_dot_q*_0_q8_0 and llamafile_sgemm at n = 1 and n = 5) must hold the same bits.  Also: the Python GGUF side knows the three types' sizes and recipes, and a tiny file of
each recipe round-trips through the writer and the reader."""
import hashlib
import os

import numpy as np
import pytest

import legacy_ref as lg
from conftest import GOLDEN
from legacy_ref import all_cases

KATS = os.path.join(GOLDEN, "legacy_kats.npz")
TYPES = list(lg.TYPES)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def stored():
    return np.load(KATS)


def stored_case(stored, key, digest):
    assert str(stored[key + "_inputs_sha256"]) == digest, "%s: the stored outputs belong to other inputs (regenerate with tests/golden/gen_legacy_kats.py)" % key
    return stored[key + "_dots"], [str(s) for s in stored[key + "_q8_sha256"]], stored[key + "_dequant"]


@pytest.mark.parametrize("t", TYPES)
def test_restatement_reproduces_the_reference(stored, t):
    for key, blocks, xs, digest, deq_rows in all_cases(t):
        dots, q8sha, deq = stored_case(stored, key, digest)
        assert np.isfinite(dots).all() and np.isfinite(deq).all(), key
        K = xs[0].size
        rb = K // 32 * lg.BB[t]
        for i, x in enumerate(xs):
            q8 = lg.quantize_row_q8_0(x)
            assert hashlib.sha256(np.ascontiguousarray(q8).tobytes()).hexdigest() == q8sha[i], "%s vector %d: Q8_0 bytes differ from the reference's" % (key, i)
            got = lg.vec_dot_rows(t, blocks, q8)
            bad = np.flatnonzero(bits(got) != bits(dots[i]))
            assert bad.size == 0, "%s vector %d: %d rows differ, first %d: %r vs %r" % (key, i, bad.size, bad[0], got[bad[0]], dots[i][bad[0]])
        for i, r in enumerate(deq_rows):
            got = lg.dequantize(t, blocks[r * rb:(r + 1) * rb])
            assert np.array_equal(bits(got), bits(deq[i])), "%s: dequantised row %d differs" % (key, r)


@pytest.mark.parametrize("t", lg.SGEMM_TYPES)
def test_the_two_reference_entry_points_agree(stored, t):
    """what ggml_compute_forward_mul_mat calls for Q8_0 / Q4_0 weights (llamafile_sgemm, one column and five) holds the bits of ggml_vec_dot_q*_0_q8_0"""
    for key, blocks, xs, digest, _ in all_cases(t):
        dots, _, _ = stored_case(stored, key, digest)
        assert np.array_equal(bits(stored[key + "_sgemm1"]), bits(dots)), key
        assert np.array_equal(bits(stored[key + "_sgemm5"]), bits(dots[lg.SGEMM_COLS(len(xs))])), key


@pytest.mark.parametrize("t", TYPES)
def test_edge_case_reaches_its_edges(t):
    """every weight kind and every activation kind occurs; the quants reach both ends (a Q8_0 byte of -128 included); d is negative, zero and subnormal
    somewhere; the activation blocks include all-zero ones, negative extrema, exact ties and blocks whose f16 d is subnormal or zero under non-zero quants"""
    blocks, xs, digest, wtags, xtags = lg.edge_case(t)
    assert set(wtags.reshape(-1)) == set(lg.EDGE_WKINDS[t]) and set(xtags.reshape(-1)) == set(lg.EDGE_AKINDS)
    d, q = lg.unpack(t, blocks)
    lo, hi = {lg.Q8_0: (-128, 127), lg.Q4_0: (-8, 7), lg.Q5_0: (-16, 15)}[t]
    assert (q == lo).all(axis=1).any() and (q == hi).all(axis=1).any()
    d16 = np.ascontiguousarray(blocks.reshape(-1, lg.BB[t])[:, 0:2]).view(np.uint16).reshape(-1)
    assert ((d16 & 0x7c00) == 0).any() and ((d16 & 0x7fff) == 0).any() and (d16 & 0x8000).any()
    if t == lg.Q5_0:
        qh = np.ascontiguousarray(blocks.reshape(-1, 22)[:, 2:6]).view(np.uint32).reshape(-1)
        assert (qh == 0).any() and (qh == 0xffffffff).any()
    seen = dict(zero=False, neg=False, tie=False, tiny=False)
    for x in xs:
        yd, qa = lg.q8_0_fields(lg.quantize_row_q8_0(x))
        xb = x.reshape(-1, 32)
        amax = np.abs(xb).max(axis=1)
        seen["zero"] |= bool(((amax == 0) & (yd == 0) & (qa == 0).all(axis=1)).any())
        seen["neg"] |= bool((xb.min(axis=1) == -amax)[amax > 0].any())
        sc = xb * np.where(amax != 0, np.float32(127.0) / np.where(amax != 0, amax, 1), 0).astype(np.float32)[:, None]
        seen["tie"] |= bool((np.abs(sc - np.trunc(sc)) == 0.5).any())
        seen["tiny"] |= bool(((yd < 6.2e-5) & (np.abs(qa).max(axis=1) == 127)).any())
    assert all(seen.values()), seen


# ---- the Python GGUF side ------------------------------------------------------------------------------------------------------------------------
def test_type_table_and_tensor_sizes():
    from booster_amd import gguf
    assert (gguf.Q4_0, gguf.Q5_0, gguf.Q8_0) == (2, 6, 8)
    assert [gguf.TYPE_NAMES[t] for t in (2, 6, 8)] == ["Q4_0", "Q5_0", "Q8_0"]
    for t, bb in ((gguf.Q4_0, 18), (gguf.Q5_0, 22), (gguf.Q8_0, 34)):
        assert gguf.GGML_TYPES[t] == (32, bb)
        assert gguf.tensor_nbytes(t, [4096, 13]) == 13 * 128 * bb
        assert gguf.tensor_nbytes(t, [288, 3]) == 3 * 9 * bb                     # a row of K % 32 == 0 is a valid GGUF tensor (the loader asks for K % 256 == 0)
        w = gguf.random_q0_tensor(t, 512, 5, np.random.default_rng(1))
        assert w.dtype == np.uint8 and w.size == gguf.tensor_nbytes(t, [512, 5])
        d = np.ascontiguousarray(w.reshape(-1, bb)[:, 0:2]).view(np.float16).astype(np.float32)
        assert np.isfinite(d).all() and (d > 0).all()
        big = gguf.random_q0_tensor(t, 4096, 64, np.random.default_rng(2)).reshape(-1, bb)
        assert len(np.unique(big[:, 2:])) == 256                                  # every byte pattern in qs / qh, 0x80 included


def test_recipes():
    """llama_tensor_get_type without an importance matrix: Q8_0 everywhere for Q8_0; Q4_0 / Q5_0 everywhere but output.weight, which is Q6_K"""
    from booster_amd import gguf
    names = ("token_embd", "output", "attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down")
    for il in (0, 1, 15, 31):
        for n in names:
            assert gguf.q8_0_type(n, il, 32) == gguf.Q8_0
            assert gguf.q4_0_type(n, il, 32) == (gguf.Q6_K if n == "output" else gguf.Q4_0)
            assert gguf.q5_0_type(n, il, 32) == (gguf.Q6_K if n == "output" else gguf.Q5_0)


@pytest.mark.parametrize("recipe", ["q8_0", "q4_0", "q5_0"])
def test_tiny_legacy_file_round_trips(tmp_path, recipe):
    from booster_amd import gguf
    E, H, Hkv, Lyr, F, V = 256, 4, 1, 2, 512, 64
    rf = {"q8_0": gguf.q8_0_type, "q4_0": gguf.q4_0_type, "q5_0": gguf.q5_0_type}[recipe]
    embd = rf("token_embd", 0, Lyr)
    path = str(tmp_path / (recipe + ".gguf"))
    gguf.write_synthetic_llama(path, E, H, Hkv, Lyr, F, V, type_fn=lambda n, il: rf(n, il, Lyr), embd_type=embd, seed=11)
    r = gguf.GGUFReader(path)
    for name in ("token_embd.weight", "blk.0.attn_q.weight", "blk.0.attn_v.weight", "blk.1.attn_output.weight", "blk.1.ffn_up.weight", "blk.1.ffn_down.weight"):
        ti = r.tensors[name]
        assert ti["type"] == embd, (name, ti["type"])
        assert ti["data"].size == int(np.prod(ti["shape"])) // 32 * gguf.GGML_TYPES[embd][1]
    assert r.tensors["output.weight"]["type"] == (gguf.Q8_0 if recipe == "q8_0" else gguf.Q6_K)
    path2 = str(tmp_path / (recipe + "_2.gguf"))
    gguf.write_synthetic_llama(path2, E, H, Hkv, Lyr, F, V, type_fn=lambda n, il: rf(n, il, Lyr), embd_type=embd, seed=11)
    assert open(path, "rb").read() == open(path2, "rb").read()
