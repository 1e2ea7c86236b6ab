"""CPU: IQ4_NL.  The numpy restatement of the two-accumulator chain and of the dequantiser (tests/iq4nl_ref.py) must reproduce, bit for bit, every stored output
of the genuine reference (tests/golden/iq4nl_kats.npz, written by tests/golden/gen_iq4nl_kats.py); the stored outputs must tell that chain from the
one-accumulator order of Q4_0.  Also: the Python GGUF side knows the type's size and llama.cpp's recipe, and a tiny file of the recipe round-trips through the
writer and the reader."""
import hashlib
import os

import numpy as np
import pytest

import iq4nl_ref as nl
import legacy_ref as lg
from conftest import GOLDEN

KATS = os.path.join(GOLDEN, "iq4nl_kats.npz")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def stored():
    return np.load(KATS)


def stored_case(stored, key, digest):
    assert str(stored[key + "_inputs_sha256"]) == digest, "%s: the stored outputs belong to other inputs (regenerate with tests/golden/gen_iq4nl_kats.py)" % key
    return stored[key + "_dots"], [str(s) for s in stored[key + "_q8_sha256"]], stored[key + "_dequant"]


def test_table():
    """kvalues_iq4nl (ggml-quants.c:3548): sixteen increasing int8 from -127 to 113"""
    assert nl.KVALUES.tolist() == [-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113]


def test_restatement_reproduces_the_reference(stored):
    for key, blocks, xs, digest, deq_rows in nl.all_cases():
        dots, q8sha, deq = stored_case(stored, key, digest)
        assert np.isfinite(dots).all() and np.isfinite(deq).all(), key
        K = xs[0].size
        rb = K // 32 * nl.BB
        for i, x in enumerate(xs):
            q8 = lg.quantize_row_q8_0(x)
            assert hashlib.sha256(np.ascontiguousarray(q8).tobytes()).hexdigest() == q8sha[i], "%s vector %d: Q8_0 bytes differ from the reference's" % (key, i)
            got = nl.vec_dot_rows(blocks, q8)
            bad = np.flatnonzero(bits(got) != bits(dots[i]))
            assert bad.size == 0, "%s vector %d: %d rows differ, first %d: %r vs %r" % (key, i, bad.size, bad[0], got[bad[0]], dots[i][bad[0]])
        for i, r in enumerate(deq_rows):
            got = nl.dequantize(blocks[r * rb:(r + 1) * rb])
            assert np.array_equal(bits(got), bits(deq[i])), "%s: dequantised row %d differs" % (key, r)


def test_stored_outputs_tell_the_two_chain_shapes_apart(stored):
    """at K = 4096 the ONE-accumulator order (the Q4_0 chain on the same terms) differs from the reference in at least one of the 32 rows for every activation
    magnitude: a kernel that ran the Q4_0 chain over table values would fail the known-answer tests"""
    blocks, xs, digest = nl.rand_case(4096)
    dots, _, _ = stored_case(stored, "iq4_nl_K4096", digest)
    for i, x in enumerate(xs):
        one = nl.vec_dot_rows(blocks, lg.quantize_row_q8_0(x), one_accumulator=True)
        assert (bits(one) != bits(dots[i])).any(), "magnitude %g does not discriminate" % nl.SCALES[i]


def test_edge_case_reaches_its_edges():
    """every weight kind and every activation kind occurs; blocks of all nibbles 0 (-127) and all nibbles 15 (113); d negative, zero and subnormal somewhere"""
    blocks, xs, digest, wtags, xtags = nl.edge_case()
    assert set(wtags.reshape(-1)) == set(nl.EDGE_WKINDS) and set(xtags.reshape(-1)) == set(nl.EDGE_AKINDS)
    assert {"quants_min", "quants_max"} <= set(nl.EDGE_WKINDS)
    d, nib, q = nl.unpack(blocks)
    assert (nib == 0).all(axis=1).any() and (nib == 15).all(axis=1).any()
    assert (q == -127).all(axis=1).any() and (q == 113).all(axis=1).any()
    d16 = np.ascontiguousarray(blocks.reshape(-1, nl.BB)[:, 0:2]).view(np.uint16).reshape(-1)
    assert ((d16 & 0x7c00) == 0).any() and ((d16 & 0x7fff) == 0).any() and (d16 & 0x8000).any()


# ---- the Python GGUF side ------------------------------------------------------------------------------------------------------------------------
def test_type_table_and_tensor_sizes():
    import booster_amd
    from booster_amd import gguf
    assert gguf.IQ4_NL == 20 == booster_amd.IQ4_NL and gguf.TYPE_NAMES[20] == "IQ4_NL" and gguf.FTYPE_MOSTLY_IQ4_NL == 25
    assert gguf.GGML_TYPES[20] == (32, 18)
    assert gguf.tensor_nbytes(20, [4096, 13]) == 13 * 128 * 18
    assert gguf.tensor_nbytes(20, [288, 3]) == 3 * 9 * 18                        # a row of K % 32 == 0 is a valid GGUF tensor (the loader asks for K % 256 == 0)
    w = gguf.random_kquant_tensor(20, 512, 5, np.random.default_rng(1))
    assert w.dtype == np.uint8 and w.size == gguf.tensor_nbytes(20, [512, 5])
    d = np.ascontiguousarray(w.reshape(-1, 18)[:, 0:2]).view(np.float16).astype(np.float32)
    assert np.isfinite(d).all() and (d > 0).all()
    big = gguf.random_iq4_nl_tensor(4096, 64, np.random.default_rng(2)).reshape(-1, 18)
    assert len(np.unique(big[:, 2:])) == 256                                     # every nibble pair


NAMES = ("token_embd", "output", "attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down")


@pytest.mark.parametrize("n_gqa", [1, 4])
@pytest.mark.parametrize("n_layer", [3, 8, 32])
@pytest.mark.parametrize("imatrix", [False, True])
def test_recipe(n_gqa, n_layer, imatrix):
    """llama_tensor_get_type under LLAMA_FTYPE_MOSTLY_IQ4_NL, the rules one by one: output.weight Q6_K; attn_v Q5_K where n_gqa >= 4 (llama.cpp:15544-15546);
    ffn_down Q5_K in the layers il < n_layer / 8 of a file made without an importance matrix (:15611-15613); everything else IQ4_NL"""
    from booster_amd import gguf
    for il in range(n_layer):
        for n in NAMES:
            got = gguf.iq4_nl_type(n, il, n_layer, n_gqa=n_gqa, imatrix=imatrix)
            if n == "output":
                want = gguf.Q6_K
            elif n == "attn_v" and n_gqa >= 4:
                want = gguf.Q5_K
            elif n == "ffn_down" and not imatrix and il < n_layer // 8:
                want = gguf.Q5_K
            else:
                want = gguf.IQ4_NL
            assert got == want, (n, il)
    q5_down = [il for il in range(n_layer) if gguf.iq4_nl_type("ffn_down", il, n_layer, n_gqa=n_gqa, imatrix=imatrix) == gguf.Q5_K]
    assert q5_down == ([] if imatrix else list(range(n_layer // 8)))             # none at 3 layers, layer 0 at 8, layers 0-3 at 32
    assert gguf.iq4_nl_type("attn_v", 0, n_layer) == gguf.Q5_K                   # the default n_gqa is the headline shape's


@pytest.mark.parametrize("tied", [False, True])
@pytest.mark.parametrize("Hkv", [1, 4])
def test_tiny_file_round_trips(tmp_path, tied, Hkv):
    """a file of the recipe: types per tensor, file type 25 in the metadata, a tied embedding written as the Q6_K output matrix; the writer is deterministic"""
    import importlib.util
    from booster_amd import gguf
    spec = importlib.util.spec_from_file_location("gen_iq4nl_fixtures", os.path.join(GOLDEN, "gen_iq4nl_fixtures.py"))
    gen = importlib.util.module_from_spec(spec); spec.loader.exec_module(gen)
    kw = dict(E=256, H=4, Hkv=Hkv, L=8, F=512, V=64)
    fn, embd = gen.type_fn_of(kw, dict(imatrix=False), tied)
    assert embd == (gguf.Q6_K if tied else gguf.IQ4_NL)
    path = str(tmp_path / "iq4nl.gguf")
    gguf.write_synthetic_llama(path, type_fn=fn, embd_type=embd, tied=tied, seed=11, file_type=gguf.FTYPE_MOSTLY_IQ4_NL, **kw)
    r = gguf.GGUFReader(path)
    assert r.kv["general.file_type"] == 25
    v = gguf.Q5_K if 4 // Hkv >= 4 else gguf.IQ4_NL
    want = {"token_embd.weight": embd, "blk.0.attn_q.weight": gguf.IQ4_NL, "blk.0.attn_k.weight": gguf.IQ4_NL, "blk.0.attn_v.weight": v, "blk.7.attn_v.weight": v,
            "blk.3.attn_output.weight": gguf.IQ4_NL, "blk.1.ffn_up.weight": gguf.IQ4_NL, "blk.0.ffn_down.weight": gguf.Q5_K, "blk.1.ffn_down.weight": gguf.IQ4_NL}
    for name, t in want.items():
        ti = r.tensors[name]
        assert ti["type"] == t, (name, ti["type"])
        assert ti["data"].size == gguf.tensor_nbytes(t, ti["shape"])
    assert ("output.weight" in r.tensors) == (not tied)
    if not tied:
        assert r.tensors["output.weight"]["type"] == gguf.Q6_K
    path2 = str(tmp_path / "iq4nl_2.gguf")
    gguf.write_synthetic_llama(path2, type_fn=fn, embd_type=embd, tied=tied, seed=11, file_type=gguf.FTYPE_MOSTLY_IQ4_NL, **kw)
    assert open(path, "rb").read() == open(path2, "rb").read()
