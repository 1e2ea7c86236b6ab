"""CPU: IQ4_XS.  The numpy restatement of the eight-lane chain with the -128 rule and of the two-rounding dequantiser (tests/iq4xs_ref.py) must reproduce, bit
for bit, every stored output of the genuine reference (tests/golden/iq4xs_kats.npz, written by tests/golden/gen_iq4xs_kats.py); the stored outputs must tell
the reference from the three ways this type is easy to get wrong.  Also: the Python GGUF side knows the type's size and llama.cpp's recipe, a tiny file of the
recipe round-trips through the writer and the reader, and the load-time message says in words why such a model runs its prompts on the integer-dot kernel."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import iq4xs_ref as xr
from conftest import GOLDEN

KATS = os.path.join(GOLDEN, "iq4xs_kats.npz")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def stored():
    return np.load(KATS)


def stored_case(stored, key, digest):
    assert str(stored[key + "_inputs_sha256"]) == digest, "%s: the stored outputs belong to other inputs (regenerate with tests/golden/gen_iq4xs_kats.py)" % key
    return stored[key + "_dots"], [str(s) for s in stored[key + "_q8_sha256"]], stored[key + "_dequant"]


def test_table_and_shapes():
    assert xr.KVALUES.tolist() == [-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113]
    assert xr.KS == [256, 768, 4096, 14336] and xr.ROWS == 32 and len(xr.SCALES) == 3


def test_restatement_reproduces_the_reference(po, stored):
    keys = []
    for key, blocks, xs, digest, deq_rows in xr.all_cases():
        keys.append(key)
        dots, q8sha, deq = stored_case(stored, key, digest)
        assert dots.shape == (len(xs), xr.ROWS) and deq.shape == (len(deq_rows), xs[0].size), key
        assert np.isfinite(dots).all() and np.isfinite(deq).all(), key
        K = xs[0].size
        rb = K // 256 * xr.BB
        for i, x in enumerate(xs):
            q8 = po.quantize_q8_K(x)
            assert hashlib.sha256(np.ascontiguousarray(q8).tobytes()).hexdigest() == q8sha[i], "%s vector %d: Q8_K bytes differ from the reference's" % (key, i)
            got = xr.vec_dot_rows(blocks, q8)
            bad = np.flatnonzero(bits(got) != bits(dots[i]))
            assert bad.size == 0, "%s vector %d: %d rows differ, first %d: %r vs %r" % (key, i, bad.size, bad[0], got[bad[0]], dots[i][bad[0]])
            assert not (xr.ei.q8_fields(q8)[1] == -128).any(), "%s vector %d: a quantised byte of -128 (the -128 rule would act in the kernels)" % (key, i)
            assert np.array_equal(bits(xr.vec_dot_rows(blocks, q8, rule=False)), bits(got)), "%s vector %d: the rule acts on a quantised vector" % (key, i)
        for i, r in enumerate(deq_rows):
            got = xr.dequantize(blocks[r * rb:(r + 1) * rb])
            assert np.array_equal(bits(got), bits(deq[i])), "%s: dequantised row %d differs" % (key, r)
        if key in xr.M128_KEYS:                                  # hand-made Q8_K vectors that hold -128: the rule, held to the reference
            m128 = stored[key + "_dots_m128"]
            hand = xr.m128_q8(key, [po.quantize_q8_K(x) for x in xs])
            assert m128.shape == (len(hand), xr.ROWS) and np.isfinite(m128).all(), key
            for i, q in enumerate(hand):
                assert (xr.ei.q8_fields(q)[1] == -128).any()
                assert np.array_equal(bits(xr.vec_dot_rows(blocks, q)), bits(m128[i])), "%s hand-made vector %d differs" % (key, i)
    assert keys == ["iq4_xs_K%d" % K for K in xr.KS] + ["iq4_xs_edge", "iq4_xs_pairs"]          # no case left out of the comparison


def test_stored_outputs_show_the_minus_128_rule(po, stored):
    """(a) at K = 4096 the plain signed dot differs from the reference in at least one of the 32 rows for every activation magnitude — where the rule can act:
    on the vectors of that magnitude with their -127 bytes (one per super-block at least: the largest element) rewritten to -128, as iscale = -128 / max
    would have stored them.  quantize_row_q8_K itself scales by -127 / max (ggml-quants.c:3613-3618) and never writes -128, so on the quantised vectors
    themselves the plain dot IS the reference's (asserted for every stored vector in test_restatement_reproduces_the_reference): 0 of 32 rows differ at
    every magnitude and no seed changes that.  Measured when the fixture was recorded: 32 of 32 rows differ on the rewritten vectors at each magnitude"""
    blocks, xs, digest = xr.rand_case(4096)
    stored_case(stored, "iq4_xs_K4096", digest)
    m128 = stored["iq4_xs_K4096_dots_m128"]
    for i, x in enumerate(xs):
        plain = xr.vec_dot_rows(blocks, xr.with_m128(po.quantize_q8_K(x)), rule=False)
        assert (bits(plain) != bits(m128[i])).any(), "magnitude %g does not discriminate" % xr.SCALES[i]


def test_stored_rows_show_the_two_roundings(stored):
    """(b) d * ((ls - 32) * value) with one rounding differs from the stored dequantised rows in at least one element"""
    blocks, xs, digest = xr.rand_case(4096)
    _, _, deq = stored_case(stored, "iq4_xs_K4096", digest)
    rb = 4096 // 256 * xr.BB
    n = sum(int((bits(xr.dequantize(blocks[r * rb:(r + 1) * rb], fused=True)) != bits(deq[j])).sum()) for j, r in enumerate(xr.DEQ_ROWS))
    assert n >= 1


def test_stored_outputs_tell_the_lane_mappings_apart(po, stored):
    """(c) at K = 4096 the Q4_K lane mapping (lane e <-> qs[32 j + 4 e ..]) differs from the reference in at least one of the 32 rows for every magnitude"""
    blocks, xs, digest = xr.rand_case(4096)
    dots, _, _ = stored_case(stored, "iq4_xs_K4096", digest)
    for i, x in enumerate(xs):
        other = xr.vec_dot_rows(blocks, po.quantize_q8_K(x), q4k_lanes=True)
        assert (bits(other) != bits(dots[i])).any(), "magnitude %g does not discriminate" % xr.SCALES[i]


def test_edge_case_reaches_its_edges(po):
    """every weight kind in every block position and every activation kind; scales -32, -1, 0 and 31; qs all 0x00 and all 0xFF; d the smallest subnormal, the
    largest finite f16, negative and zero; a zero activation block; an activation block that quantises to every byte a Q8_K block can hold, -127 .. 127"""
    blocks, xs, digest, wtags, xtags = xr.edge_case()
    assert set(xtags.reshape(-1)) == set(xr.EDGE_AKINDS)
    for c in range(wtags.shape[1]):
        assert set(wtags[:, c]) >= {"ls_0", "ls_31", "ls_32", "ls_63"}, "block position %d" % c
    assert set(wtags.reshape(-1)) == set(xr.EDGE_WKINDS)
    d, ls, nib, q = xr.unpack(blocks)
    for v in (-32, -1, 0, 31):
        assert (ls == v).all(axis=1).any(), v
    assert (nib == 0).all(axis=1).any() and (nib == 15).all(axis=1).any()
    d16 = np.ascontiguousarray(blocks.reshape(-1, xr.BB)[:, 0:2]).view(np.uint16).reshape(-1)
    assert ((d16 & 0x7fff) == 0x0001).any() and ((d16 & 0x7fff) == 0x7bff).any() and (d16 & 0x8000).any() and ((d16 & 0x7fff) == 0).any()
    seen_all = seen_zero = False
    for x in xs:
        yd, qa, _ = xr.ei.q8_fields(po.quantize_q8_K(x))
        for b in range(yd.size):
            seen_zero |= yd[b] == 0.0
            seen_all |= sorted(set(qa[b].tolist())) == list(range(-127, 128))
    assert seen_all and seen_zero


def test_pairs_case_meets_every_nibble_with_every_byte(po):
    """all 16 x 255 (nibble, byte) pairs on quantised vectors (integers -127 .. 127 with 127 present quantise to themselves or their negatives), all 16 x 256 on
    the hand-made blocks"""
    blocks, xs, _, q8s = xr.pairs_case()
    _, _, nib, _ = xr.unpack(blocks)
    for vecs, lo in (([po.quantize_q8_K(x) for x in xs], -127), (q8s, -128)):
        seen = np.zeros((16, 256), bool)
        for q8 in vecs:
            yd, qa, _ = xr.ei.q8_fields(q8)
            assert yd.size == 1 and abs(float(yd[0])) == 1.0
            for r in range(xr.ROWS):
                seen[nib[r], qa[0].astype(np.int32) + 128] = True
        assert seen[:, lo + 128:].all() and not seen[:, :lo + 128].any()
    for x in xs:
        qa = xr.ei.q8_fields(po.quantize_q8_K(x))[1][0].astype(np.float32)
        assert np.array_equal(qa, x) or np.array_equal(qa, -x)


def test_live_reference_reproduces_the_stored_outputs(stored):
    L = xr.load_ref()
    if L is None:
        pytest.skip("oracle/_ref/libggml_ref.so is not built here: the stored outputs stand in for it")
    for key, blocks, xs, digest, deq_rows in xr.all_cases():
        dots, q8sha, deq = stored_case(stored, key, digest)
        q8s = []
        d2, s2, q2 = xr.reference_outputs(L, blocks, xs, deq_rows, q8s)
        assert np.array_equal(bits(d2), bits(dots)) and s2 == q8sha and np.array_equal(bits(q2), bits(deq)), key
        if key in xr.M128_KEYS:
            K = xs[0].size
            assert np.array_equal(bits(np.stack([xr.reference_dots(L, blocks, K, q) for q in xr.m128_q8(key, q8s)])), bits(stored[key + "_dots_m128"])), key


# ---- the Python GGUF side ------------------------------------------------------------------------------------------------------------------------
def test_type_table_and_tensor_sizes():
    import booster_amd
    from booster_amd import gguf
    assert gguf.IQ4_XS == 23 == booster_amd.IQ4_XS and gguf.TYPE_NAMES[23] == "IQ4_XS" and gguf.FTYPE_MOSTLY_IQ4_XS == 30
    assert gguf.GGML_TYPES[23] == (256, 136)
    assert gguf.tensor_nbytes(23, [4096, 13]) == 13 * 16 * 136
    w = gguf.random_kquant_tensor(23, 512, 5, np.random.default_rng(1))
    assert w.dtype == np.uint8 and w.size == gguf.tensor_nbytes(23, [512, 5])
    d = np.ascontiguousarray(w.reshape(-1, 136)[:, 0:2]).view(np.float16).astype(np.float32)
    assert np.isfinite(d).all() and (d > 0).all()
    big = gguf.random_iq4_xs_tensor(4096, 64, np.random.default_rng(2))
    assert len(np.unique(big.reshape(-1, 136)[:, 8:])) == 256                    # every nibble pair
    _, ls, _, _ = xr.unpack(big)
    assert set(np.unique(ls).tolist()) == set(range(-32, 32))                   # every 6-bit scale, 0 and 63 included
    sh = np.ascontiguousarray(big.reshape(-1, 136)[:, 2:4]).view(np.uint16)
    assert int(np.bitwise_or.reduce(sh.reshape(-1))) == 0xffff and int(np.bitwise_and.reduce(sh.reshape(-1))) == 0      # every bit of scales_h set somewhere, and clear somewhere


NAMES = ("token_embd", "output", "attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down")


@pytest.mark.parametrize("n_gqa", [1, 4, 8])
@pytest.mark.parametrize("n_layer", [3, 8, 32])
@pytest.mark.parametrize("imatrix", [False, True])
def test_recipe(n_gqa, n_layer, imatrix):
    """llama_tensor_get_type under LLAMA_FTYPE_MOSTLY_IQ4_XS, the rules one by one: output.weight Q6_K; attn_v Q5_K where n_gqa >= 4 (llama.cpp:15544-15546);
    ffn_down Q5_K in the layers il < n_layer / 8 of a file made without an importance matrix (:15611-15613); everything else the ftype's default type,
    IQ4_XS (:15807-15808)"""
    from booster_amd import gguf
    for il in range(n_layer):
        for n in NAMES:
            got = gguf.iq4_xs_type(n, il, n_layer, n_gqa=n_gqa, imatrix=imatrix)
            if n == "output":
                want = gguf.Q6_K
            elif n == "attn_v" and n_gqa >= 4:
                want = gguf.Q5_K
            elif n == "ffn_down" and not imatrix and il < n_layer // 8:
                want = gguf.Q5_K
            else:
                want = gguf.IQ4_XS
            assert got == want, (n, il)
    q5_down = [il for il in range(n_layer) if gguf.iq4_xs_type("ffn_down", il, n_layer, n_gqa=n_gqa, imatrix=imatrix) == gguf.Q5_K]
    assert q5_down == ([] if imatrix else list(range(n_layer // 8)))             # none at 3 layers, layer 0 at 8, layers 0-3 at 32
    assert gguf.iq4_xs_type("attn_v", 0, n_layer) == gguf.Q5_K                   # the default n_gqa is the headline shape's


@pytest.mark.parametrize("tied", [False, True])
@pytest.mark.parametrize("Hkv", [1, 4])
def test_tiny_file_round_trips(tmp_path, tied, Hkv):
    """a file of the recipe: types per tensor, file type 30 in the metadata, a tied embedding written as the Q6_K output matrix; the writer is deterministic"""
    import importlib.util
    from booster_amd import gguf
    spec = importlib.util.spec_from_file_location("gen_iq4xs_fixtures", os.path.join(GOLDEN, "gen_iq4xs_fixtures.py"))
    gen = importlib.util.module_from_spec(spec); spec.loader.exec_module(gen)
    kw = dict(E=256, H=4, Hkv=Hkv, L=8, F=512, V=64)
    fn, embd = gen.type_fn_of(kw, dict(imatrix=False), tied)
    assert embd == (gguf.Q6_K if tied else gguf.IQ4_XS)
    path = str(tmp_path / "iq4xs.gguf")
    gguf.write_synthetic_llama(path, type_fn=fn, embd_type=embd, tied=tied, seed=11, file_type=gguf.FTYPE_MOSTLY_IQ4_XS, **kw)
    r = gguf.GGUFReader(path)
    assert r.kv["general.file_type"] == 30
    v = gguf.Q5_K if 4 // Hkv >= 4 else gguf.IQ4_XS
    want = {"token_embd.weight": embd, "blk.0.attn_q.weight": gguf.IQ4_XS, "blk.0.attn_k.weight": gguf.IQ4_XS, "blk.0.attn_v.weight": v, "blk.7.attn_v.weight": v,
            "blk.3.attn_output.weight": gguf.IQ4_XS, "blk.1.ffn_up.weight": gguf.IQ4_XS, "blk.0.ffn_down.weight": gguf.Q5_K, "blk.1.ffn_down.weight": gguf.IQ4_XS}
    for name, t in want.items():
        ti = r.tensors[name]
        assert ti["type"] == t, (name, ti["type"])
        assert ti["data"].size == gguf.tensor_nbytes(t, ti["shape"])
    assert ("output.weight" in r.tensors) == (not tied)
    path2 = str(tmp_path / "iq4xs_2.gguf")
    gguf.write_synthetic_llama(path2, type_fn=fn, embd_type=embd, tied=tied, seed=11, file_type=gguf.FTYPE_MOSTLY_IQ4_XS, **kw)
    assert open(path, "rb").read() == open(path2, "rb").read()


# ---- the load-time message -----------------------------------------------------------------------------------------------------------------------
SWITCHES = ("lowbit", "q0", "q1", "nl", "flt")
SENTENCE = ("the model holds an IQ4_XS matrix: these have no matrix-core kernel, and side tables are all-or-nothing per model, so every prompt mat-mul runs on the "
            "integer-dot kernel (token by token where K > 35840)")


def test_prefill_reason_under_all_32_switch_settings():
    """IQ4_XS belongs to no matrix-core family: whatever the switches say, never "tables", always the literal sentence"""
    import booster_amd
    f = booster_amd.lib().bamd_prefill_reason_test
    f.argtypes = [C.c_int]; f.restype = C.c_char_p
    try:
        for setting in range(32):
            for i, s in enumerate(SWITCHES):
                getattr(booster_amd, "set_prefill_" + s)(bool(setting >> i & 1))
            assert f(23).decode() == SENTENCE, setting
    finally:
        for s in SWITCHES:
            getattr(booster_amd, "set_prefill_" + s)(os.environ.get("BAMD_PREFILL_" + s.upper(), "")[:1] == "1")
