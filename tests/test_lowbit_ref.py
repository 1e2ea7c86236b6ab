"""CPU: Q3_K / Q2_K.  The numpy restatement of the two eight-lane chains (tests/lowbit_ref.py) must reproduce, bit for bit, every stored output of
the genuine reference (tests/golden/lowbit_kats.npz, written by tests/golden/gen_lowbit_kats.py); where oracle/_ref/libggml_ref.so is built, the live
library must reproduce the stored outputs too.  Also: the synthetic-file generator draws the same bytes as before for the existing types, and tiny
Q3_K_M / Q2_K files round-trip through the reader and the loader's GGUF probe."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import lowbit_ref as lr
from conftest import GOLDEN
from lowbit_ref import DEQ_ROWS, all_cases, load_ref, reference_outputs  # noqa: F401

KATS = os.path.join(GOLDEN, "lowbit_kats.npz")
TYPES = [lr.Q2_K, lr.Q3_K]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def ref():
    return load_ref()


@pytest.fixture(scope="module")
def stored():
    return np.load(KATS)


def stored_case(stored, key, digest):
    assert str(stored[key + "_inputs_sha256"]) == digest, "%s: the stored outputs belong to other inputs (regenerate with tests/golden/gen_lowbit_kats.py)" % key
    return stored[key + "_dots"], [str(s) for s in stored[key + "_q8_sha256"]], stored[key + "_dequant"]


@pytest.mark.parametrize("t", TYPES)
def test_restatement_reproduces_the_reference(po, stored, t):
    for key, blocks, xs, digest, deq_rows in all_cases(t):
        dots, q8sha, deq = stored_case(stored, key, digest)
        assert np.isfinite(dots).all() and np.isfinite(deq).all(), key
        K = xs[0].size
        rb = K // 256 * lr.BB[t]
        for i, x in enumerate(xs):
            q8 = po.quantize_q8_K(x)
            assert hashlib.sha256(np.ascontiguousarray(q8).tobytes()).hexdigest() == q8sha[i], "%s vector %d: Q8_K bytes differ from the reference's" % (key, i)
            got = lr.vec_dot_rows(t, blocks, q8)
            bad = np.flatnonzero(bits(got) != bits(dots[i]))
            assert bad.size == 0, "%s vector %d: %d rows differ, first %d: %r vs %r" % (key, i, bad.size, bad[0], got[bad[0]], dots[i][bad[0]])
        for i, r in enumerate(deq_rows):
            got = lr.dequantize(t, blocks[r * rb:(r + 1) * rb])
            assert np.array_equal(bits(got), bits(deq[i])), "%s: dequantised row %d differs" % (key, r)


@pytest.mark.parametrize("t", TYPES)
def test_edge_case_reaches_its_edges(stored, t):
    """every weight kind and every activation kind occurs, and the integer sums come near their bounds"""
    blocks, xs, digest, wtags, xtags = lr.edge_case(t)
    assert set(wtags.reshape(-1)) == set(lr.EDGE_WKINDS[t]) and set(xtags.reshape(-1)) == set(lr.EDGE_AKINDS)
    f = lr.unpack(t, blocks)
    lo, hi = (-32, 31) if t == lr.Q3_K else (0, 15)
    assert f["scale"].min() == lo and f["scale"].max() == hi
    qlo, qhi = (-4, 3) if t == lr.Q3_K else (0, 3)
    assert (f["q"] == qlo).all(axis=1).any() and (f["q"] == qhi).all(axis=1).any()
    d16 = np.ascontiguousarray(blocks.reshape(-1, lr.BB[t])[:, lr.D_OFF[t]:lr.D_OFF[t] + 2]).view(np.uint16).reshape(-1)
    assert ((d16 & 0x7c00) == 0).any() and ((d16 & 0x7fff) == 0).any() and (d16 & 0x8000).any()


@pytest.mark.parametrize("t", TYPES)
def test_live_reference_reproduces_the_stored_outputs(ref, stored, t):
    if ref is None:
        pytest.skip("oracle/_ref/libggml_ref.so is not built here: the stored outputs stand in for it")
    for key, blocks, xs, digest, deq_rows in all_cases(t):
        dots, q8sha, deq = stored_case(stored, key, digest)
        ldots, lsha, ldeq = reference_outputs(ref, t, blocks, xs, deq_rows)
        assert np.array_equal(bits(ldots), bits(dots)) and lsha == q8sha and np.array_equal(bits(ldeq), bits(deq)), key


def test_fma32_is_correctly_rounded():
    """against exact rational arithmetic, on operands built to hit the double-rounding cases of a float64 add"""
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a = rng.standard_normal(4000).astype(np.float32); b = rng.standard_normal(4000).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.integers(-3, 4, 4000) * 2.0 ** -24)).astype(np.float32)    # massive cancellation
    c[::3] = (rng.standard_normal(1334) * 10.0 ** rng.uniform(-12, 12, 1334)).astype(np.float32)
    # exact ties of the float64 sum: p + c with c = 2^-30 p-sized odd multiples
    a[::5] = np.float32(1 + 2.0 ** -23); b[::5] = np.float32(1 + 2.0 ** -23); c[::5] = (2.0 ** rng.integers(20, 60, 800)).astype(np.float32)
    got = lr.fma32(a, b, c)
    def rn32(fr):                                              # correctly rounded Fraction -> float32 (normal range; the operands stay inside it)
        if fr == 0:
            return np.float32(0.0)
        s, m = (-1 if fr < 0 else 1), abs(fr)
        e = m.numerator.bit_length() - m.denominator.bit_length()
        if Fraction(2) ** e > m:
            e -= 1
        q = m / Fraction(2) ** (e - 23)                         # in [2^23, 2^24)
        n = q.numerator // q.denominator
        rem = q - n
        if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (n & 1)):
            n += 1
        return np.float32(s * float(n) * 2.0 ** (e - 23))
    for i in range(a.size):
        want = rn32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
        if abs(float(want)) < 1e-30:
            continue
        assert bits(got[i:i + 1])[0] == bits(np.array([want], np.float32))[0], (i, a[i], b[i], c[i], got[i], want)


# ---- the synthetic-file generator --------------------------------------------------------------------------------------------------------------
def test_existing_synthetic_files_do_not_move(tmp_path):
    """adding the two types to the generator must not move one byte of an existing file: `shift` regenerated has the size and digest of its committed side file"""
    import sys
    sys.path.insert(0, GOLDEN)
    import gen_fullsize_fixtures as g
    from booster_amd import gguf
    line = open(os.path.join(GOLDEN, "fullsize_shift.bgld.txt")).read().splitlines()[-1]
    side = dict(tok.split("=", 1) for tok in line.split() if "=" in tok)
    kw = dict(g.CONFIGS["shift"][0])
    tf = kw.pop("type_fn", None)
    path = str(tmp_path / "shift.gguf")
    gguf.write_synthetic_llama(path, seed=7, reuse_layers=True, type_fn=g.type_fn_of(tf, kw["L"]), **kw)
    dg, sz = g.file_digest(path)
    assert sz == int(side["gguf_bytes"]) and dg == side["gguf_sha256_first64MiB"]


@pytest.mark.parametrize("recipe", ["q3_k_m", "q2_k"])
def test_tiny_lowbit_file_round_trips(tmp_path, recipe):
    from booster_amd import gguf
    E, H, Hkv, Lyr, F, V = 256, 4, 1, 2, 512, 64
    fn = (lambda n, il: gguf.q3_k_m_type(n, il, Lyr)) if recipe == "q3_k_m" else (lambda n, il: gguf.q2_k_type(n, il, Lyr, n_gqa=H // Hkv))
    embd = gguf.Q3_K if recipe == "q3_k_m" else gguf.Q2_K
    path = str(tmp_path / (recipe + ".gguf"))
    gguf.write_synthetic_llama(path, E, H, Hkv, Lyr, F, V, type_fn=fn, embd_type=embd, seed=11)
    r = gguf.GGUFReader(path)
    want = {"token_embd.weight": embd, "output.weight": gguf.Q6_K, "blk.0.attn_q.weight": embd, "blk.1.ffn_up.weight": embd,
            "blk.0.attn_v.weight": gguf.Q5_K if recipe == "q3_k_m" else gguf.Q4_K, "blk.1.attn_output.weight": gguf.Q4_K if recipe == "q3_k_m" else gguf.Q3_K,
            "blk.1.ffn_down.weight": gguf.Q4_K if recipe == "q3_k_m" else gguf.Q3_K}
    for name, t in want.items():
        ti = r.tensors[name]
        assert ti["type"] == t, (name, ti["type"], t)
        assert ti["data"].size == int(np.prod(ti["shape"])) // 256 * gguf.GGML_TYPES[t][1]
    # d / dmin of the new types are finite, non-zero f16
    for name, t in want.items():
        if t in (gguf.Q2_K, gguf.Q3_K):
            blk = np.asarray(r.tensors[name]["data"]).reshape(-1, gguf.GGML_TYPES[t][1])
            d = np.ascontiguousarray(blk[:, lr.D_OFF[t]:]).view(np.float16).astype(np.float32)
            assert np.isfinite(d).all() and (d > 0).all()
    # the same seed draws the same bytes
    path2 = str(tmp_path / (recipe + "_2.gguf"))
    gguf.write_synthetic_llama(path2, E, H, Hkv, Lyr, F, V, type_fn=fn, embd_type=embd, seed=11)
    assert open(path, "rb").read() == open(path2, "rb").read()
    # the loader's own GGUF parser (no device needed) accepts the file and digests every tensor: same count and bytes as the Python reader sees
    import booster_amd
    L = booster_amd.lib()
    L.bamd_gguf_probe.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p]
    n, b, d = C.c_int64(0), C.c_int64(0), C.c_uint64(0)
    assert L.bamd_gguf_probe(path.encode(), C.byref(n), C.byref(b), C.byref(d)) == 0, booster_amd.lib().bamd_last_error()
    assert n.value == len(r.tensors) and b.value == sum(int(ti["data"].size) for ti in r.tensors.values())
