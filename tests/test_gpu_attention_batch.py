"""GPU: the attention of a prefill micro-batch (T > 1 tokens) at op level, through bamd_op_attention_batch (include/bamd.h), against the oracle's
bo_attention (oracle/booster_oracle.c, the reference's llm_build_kv with n_tokens = T) on seeded inputs.

Every case compares the raw bits of the output AND of both whole caches: the KV store of the micro-batch (kv_store_batch_kernel) must write its
cells and no other.  The caches start as random finite f16 in every cell, cells past the micro-batch included (what kv_seq_rm leaves behind).

Launch paths (bamd_launch_attention_batch, impl 0 = the engine's choice, 1 = VALU only, 2 = matrix cores only):
  attn_batch_mfma_kernel<GQ, false>     head_dim 128, gq 1/2/4/8, padded length <= 512              test_mfma_short
  attn_batch_mfma_kernel<GQ, true>      ... beyond 512 positions (global scratch block)             test_mfma_long_positions, test_mfma_long_ld
  attn_batch_kernel<8|4|2>              gq 2/4/8 on the VALU; GQH halved while gqh * ld * 4 > 144 KB  test_valu_grid, test_valu_gqh_ladder, test_valu_long
  attn_fused_kernel<hd / 64>            gq 1/3/5/6/7 on the VALU, one workgroup per (head, token)    test_valu_grid, test_fused_gq3_long
"""
import os
import sys

import numpy as np
import pytest

import booster_amd
from bitcheck import assert_bits
from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import f64_softmax_search as ss  # noqa: E402

pytestmark = pytest.mark.gpu
THETA = 500000.0


def assert_cache(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d/%d cells differ, first at %d" % (what, bad.size, got.size, bad[0])


def rope_table(po, n_ctx, hd, pos0, T):
    """[n_ctx][hd] (cos, sin) table: the rows of the micro-batch's positions (the only ones the kernels may read), zeros elsewhere"""
    t = np.zeros((n_ctx, hd), np.float32)
    for p in range(pos0, pos0 + T):
        t[p] = po.rope_cache(p, hd, THETA)
    return t


def make_inputs(rng, H, Hkv, hd, n_ctx, T):
    Ekv = Hkv * hd
    kc = (rng.standard_normal(n_ctx * Ekv) * 0.7).astype(np.float16).view(np.uint16).copy()
    vc = rng.standard_normal(Ekv * n_ctx).astype(np.float16).view(np.uint16).copy()
    q = (rng.standard_normal((T, H * hd)) * 2).astype(np.float32)
    k = rng.standard_normal((T, Ekv)).astype(np.float32)
    v = rng.standard_normal((T, Ekv)).astype(np.float32)
    return q, k, v, kc, vc


def check(bamd, po, H, Hkv, hd, n_ctx, pos0, T, impl=0, lds=(0,), seed=0):
    """one micro-batch through the op at every ld of `lds`: each run == the oracle (output and both caches)"""
    rng = np.random.default_rng(seed or (H * 1000003 + Hkv * 10007 + hd * 101 + n_ctx * 7 + pos0 * 3 + T))
    q, k, v, kc, vc = make_inputs(rng, H, Hkv, hd, n_ctx, T)
    rope = rope_table(po, n_ctx, hd, pos0, T)
    kw, vw = kc.copy(), vc.copy()
    want = po.attention(q, k, v, kw, vw, rope, H, Hkv, hd, n_ctx, pos0, True)
    for ld in lds:
        kg, vg = kc.copy(), vc.copy()
        got = bamd.op_attention_batch(q, k, v, kg, vg, rope, H, Hkv, hd, n_ctx, pos0, impl=impl, ld=ld)
        what = "H %d Hkv %d hd %d n_ctx %d pos0 %d T %d impl %d ld %d" % (H, Hkv, hd, n_ctx, pos0, T, impl, ld)
        assert_cache(kg, kw, "K cache, " + what)
        assert_cache(vg, vw, "V cache, " + what)
        assert_bits(got, want, "out, " + what)


# ---- matrix-core kernel (impl 2): head_dim 128, 16 (token, head) columns per workgroup = tiles of 16 / gq tokens ----
@pytest.mark.parametrize("H,Hkv,n_ctx,pos0,T", [
    (4, 4, 256, 37, 17), (4, 4, 64, 0, 2),                 # gq 1: 16-token tiles, one ragged; the smallest micro-batch
    (8, 4, 320, 100, 15), (8, 4, 160, 131, 29),            # gq 2: 8-token tiles; n_ctx 160 = 32 mod 64, last cell filled
    (8, 2, 512, 45, 37), (4, 1, 128, 61, 7),               # gq 4: 4-token tiles; a sequence ending at n_kv % 64 == 32
    (16, 2, 256, 0, 3), (16, 2, 512, 430, 2), (16, 2, 224, 205, 19),   # gq 8: 2-token tiles; n_ctx 224 = 32 mod 64, last cell filled
])
def test_mfma_short(bamd, po, H, Hkv, n_ctx, pos0, T):
    check(bamd, po, H, Hkv, 128, n_ctx, pos0, T, impl=2)


@pytest.mark.parametrize("H,Hkv,n_ctx,pos0,T", [
    (2, 2, 1024, 700, 17),                                 # gq 1
    (4, 2, 1056, 1041, 15),                                # gq 2: n_ctx 1056 = 32 mod 64, last cell filled (n_kv % 64 == 32)
    (8, 2, 2048, 1500, 37),                                # gq 4: chunks of 512 positions in the P.V pass
    (16, 2, 1024, 600, 15),                                # gq 8
    (8, 2, 1024, 33, 512),                                 # gq 4, a full micro-batch of 512 tokens: tiles from 33 to 544 positions
    (4, 1, 4096, 3001, 3),                                 # gq 4, 4000 positions: eight chunks, pos0 odd
])
def test_mfma_long_positions(bamd, po, H, Hkv, n_ctx, pos0, T):
    check(bamd, po, H, Hkv, 128, n_ctx, pos0, T, impl=2)


@pytest.mark.parametrize("H,Hkv,n_ctx,pos0,T,lds", [
    (2, 2, 1024, 10, 17, (576, 1024)),                     # gq 1: a short sequence on the LONG kernel (ld > 512)
    (4, 2, 640, 90, 5, (640,)),                            # gq 2
    (8, 2, 1024, 0, 37, (0, 1024)),                        # gq 4: the engine's ld (short kernel) and a larger one (LONG): same bits
    (16, 2, 2048, 300, 9, (0, 512, 2048)),                 # gq 8
])
def test_mfma_long_ld(bamd, po, H, Hkv, n_ctx, pos0, T, lds):
    check(bamd, po, H, Hkv, 128, n_ctx, pos0, T, impl=2, lds=lds)


def test_mfma_declines(bamd, po):
    """impl 2 is an error (not a quiet fall-back) where the matrix-core kernel does not cover the shape; the host caches stay untouched"""
    for H, Hkv, hd, T in ((4, 1, 64, 5), (6, 2, 128, 5), (8, 1, 256, 5), (6, 2, 192, 5), (4, 1, 128, 1)):
        rng = np.random.default_rng(H + hd + T)
        n_ctx = 128
        q, k, v, kc, vc = make_inputs(rng, H, Hkv, hd, n_ctx, T)
        k0, v0 = kc.copy(), vc.copy()
        with pytest.raises(booster_amd.BamdError):
            bamd.op_attention_batch(q, k, v, kc, vc, rope_table(po, n_ctx, hd, 20, T), H, Hkv, hd, n_ctx, 20, impl=2)
        assert np.array_equal(kc, k0) and np.array_equal(vc, v0)


def test_bad_ld_is_refused(bamd, po):
    """ld must bound the padded sequence length (the kernels size their LDS rows / scratch columns by it) and be a multiple of 64"""
    H, Hkv, hd, n_ctx, pos0, T = 4, 1, 128, 1024, 600, 9
    rng = np.random.default_rng(5)
    q, k, v, kc, vc = make_inputs(rng, H, Hkv, hd, n_ctx, T)
    rope = rope_table(po, n_ctx, hd, pos0, T)
    for ld in (576, 672, 1088, 100):
        with pytest.raises(booster_amd.BamdError):
            bamd.op_attention_batch(q, k, v, kc, vc, rope, H, Hkv, hd, n_ctx, pos0, impl=0, ld=ld)


# ---- VALU kernels (impl 1): every ratio x every head_dim ----
@pytest.mark.parametrize("hd", [64, 128, 192, 256])
@pytest.mark.parametrize("gq", [1, 2, 3, 4, 5, 6, 7, 8])
def test_valu_grid(bamd, po, gq, hd):
    Hkv = 2 if gq <= 4 else 1
    check(bamd, po, gq * Hkv, Hkv, hd, 192, 41 + gq, 3 + 2 * gq, impl=1)


@pytest.mark.parametrize("gq,ld", [(8, 4608), (8, 4672), (8, 9216), (8, 9280), (8, 18432), (4, 9216), (4, 9280), (2, 18432)])
def test_valu_gqh_ladder(bamd, po, gq, ld):
    """each rung of attn_batch_kernel's GQH ladder (8 -> 4 -> 2 heads per workgroup while gqh * ld * 4 > 144 KB), chosen through ld on a short
    sequence, and the largest ld the launcher takes (18432: 2 x 72 KB)"""
    check(bamd, po, gq, 1, 64, 18432, 77, 11, impl=1, lds=(ld,))


@pytest.mark.parametrize("H,Hkv,hd,n_ctx,pos0,T", [
    (8, 2, 128, 4096, 3000, 9),                            # gq 4 at 3000 positions: what runs when the scratch block cannot be allocated
    (8, 1, 128, 8192, 7001, 5),                            # gq 8 at 7000 positions: ld 7040 -> four heads per workgroup
    (4, 2, 128, 2080, 2050, 30),                           # gq 2, n_ctx 2080 = 32 mod 64, last cell filled
    (2, 2, 64, 3072, 2500, 17),                            # gq 1: attn_fused_kernel
])
def test_valu_long(bamd, po, H, Hkv, hd, n_ctx, pos0, T):
    check(bamd, po, H, Hkv, hd, n_ctx, pos0, T, impl=1)


def test_fused_gq3_long(bamd, po):
    """gq 3 (Llama-3.2-3B) at head_dim 128: the launcher's choice is attn_fused_kernel once per (head, token) — on a long sequence"""
    check(bamd, po, 6, 2, 128, 4096, 3900, 17, impl=0)


# ---- the launcher's own choice (impl 0) at the models' head layouts ----
@pytest.mark.parametrize("name,H,Hkv,hd,n_ctx,pos0,T", [
    ("llama3-8b", 32, 8, 128, 640, 500, 40),               # gq 4, LONG (576 positions)
    ("llama3-8b-short", 32, 8, 128, 256, 0, 64),
    ("llama3-70b", 64, 8, 128, 256, 77, 16),               # gq 8
    ("llama3.2-3b", 24, 8, 128, 512, 200, 20),             # gq 3: per-head fused kernel
    ("llama3.2-1b", 32, 8, 64, 256, 60, 11),               # gq 4 at head_dim 64: attn_batch_kernel<4>
    ("llama2-7b", 32, 32, 128, 128, 0, 9),                 # gq 1
    ("llama2-7b-long", 8, 8, 128, 1024, 900, 21),          # gq 1, LONG (Hkv reduced: the ratio is what matters)
])
def test_model_layouts(bamd, po, name, H, Hkv, hd, n_ctx, pos0, T):
    check(bamd, po, H, Hkv, hd, n_ctx, pos0, T, impl=0)


@pytest.mark.parametrize("impl,H,Hkv,hd,n_ctx,pos0,T,ld", [
    (0, 8, 2, 128, 1024, 200, 13, 1024),                   # the engine's ld 256 (short MFMA) vs 1024 (LONG)
    (1, 8, 1, 128, 4096, 100, 7, 4096),                    # VALU: attn_batch_kernel<8> at both (8 x 4096 x 4 B = 128 KB)
    (1, 8, 1, 64, 8192, 100, 7, 8192),                     # VALU: attn_batch_kernel<8> at the engine's ld 128, <4> at 8192
    (0, 6, 2, 192, 2048, 30, 5, 2048),                     # per-head fused kernel
])
def test_larger_ld_same_bits(bamd, po, impl, H, Hkv, hd, n_ctx, pos0, T, ld):
    check(bamd, po, H, Hkv, hd, n_ctx, pos0, T, impl=impl, lds=(0, ld))


# ---- the constructed softmax row (tests/golden/f64_softmax_kat.npz): its 1 / sum rounds differently in the sequential and a tree order ----
@pytest.mark.parametrize("gq", [1, 2, 4, 8])
def test_constructed_softmax_row(bamd, po, gq):
    """head_dim 64 (scale 1/8), q = e_0, identity RoPE, K rows = score x e_0: the scores of the token at position 63 ARE the constructed row,
    and the batched VALU kernel's guard must send its denominator down the reference's sequential order (the micro-batch: positions 60 .. 63)"""
    skat = np.load(os.path.join(GOLDEN, "f64_softmax_kat.npz"))
    s = skat["scores"]
    H, Hkv, hd, n_ctx, pos0, T = gq, 1, 64, 64, 60, 4
    rng = np.random.default_rng(99 + gq)
    kc = np.zeros(n_ctx * hd, np.float16); kc[0::hd] = s.astype(np.float16)
    kc = kc.view(np.uint16).copy()
    vc = rng.standard_normal(hd * n_ctx).astype(np.float16).view(np.uint16).copy()
    q = np.zeros((T, H * hd), np.float32); q[:, 0::hd] = 1.0
    k = np.zeros((T, hd), np.float32); k[:, 0] = s[pos0:pos0 + T]
    v = rng.standard_normal((T, hd)).astype(np.float32)
    rope = np.tile(np.array([1.0, 0.0], np.float32), (n_ctx, hd // 2))
    kw, vw = kc.copy(), vc.copy()
    want = po.attention(q, k, v, kw, vw, rope, H, Hkv, hd, n_ctx, pos0, True)
    # the row is sensitive: the tree-order denominator gives other bits for the last token
    L = po.lib()
    e = ss.expf_table(po, s * np.float32(0.125))
    den = ss.denominators(e)
    p_tree = (e * np.float32(1.0 / den["tree"])).astype(np.float32)
    vt = vw.reshape(hd, n_ctx)
    alt = np.array([L.bo_dot_f16_f32_tinyblas(np.ascontiguousarray(vt[d]).ctypes.data, p_tree.ctypes.data, 64) for d in range(hd)], np.float32)
    assert not np.array_equal(alt.view(np.uint32), want[-1, :hd].view(np.uint32))
    got = bamd.op_attention_batch(q, k, v, kc, vc, rope, H, Hkv, hd, n_ctx, pos0, impl=1)
    assert_cache(kc, kw, "K cache"); assert_cache(vc, vw, "V cache")
    assert_bits(got, want, "out on the constructed row, gq %d" % gq)
