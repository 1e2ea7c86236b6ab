"""GPU: the attention of a prefill micro-batch BEYOND the LDS bound (two score rows of ld floats no longer fit 144 KiB: ld > 18432), at op level, against the
oracle's bo_attention with n_tokens = T.  Inputs, oracle call and comparison are those of tests/test_gpu_attention_batch.py: raw bits of the output and of both
whole caches.

Launch paths beyond the bound (bamd_launch_attention_batch through bamd_attention_batch_plan):
  attn_batch_mfma_kernel<GQ, true>   head_dim 128, gq 1/2/4/8: score rows in the scratch block, P.V in chunks of 512 positions      impl 0 / 2
  attn_batch_gs_kernel<GQ>           every other shape (and impl 1): the VALU arithmetic with its rows in the scratch block         impl 0 / 1
both issued in token slices that reuse the one block when the micro-batch's rows exceed the budget.

The shapes are the smallest at which these kernels can still go wrong, not workload shapes; every case except the four long sequences puts a short sequence
(positions 77 .. 87) under a large ld, which costs nothing.
"""
import numpy as np
import pytest

import booster_amd
from bitcheck import assert_bits
from test_gpu_attention_batch import assert_cache, make_inputs, rope_table

pytestmark = pytest.mark.gpu


def run(bamd, po, H, Hkv, hd, n_ctx, pos0, T, cases, seed=0):
    """one micro-batch, the oracle once, then every (impl, ld, scratch_bytes) of `cases` through the op: each == the oracle; returns [(out, slices)]"""
    rng = np.random.default_rng(seed or (H * 1000003 + Hkv * 10007 + hd * 101 + n_ctx * 7 + pos0 * 3 + T))
    q, k, v, kc, vc = make_inputs(rng, H, Hkv, hd, n_ctx, T)
    rope = rope_table(po, n_ctx, hd, pos0, T)
    kw, vw = kc.copy(), vc.copy()
    want = po.attention(q, k, v, kw, vw, rope, H, Hkv, hd, n_ctx, pos0, True)
    res = []
    for impl, ld, sb in cases:
        kg, vg = kc.copy(), vc.copy()
        got, ns = bamd.op_attention_batch_ex(q, k, v, kg, vg, rope, H, Hkv, hd, n_ctx, pos0, impl=impl, ld=ld, scratch_bytes=sb)
        what = "H %d Hkv %d hd %d n_ctx %d pos0 %d T %d impl %d ld %d scratch %d (%d slices)" % (H, Hkv, hd, n_ctx, pos0, T, impl, ld, sb, ns)
        assert_cache(kg, kw, "K cache, " + what)
        assert_cache(vg, vw, "V cache, " + what)
        assert_bits(got, want, "out, " + what)
        res.append((got, ns))
    return res


# ---- the first refused ld, on a short sequence: each of these raised BamdError before the scratch-block kernels existed ----
FIRST = dict(n_ctx=18560, pos0=77, T=11)
LDS = (18496, 18560)


@pytest.mark.parametrize("gq", [1, 2, 4, 8])
def test_first_ld_beyond_the_lds_mfma(bamd, po, gq):
    run(bamd, po, gq, 1, 128, FIRST["n_ctx"], FIRST["pos0"], FIRST["T"], [(2, ld, 0) for ld in LDS])


@pytest.mark.parametrize("gq,hd", [(g, 64) for g in range(1, 9)] + [(g, h) for h in (128, 192, 256) for g in (3, 8)])
def test_first_ld_beyond_the_lds_valu(bamd, po, gq, hd):
    run(bamd, po, gq, 1, hd, FIRST["n_ctx"], FIRST["pos0"], FIRST["T"], [(1, ld, 0) for ld in LDS])


# ---- attn_batch_body's two instantiations on identical inputs ----
@pytest.mark.parametrize("gq,hd", [(2, 64), (4, 64), (8, 64), (8, 256)])
def test_lds_rows_equal_scratch_rows(bamd, po, gq, hd):
    """one micro-batch through impl 1 with its rows in LDS (ld 4608: attn_batch_kernel<gq>, no ladder step — 8 x 4608 x 4 B = 144 KiB) and in the scratch block
    (ld 18496: attn_batch_gs_kernel<gq>): each == the oracle (run()) and the two == each other.  Positions 77 .. 87 in n_kv = 96: a masked tail and a half-filled
    last 64-block"""
    (a, _), (b, _) = run(bamd, po, gq, 1, hd, FIRST["n_ctx"], FIRST["pos0"], FIRST["T"], [(1, 4608, 0), (1, 18496, 0)])
    assert_bits(a, b, "rows in LDS (ld 4608) vs rows in the scratch block (ld 18496)")


# ---- really long sequences ----
@pytest.mark.parametrize("H,Hkv,hd,n_ctx,pos0,T,impls", [
    (8, 2, 128, 18592, 18530, 37, (0, 1, 2)),              # n_ctx = 32 mod 64, last cell filled, T ragged against the token tile of 4
    (6, 2, 128, 20480, 19001, 9, (0, 1)),                  # gq 3: VALU only
    (2, 2, 64, 36928, 36900, 17, (0, 1)),                  # beyond ONE in-place LDS row of 144 KiB too
    (4, 1, 128, 131072, 131067, 5, (0, 1, 2)),             # index widths at 128 K positions (Hkv 1 keeps the host arrays at 32 MB each)
])
def test_long_sequences(bamd, po, H, Hkv, hd, n_ctx, pos0, T, impls):
    run(bamd, po, H, Hkv, hd, n_ctx, pos0, T, [(impl, 0, 0) for impl in impls])


def test_mfma_still_declines_beyond_the_lds(bamd, po):
    """impl 2 stays an error where the matrix-core kernel does not take the head shape"""
    H, Hkv, hd, n_ctx, pos0, T = 6, 2, 128, 18560, 77, 5
    q, k, v, kc, vc = make_inputs(np.random.default_rng(3), H, Hkv, hd, n_ctx, T)
    k0, v0 = kc.copy(), vc.copy()
    with pytest.raises(booster_amd.BamdError):
        bamd.op_attention_batch_ex(q, k, v, kc, vc, rope_table(po, n_ctx, hd, pos0, T), H, Hkv, hd, n_ctx, pos0, impl=2, ld=18560)
    assert np.array_equal(kc, k0) and np.array_equal(vc, v0)


# ---- slicing: a budget that forces at least three slices with a ragged last one gives the bits of the one-slice run (and the oracle's) ----
@pytest.mark.parametrize("H,Hkv,hd,n_ctx,pos0,T,impl,tiles", [
    (8, 2, 128, 18592, 18530, 37, 0, 4),                   # gq 4 on the matrix cores: 10 tiles of 4 tokens, 4 per slice -> 16 + 16 + 5 tokens
    (8, 2, 128, 18592, 18530, 37, 1, 15),                  # the same micro-batch on the VALU kernel: 37 tiles of one token, balanced 13 + 13 + 11
    (6, 2, 128, 20480, 19001, 9, 0, 2),                    # gq 3: tiles of one token, 2 + 2 + 2 + 2 + 1
])
def test_slices(bamd, po, H, Hkv, hd, n_ctx, pos0, T, impl, tiles):
    gq, ld = H // Hkv, min((pos0 + T + 63) // 64 * 64, (n_ctx + 63) // 64 * 64)
    one = bamd.attention_batch_plan(Hkv, gq, hd, T, ld, impl, 0)
    assert one is not None and one[1] == 1
    tt = 16 // gq if (impl != 1 and gq in (1, 2, 4, 8)) else 1
    ntiles = (T + tt - 1) // tt
    budget = one[2] // ntiles * tiles + 100                # `tiles` tiles and a little: not a multiple of the tile size
    tps, ns, sb = bamd.attention_batch_plan(Hkv, gq, hd, T, ld, impl, budget)
    assert ns >= 3 and T % tps != 0 and sb <= budget, (tps, ns, sb)
    (o1, n1), (o2, n2) = run(bamd, po, H, Hkv, hd, n_ctx, pos0, T, [(impl, 0, 0), (impl, 0, budget)])
    assert n1 == 1 and n2 == ns
    assert_bits(o2, o1, "sliced vs one slice")


def test_budget_below_one_tile_is_refused(bamd, po):
    H, Hkv, hd, n_ctx, pos0, T = 6, 2, 128, 18560, 77, 5
    q, k, v, kc, vc = make_inputs(np.random.default_rng(4), H, Hkv, hd, n_ctx, T)
    with pytest.raises(booster_amd.BamdError):
        bamd.op_attention_batch_ex(q, k, v, kc, vc, rope_table(po, n_ctx, hd, pos0, T), H, Hkv, hd, n_ctx, pos0, impl=0, ld=18560, scratch_bytes=4096)


# ---- ld invariance beyond the bound ----
@pytest.mark.parametrize("H,Hkv,hd,impl", [(8, 2, 128, 0), (6, 2, 128, 0), (4, 1, 64, 1), (2, 2, 256, 0)])
def test_ld_invariance(bamd, po, H, Hkv, hd, impl):
    """the same micro-batch with its rows at ld 18496 and at the padded n_ctx: same bits (run() compares both with the one oracle result)"""
    (a, _), (b, _) = run(bamd, po, H, Hkv, hd, 20448, 300, 13, [(impl, 18496, 0), (impl, 20480, 0)])      # n_ctx 20448 = 32 mod 64: padded 20480
    assert_bits(a, b, "ld 18496 vs 20480")


# ---- the 2 GiB rule ----
def test_layer_cache_of_2_gib_is_refused(bamd, tmp_path):
    """one layer's K (or V^T) cache is read through 32-bit byte offsets: n_ctx_pad x Hkv x hd x 2 >= 2^31 - 1 is an error with a message at context creation —
    it used to read zeros past the window silently — and nothing stays allocated"""
    import torch
    from booster_amd import gguf
    p = str(tmp_path / "wide_kv.gguf")
    gguf.write_synthetic_llama(p, E=1024, H=8, Hkv=8, L=1, F=256, V=256, seed=5)              # 1024 KV elements per position
    m = bamd.Model(p)
    free0 = torch.cuda.mem_get_info()[0]
    with pytest.raises(booster_amd.BamdError, match="2 GiB"):
        bamd.Context(m, 1048576)                                                                # x 1 Mi positions x 2 B = 2 GiB
    assert torch.cuda.mem_get_info()[0] >= free0 - (8 << 20)
    ctx = bamd.Context(m, 64)                                                                   # the model is still usable
    ctx.decode([3, 4, 5], 0)
    ctx.close(); m.close()
