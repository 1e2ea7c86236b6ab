"""GPU: the matrix-core batched-prefill attention at head_dim 64 and at the ratios gq 3 / 5 / 6 / 7 (booster_amd/csrc/bamd_attention_mfma_ext.hip, behind
set_attn_mfma_ext / BAMD_ATTN_MFMA_EXT=1; default off), at op level against the oracle's bo_attention: raw bits of the output and of both whole caches.  Every case
runs with impl=2 (matrix cores only), which is an error for all of these shapes while the switch is off."""
import os

import numpy as np
import pytest

from bitcheck import assert_bits
from booster_amd import gguf
from conftest import GOLDEN
from test_gpu_attention_batch import assert_cache, make_inputs, rope_table, ss

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def ext_on(bamd):
    bamd.set_attn_mfma_ext(True)
    try:
        yield
    finally:
        bamd.set_attn_mfma_ext(os.environ.get("BAMD_ATTN_MFMA_EXT", "")[:1] == "1")


def check(bamd, po, H, Hkv, hd, n_ctx, pos0, T, lds=(0,), scratch_bytes=0):
    """one micro-batch through the op on the matrix cores at every ld of `lds`: each run == the oracle (output and both caches); returns the launches of the last"""
    rng = np.random.default_rng(H * 1000003 + Hkv * 10007 + hd * 101 + n_ctx * 7 + pos0 * 3 + T)
    q, k, v, kc, vc = make_inputs(rng, H, Hkv, hd, n_ctx, T)
    rope = rope_table(po, n_ctx, hd, pos0, T)
    kw, vw = kc.copy(), vc.copy()
    want = po.attention(q, k, v, kw, vw, rope, H, Hkv, hd, n_ctx, pos0, True)
    for ld in lds:
        kg, vg = kc.copy(), vc.copy()
        runs = bamd.attn_batch_mfma_runs()
        got, launches = bamd.op_attention_batch_ex(q, k, v, kg, vg, rope, H, Hkv, hd, n_ctx, pos0, impl=2, ld=ld, scratch_bytes=scratch_bytes)
        what = "H %d Hkv %d hd %d n_ctx %d pos0 %d T %d ld %d" % (H, Hkv, hd, n_ctx, pos0, T, ld)
        assert bamd.attn_batch_mfma_runs() == runs + launches, what
        assert_cache(kg, kw, "K cache, " + what)
        assert_cache(vg, vw, "V cache, " + what)
        assert_bits(got, want, "out, " + what)
    return launches


@pytest.mark.parametrize("H,Hkv,hd,n_ctx,pos0,T,lds", [
    (4, 4, 64, 64, 0, 2, (0,)),                            # head_dim 64, gq 1: the smallest micro-batch
    (8, 4, 64, 160, 131, 29, (0,)),                        # gq 2: n_ctx 160 = 32 mod 64, last cell filled
    (8, 2, 64, 512, 45, 37, (0,)),                         # gq 4: ragged tiles
    (8, 1, 64, 224, 205, 19, (0,)),                        # gq 8: n_ctx 224 = 32 mod 64
    (4, 1, 64, 2048, 1100, 9, (0,)),                       # LONG: an odd number of 64-blocks across the chunk boundaries
    (2, 2, 64, 1024, 600, 17, (0, 1024)),                  # short and LONG kernel: the same bits
    (6, 2, 128, 256, 59, 12, (0,)),                        # gq 3: tile 0 covers positions 59 .. 63, the would-be sixth token (a dead column) sits at 64
    (6, 2, 64, 256, 59, 12, (0,)),
    (5, 1, 128, 256, 61, 8, (0,)),                         # gq 5, 6, 7: ragged last tiles
    (6, 1, 64, 192, 62, 5, (0,)),
    (7, 1, 128, 192, 62, 5, (0,)),
    (6, 2, 128, 1024, 700, 11, (0,)),                      # gq 3, LONG: dead columns in the scratch block
    (6, 2, 64, 1088, 1041, 7, (0,)),
])
def test_ext_shapes(bamd, po, H, Hkv, hd, n_ctx, pos0, T, lds):
    assert check(bamd, po, H, Hkv, hd, n_ctx, pos0, T, lds=lds) == 1


def test_slices_at_an_odd_ratio(bamd, po):
    """gq 3 with a block of two tiles' worth (ld 640): five tiles of 5 tokens in three launches, the bits of one"""
    assert check(bamd, po, 6, 2, 128, 1024, 600, 23, scratch_bytes=2 * 2 * 16 * 640 * 4) == 3


@pytest.mark.parametrize("gq", [1, 3])
def test_constructed_softmax_row(bamd, po, gq):
    """the row of tests/golden/f64_softmax_kat.npz as test_gpu_attention_batch builds it (head_dim 64, q = e_0, identity RoPE, K rows = score x e_0, the
    micro-batch at positions 60 .. 63): its 1 / sum rounds differently in a tree order, so the guard's sequential fallback runs in the new instances"""
    s = np.load(os.path.join(GOLDEN, "f64_softmax_kat.npz"))["scores"]
    H, hd, n_ctx, pos0, T = gq, 64, 64, 60, 4
    rng = np.random.default_rng(99 + gq)
    kc = np.zeros(n_ctx * hd, np.float16); kc[0::hd] = s.astype(np.float16)
    kc = kc.view(np.uint16).copy()
    vc = rng.standard_normal(hd * n_ctx).astype(np.float16).view(np.uint16).copy()
    q = np.zeros((T, H * hd), np.float32); q[:, 0::hd] = 1.0
    k = np.zeros((T, hd), np.float32); k[:, 0] = s[pos0:pos0 + T]
    v = rng.standard_normal((T, hd)).astype(np.float32)
    rope = np.tile(np.array([1.0, 0.0], np.float32), (n_ctx, hd // 2))
    kw, vw = kc.copy(), vc.copy()
    want = po.attention(q, k, v, kw, vw, rope, H, 1, hd, n_ctx, pos0, True)
    e = ss.expf_table(po, s * np.float32(0.125))
    p_tree = (e * np.float32(1.0 / ss.denominators(e)["tree"])).astype(np.float32)
    alt = np.array([po.lib().bo_dot_f16_f32_tinyblas(np.ascontiguousarray(r).ctypes.data, p_tree.ctypes.data, 64) for r in vw.reshape(hd, n_ctx)], np.float32)
    assert not np.array_equal(alt.view(np.uint32), want[-1, :hd].view(np.uint32))
    got = bamd.op_attention_batch(q, k, v, kc, vc, rope, H, 1, hd, n_ctx, pos0, impl=2)
    assert_cache(kc, kw, "K cache"); assert_cache(vc, vw, "V cache")
    assert_bits(got, want, "out on the constructed row, gq %d" % gq)


@pytest.mark.parametrize("E,H,Hkv", [(256, 4, 1), (768, 6, 2)])      # head_dim 64 at gq 4; head_dim 128 at gq 3
def test_engine_prompt(bamd, tmp_path, E, H, Hkv):
    """a 40-token prompt of a two-layer model: one matrix-core attention launch per layer with the switch on, none with it off, the same logits"""
    p = str(tmp_path / "m.gguf")
    gguf.write_synthetic_llama(p, E=E, H=H, Hkv=Hkv, L=2, F=768, V=512, seed=37)
    m, out = bamd.Model(p), {}
    try:
        for on in (False, True):
            bamd.set_attn_mfma_ext(on)
            ctx, runs = bamd.Context(m, 64), bamd.attn_batch_mfma_runs()
            out[on] = ctx.decode([(31 * i + 7) % 512 for i in range(40)], 0).copy()
            ctx.close()
            assert bamd.attn_batch_mfma_runs() == runs + (2 if on else 0)
    finally:
        bamd.set_attn_mfma_ext(True)
        m.close()
    assert_bits(out[True], out[False], "logits, switch on against off")
