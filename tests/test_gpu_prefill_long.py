"""GPU, whole model at reduced width: prompt micro-batches BEYOND 18 432 positions run through the batched prefill kernels (their attention with its score rows in
the context's scratch block, bamd_attention_batch_plan) and give the bits of token-by-token evaluation.

As test_gpu_model.py::test_large_context_uses_the_same_kernels: a synthetic Q4_K model (E 1024, H 8, Hkv 2, two layers) opened with n_ctx 32768 on a
zero-initialised cache, the same in both modes.  The token-by-token reference of each model is computed once per module.
"""
import os

import numpy as np
import pytest

from booster_amd import gguf

pytestmark = pytest.mark.gpu
Q4_K = 12
N_CTX, POS0, T = 32768, 19000, 29
TOKS = [(7919 * i + 13) % 1024 for i in range(T)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def decode_pair(bamd, m):
    ctx = bamd.Context(m, N_CTX)
    l1 = ctx.decode(TOKS, POS0).copy()
    l2 = ctx.decode([9], POS0 + T).copy()
    ctx.close()
    return l1, l2


def batched_off_by_env():
    return os.environ.get("BAMD_ATTN_FUSED") == "0" or os.environ.get("BAMD_PREFILL_BATCH") == "0"


@pytest.fixture(scope="module")
def gq4(bamd, tmp_path_factory):
    """the model (gq 4: the LONG matrix-core attention kernel) and its token-by-token logits"""
    p = str(tmp_path_factory.mktemp("longctx") / "gq4.gguf")
    gguf.write_synthetic_llama(p, E=1024, H=8, Hkv=2, L=2, F=1792, V=1024, seed=23)
    m = bamd.Model(p)
    bamd.set_prefill_batch(0)
    try:
        ref = decode_pair(bamd, m)
    finally:
        bamd.set_prefill_batch(1)
    yield p, m, ref
    m.close()


def test_decode_beyond_18432_is_batched(bamd, gq4):
    """bamd_decode of 29 tokens at positions 19000 ..: the batched kernels run (the Q4_K matrix-core mat-mul counter moves: before the scratch-block kernels the
    call fell back to token by token and it did not) and the logits, and those of the next single token, are the token-by-token bits"""
    if batched_off_by_env():
        pytest.skip("the batched prefill kernels are switched off by the environment")
    _, m, ref = gq4
    ctx = bamd.Context(m, N_CTX)
    before = bamd.prefill_mfma_runs(Q4_K)
    l1 = ctx.decode(TOKS, POS0).copy()
    assert bamd.prefill_mfma_runs(Q4_K) > before, "the micro-batch at position %d did not run on the batched kernels" % POS0
    l2 = ctx.decode([9], POS0 + T).copy()
    ctx.close()
    assert np.array_equal(bits(l1), bits(ref[0])), "max |d| = %g" % np.abs(l1 - ref[0]).max()
    assert np.array_equal(bits(l2), bits(ref[1])), "max |d| = %g" % np.abs(l2 - ref[1]).max()


def test_stage_prefill_beyond_18432(bamd, gq4):
    """two layer-split stages: bamd_stage_prefill takes the micro-batch at n_past 19000 on every stage (it returned 2 = 'no batched kernels' there), and the last
    stage's logits are the single-stage bits"""
    import torch
    if batched_off_by_env():
        pytest.skip("the batched prefill kernels are switched off by the environment: bamd_stage_prefill reports 'no batched kernels' by design")
    p, _, ref = gq4
    stages = [bamd.Model(p, 0, 0, 1, True, False), bamd.Model(p, 0, 1, 2, False, True)]
    ctxs = [bamd.Context(s, N_CTX) for s in stages]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        stream = torch.cuda.current_stream().cuda_stream
        hid = torch.zeros(T * 1024, dtype=torch.float32, device="cuda")
        assert ctxs[0].stage_prefill(TOKS, T, POS0, None, hid.data_ptr(), False, stream)
        assert ctxs[1].stage_prefill(None, T, POS0, hid.data_ptr(), None, True, stream)
        lg = ctxs[1].stage_logits(stream)
    for c in ctxs:
        c.close()
    for s in stages:
        s.close()
    assert np.array_equal(bits(lg), bits(ref[0])), "max |d| = %g" % np.abs(lg - ref[0]).max()


def test_engine_slices_give_the_same_bits(bamd, gq4):
    """a scratch budget of 5 MiB: the plan of this micro-batch (8 tiles of 4 tokens, 2.3 MiB of score rows each) is four slices per layer"""
    _, m, ref = gq4
    tps, ns, sb = bamd.attention_batch_plan(2, 4, 128, T, (POS0 + T + 63) // 64 * 64, 0, 5 << 20)
    assert ns >= 3 and sb <= 5 << 20
    bamd.set_attn_scratch_mb(5)
    try:
        got = decode_pair(bamd, m)
    finally:
        bamd.set_attn_scratch_mb(0)
    for a, b in zip(got, ref):
        assert np.array_equal(bits(a), bits(b)), "max |d| = %g" % np.abs(a - b).max()


def test_gq3_model_beyond_18432(bamd, tmp_path):
    """a head shape only the VALU kernel serves (H 6, Hkv 2, head_dim 128: Llama-3.2-3B's ratio), in one slice and in three"""
    p = str(tmp_path / "gq3.gguf")
    gguf.write_synthetic_llama(p, E=768, H=6, Hkv=2, L=2, F=1792, V=1024, seed=29)
    m = bamd.Model(p)
    out = {}
    try:
        for mode, mb in ((0, 0), (1, 0), (1, 5)):
            bamd.set_prefill_batch(mode); bamd.set_attn_scratch_mb(mb)
            before = bamd.prefill_mfma_runs(Q4_K)
            out[mode, mb] = decode_pair(bamd, m)
            if mode == 1 and not batched_off_by_env():
                assert bamd.prefill_mfma_runs(Q4_K) > before
    finally:
        bamd.set_prefill_batch(1); bamd.set_attn_scratch_mb(0)
        m.close()
    assert bamd.attention_batch_plan(2, 3, 128, T, (POS0 + T + 63) // 64 * 64, 0, 5 << 20)[1] >= 3
    for key in ((1, 0), (1, 5)):
        for a, b in zip(out[key], out[0, 0]):
            assert np.array_equal(bits(a), bits(b)), "%r: max |d| = %g" % (key, np.abs(a - b).max())
