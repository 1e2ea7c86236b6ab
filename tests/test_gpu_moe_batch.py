"""GPU: the batched mixture-of-experts feed-forward of a prompt micro-batch (bamd_op_moe_ffn_batch: batched router | grouping | Q8_K | grouped gate/up | Q8_K of h |
grouped down | combine, bamd_moe_batch.hip) against llm_build_moe_ffn composed token by token as tests/test_gpu_moe_ops.py composes it, and whole models through
it against their own token-by-token evaluation.  Everything compared as bits."""
import numpy as np
import pytest

from bitcheck import EPS, assert_bits
from refmodel import Family, load_fixture, model_for, prompt_of
from test_gpu_moe_ops import Q4_K, Q5_K, Q6_K, experts, reference

pytestmark = pytest.mark.gpu
MOE = Family("moe", "moe_")


# the smallest shape | one pair past a full tile somewhere, mixed types, an odd record count in down | several tiles per expert, two softmax groups | most experts
# empty, more table entries than tiles | every token meets every expert: two full tiles and a tile of 4 each | eight 9.2 KB images in the down launch, past the
# 64 KB a launch gets unasked | all rows of x equal: two experts with 17 pairs, six with none, the same y row 17 times
@pytest.mark.parametrize("T,n_expert,n_used,E,F,tgu,td,same", [(2, 8, 2, 256, 256, Q4_K, Q4_K, False), (9, 8, 2, 512, 768, Q4_K, Q6_K, False),
                                                                (33, 16, 4, 256, 512, Q5_K, Q5_K, False), (5, 64, 8, 256, 256, Q4_K, Q4_K, False),
                                                                (20, 8, 8, 256, 256, Q4_K, Q4_K, False), (9, 8, 2, 256, 8192, Q4_K, Q4_K, False),
                                                                (17, 8, 2, 256, 256, Q4_K, Q4_K, True)])
def test_moe_ffn_batch(bamd, po, T, n_expert, n_used, E, F, tgu, td, same):
    rng = np.random.default_rng(9300 + T + n_expert * 16 + n_used + E + F)
    ge, ue, de = experts(rng, tgu, td, E, F, n_expert)
    gi = rng.standard_normal((n_expert, E)).astype(np.float32) * np.float32(2.0 / np.sqrt(E))
    x = rng.standard_normal((T, E)).astype(np.float32)
    if same:
        x[:] = x[0]
    nw = (1.0 + 0.1 * rng.standard_normal(E)).astype(np.float32)
    y, sel, w = bamd.op_moe_ffn_batch(gi, tgu, ge, ue, td, de, E, F, n_expert, n_used, x, nw, EPS)
    for t in range(1 if same else T):
        ry, rsel, rw = reference(po, gi, tgu, ge, ue, td, de, E, F, n_used, x[t], nw)
        for u in range(t, T if same else t + 1):
            assert sel[u].tolist() == rsel.tolist(), "token %d: selected experts" % u
            assert_bits(w[u], rw, "token %d: weights" % u)
            assert_bits(y[u], ry, "token %d: y" % u)


@pytest.mark.parametrize("cfg", ["tiny_mixtral", "tiny_moe16"])
def test_model_prompt_matches_token_by_token(bamd, cfg):
    """a 24-token prompt at n_past = 0 and a 7-token one behind it (below the 8 tokens from which a mixture-of-experts prompt is batched: the routed launches
    behind a batched prompt): the logits of the batched evaluation are those of set_prefill_batch(False), and only the batched one goes through the grouped launches"""
    path = model_for(MOE, cfg, load_fixture(MOE, cfg))
    m = bamd.Model(path)
    prompt = prompt_of(31, m.n_vocab)
    got = {}
    try:
        for batched in (False, True):
            bamd.set_prefill_batch(batched)
            ctx = bamd.Context(m, 64)
            runs = bamd.moe_batch_runs()
            got[batched] = [ctx.decode(prompt[:24], 0).copy(), ctx.decode(prompt[24:], 24).copy()]
            assert (bamd.moe_batch_runs() - runs > 0) == batched
            ctx.close()
    finally:
        bamd.set_prefill_batch(True)
        m.close()
    for k in range(2):
        assert_bits(got[True][k], got[False][k], "%s: logits behind prompt %d" % (cfg, k))
