"""GPU: the grouped expert mat-muls of a mixture-of-experts prompt micro-batch on the matrix cores (booster_amd/csrc/bamd_moe_batch_mfma.hip, behind set_prefill_moe /
BAMD_PREFILL_MOE=1; default off) against llm_build_moe_ffn composed token by token as tests/test_gpu_moe_ops.py composes it, and whole models against the genuine
reference's logits.  Everything compared as bits; moe_batch_mfma_runs tells the matrix-core launches from the integer-dot ones (moe_batch_runs)."""
import os

import numpy as np
import pytest

from bitcheck import EPS, assert_bits
from refmodel import Family, check_step, load_fixture, model_for, prompt_of
from test_gpu_moe_ops import Q4_K, Q5_K, Q6_K, experts, reference

pytestmark = pytest.mark.gpu
MOE = Family("moe", "moe_")
SETTERS = {"moe": "set_prefill_moe", "q0": "set_prefill_q0"}


def switches(bamd, on):
    """the named switches on, the others at off; on=None: everything back to the process's environment default"""
    for name, setter in SETTERS.items():
        getattr(bamd, setter)(os.environ.get("BAMD_PREFILL_" + name.upper(), "")[:1] == "1" if on is None else name in on)


# one super-block (the prologue only), tiles of 1 - 3 pairs | every token meets every expert: a partial tile of 40 each, two and three super-blocks, both kernel
# layouts | Q5_K's high bits, experts without pairs | 70 pairs per expert: a full tile and a tile of 6 | all rows of x equal: two experts with 64 + 1 pairs
@pytest.mark.parametrize("T,n_expert,n_used,E,F,tgu,td,same", [(9, 8, 2, 256, 256, Q4_K, Q4_K, False), (40, 8, 8, 512, 768, Q4_K, Q6_K, False),
                                                                (33, 16, 4, 256, 512, Q5_K, Q5_K, False), (70, 8, 8, 256, 256, Q6_K, Q4_K, False),
                                                                (65, 8, 2, 256, 256, Q4_K, Q4_K, True)])
def test_moe_ffn_batch_on_the_matrix_cores(bamd, po, T, n_expert, n_used, E, F, tgu, td, same):
    rng = np.random.default_rng(9500 + T + n_expert * 16 + n_used + E + F)
    ge, ue, de = experts(rng, tgu, td, E, F, n_expert)
    gi = rng.standard_normal((n_expert, E)).astype(np.float32) * np.float32(2.0 / np.sqrt(E))
    x = rng.standard_normal((T, E)).astype(np.float32)
    if same:
        x[:] = x[0]
    nw = (1.0 + 0.1 * rng.standard_normal(E)).astype(np.float32)
    try:
        switches(bamd, {"moe"})
        mfma, dot = bamd.moe_batch_mfma_runs(), bamd.moe_batch_runs()
        y, sel, w = bamd.op_moe_ffn_batch(gi, tgu, ge, ue, td, de, E, F, n_expert, n_used, x, nw, EPS)
        assert bamd.moe_batch_mfma_runs() == mfma + 1 and bamd.moe_batch_runs() == dot
    finally:
        switches(bamd, None)
    for t in range(1 if same else T):
        ry, rsel, rw = reference(po, gi, tgu, ge, ue, td, de, E, F, n_used, x[t], nw)
        for u in range(t, T if same else t + 1):
            assert sel[u].tolist() == rsel.tolist(), "token %d: selected experts" % u
            assert_bits(w[u], rw, "token %d: weights" % u)
            assert_bits(y[u], ry, "token %d: y" % u)


@pytest.mark.parametrize("cfg,on", [("tiny_moe16", {"moe"}), ("tiny_mixtral", {"moe", "q0"})])
def test_model_prompt_on_the_matrix_cores(bamd, cfg, on):
    """the fixture's 24-token prompt with per-expert side tables: the reference's logits through the grouped matrix-core launches; a fresh model of the same file
    with the switches off builds no tables and leaves the counter still"""
    fx = load_fixture(MOE, cfg)
    path = model_for(MOE, cfg, fx)
    try:
        for tables in (True, False):
            switches(bamd, on if tables else set())
            m = bamd.Model(path)
            try:
                assert (m.prefill_aux_bytes() > 0) == tables
                ctx = bamd.Context(m, 64)
                runs = bamd.moe_batch_mfma_runs()
                check_step(fx, 0, ctx.decode(prompt_of(24, m.n_vocab), 0), "%s, tables %d" % (cfg, tables))
                assert (bamd.moe_batch_mfma_runs() > runs) == tables
                ctx.close()
            finally:
                m.close()
    finally:
        switches(bamd, None)


def test_eight_expert_recipe_needs_q0_too(bamd):
    """tiny_mixtral holds Q8_0 attn_k / attn_v: side tables are all-or-nothing per model, so set_prefill_moe alone builds none"""
    path = model_for(MOE, "tiny_mixtral", load_fixture(MOE, "tiny_mixtral"))
    try:
        switches(bamd, {"moe"})
        m = bamd.Model(path)
        try:
            assert m.prefill_aux_bytes() == 0
        finally:
            m.close()
    finally:
        switches(bamd, None)
