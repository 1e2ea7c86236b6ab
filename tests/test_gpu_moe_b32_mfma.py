"""GPU: the grouped expert mat-muls of a mixture-of-experts prompt micro-batch on the matrix cores for experts of the 32-weight block formats
(booster_amd/csrc/bamd_moe_batch_b32_mfma.hip: behind set_prefill_moe AND the type's own family switch, set_prefill_q0 / _q1 / _nl; all default off) against
llm_build_moe_ffn composed token by token as tests/test_gpu_moe_b32_ops.py composes it, and whole models against the genuine reference's logits.  Everything
compared as bits; moe_batch_mfma_runs tells the matrix-core launches from the integer-dot ones (moe_batch_runs)."""
import os

import numpy as np
import pytest

from bitcheck import EPS, assert_bits, normed, silu_mul
from family_cases import FAMILIES, IQ4_NL, Q4_0, Q4_1, Q5_0, Q5_1, Q6_K, Q8_0, family
from float_ref import sgemm_rows
from refmodel import Family, check_step, load_fixture, model_for, prompt_of
from test_gpu_moe_ops import top_k_literal

pytestmark = pytest.mark.gpu
Q5_K = 13
MOE_B32 = Family("moe_b32", "moe_b32_")
SETTERS = {"moe": "set_prefill_moe", "q0": "set_prefill_q0", "q1": "set_prefill_q1", "nl": "set_prefill_nl"}


def switches(bamd, on):
    """the named switches on, the others at off; on=None: everything back to the process's environment default"""
    for name, setter in SETTERS.items():
        getattr(bamd, setter)(os.environ.get("BAMD_PREFILL_" + name.upper(), "")[:1] == "1" if on is None else name in on)


def fam(t):
    """a K-quant sibling takes the oracle, as family_cases gives it to Q6_K; the 32-weight block types their restatements"""
    return family(Q6_K) if t in (Q5_K, Q6_K) else FAMILIES[t]


def mul_mat(po, t, W, rows, K, x):
    return fam(t).ref(po, t, W, rows, K, np.ascontiguousarray(x, np.float32))


def reference(po, gi, tgu, ge, ue, td, de, E, F, n_used, x, nw):
    """reference() of tests/test_gpu_moe_b32_ops.py with a K-quant allowed on either side"""
    cur = normed(po, x, nw)
    probs = po.soft_max(sgemm_rows(gi, cur), None, 1.0)
    sel = top_k_literal(probs, n_used)
    s = np.float64(0.0)
    for v in probs[sel]:
        s += np.float64(v)
    w = probs[sel] / np.float32(s)
    gub, db = len(ge) // gi.shape[0], len(de) // gi.shape[0]
    acc = None
    for e, we in zip(sel, w):
        gate = mul_mat(po, tgu, ge[e * gub:(e + 1) * gub], F, E, cur)
        up = mul_mat(po, tgu, ue[e * gub:(e + 1) * gub], F, E, cur)
        down = mul_mat(po, td, de[e * db:(e + 1) * db], E, F, silu_mul(po, gate, up)) * we
        acc = down if acc is None else acc + down
    return x + acc, sel, w


def run(bamd, po, T, n_expert, n_used, E, F, tgu, td, same, on, mfma_runs):
    rng = np.random.default_rng(9800 + T + n_expert * 16 + n_used + E + F + tgu + td)
    ge, ue, de = fam(tgu).gen(tgu, E, F * n_expert, rng, 1.5), fam(tgu).gen(tgu, E, F * n_expert, rng, 1.5), fam(td).gen(td, F, E * n_expert, rng, 1.0)
    gi = rng.standard_normal((n_expert, E)).astype(np.float32) * np.float32(2.0 / np.sqrt(E))
    x = rng.standard_normal((T, E)).astype(np.float32)
    if same:
        x[:] = x[0]
    nw = (1.0 + 0.1 * rng.standard_normal(E)).astype(np.float32)
    try:
        switches(bamd, on)
        mfma, dot = bamd.moe_batch_mfma_runs(), bamd.moe_batch_runs()
        y, sel, w = bamd.op_moe_ffn_batch(gi, tgu, ge, ue, td, de, E, F, n_expert, n_used, x, nw, EPS)
        assert bamd.moe_batch_mfma_runs() == mfma + mfma_runs and bamd.moe_batch_runs() == dot + 1 - mfma_runs
    finally:
        switches(bamd, None)
    for t in range(1 if same else T):
        ry, rsel, rw = reference(po, gi, tgu, ge, ue, td, de, E, F, n_used, x[t], nw)
        for u in range(t, T if same else t + 1):
            assert sel[u].tolist() == rsel.tolist(), "token %d: selected experts" % u
            assert_bits(w[u], rw, "token %d: weights" % u)
            assert_bits(y[u], ry, "token %d: y" % u)


# one record (the prologue only, the buffer never cycles), tiles of 1 - 3 pairs | 40 pairs per expert: a full sub-tile of 32 and one of 8, even and odd record
# counts, Q8_0's two 16-byte pieces, qh bits | the summs chain, experts without pairs | a full tile and a tile of 6, so empty sub-tiles; both accumulator sets;
# sub-tiles of 16 | all rows of x equal: two experts with 64 + 1 pairs, two activation forms in one feed-forward | a new kernel and an existing one on one tile
# table, both ways
@pytest.mark.parametrize("T,n_expert,n_used,E,F,tgu,td,same", [(9, 8, 2, 256, 256, Q4_0, Q4_0, False), (40, 8, 8, 512, 768, Q5_0, Q8_0, False),
                                                                (33, 16, 4, 256, 512, Q4_1, Q5_1, False), (70, 8, 8, 256, 256, IQ4_NL, IQ4_NL, False),
                                                                (65, 8, 2, 256, 256, Q4_0, Q4_1, True), (9, 8, 2, 256, 512, IQ4_NL, Q5_K, False),
                                                                (9, 8, 2, 256, 512, Q6_K, Q8_0, False)])
def test_moe_ffn_batch_b32_on_the_matrix_cores(bamd, po, T, n_expert, n_used, E, F, tgu, td, same):
    run(bamd, po, T, n_expert, n_used, E, F, tgu, td, same, {"moe"} | {fam(t).switch for t in (tgu, td)} - {None}, 1)


def test_family_switch_off_keeps_the_integer_dot_kernels(bamd, po):
    """set_prefill_moe alone: Q4_0 experts need set_prefill_q0 as well, so the grouped integer-dot launches run, with the same bits"""
    run(bamd, po, 9, 8, 2, 256, 256, Q4_0, Q4_0, False, {"moe"}, 0)


@pytest.mark.parametrize("cfg,on", [("tiny_q4_0", {"moe", "q0"}), ("tiny_q5_1", {"moe", "q0", "q1"}), ("tiny_iq4nl", {"moe", "q0", "nl"})])
def test_model_prompt_on_the_matrix_cores(bamd, cfg, on):
    """the fixture's 24-token prompt with per-expert side tables under the smallest switch set its tensor types allow (Q8_0 attn_k / attn_v need q0 in all three):
    the reference's logits through the grouped matrix-core launches; a fresh model of the same file with the switches off builds no tables and leaves the counter still"""
    fx = load_fixture(MOE_B32, cfg)
    path = model_for(MOE_B32, cfg, fx)
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
