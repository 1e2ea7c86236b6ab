"""GPU: the grouped expert mat-muls of a mixture-of-experts prompt micro-batch on the matrix cores for Q3_K / Q2_K / IQ4_XS experts (bamd_moe_batch_kq_mfma.hip,
bamd_moe_batch_xs_mfma.hip: behind set_prefill_moe AND set_prefill_lowbit / _xs; all default off) against the grouped integer-dot launches of the same call with every
switch off, against llm_build_moe_ffn composed token by token from the CPU restatements (lowbit_ref, iq4xs_ref; the oracle for a Q4_K / Q5_K / Q6_K sibling), and whole
models against the genuine reference's logits.  Compared as bits; moe_batch_mfma_runs tells the matrix-core launches from the integer-dot ones (moe_batch_runs)."""
import os

import numpy as np
import pytest

import iq4xs_ref
from bitcheck import EPS, assert_bits, normed, silu_mul
from booster_amd.gguf import random_iq4_xs_tensor
from family_cases import FAMILIES, Q2_K, Q3_K, Q6_K, family
from float_ref import sgemm_rows
from refmodel import Family, check_step, load_fixture, model_for, prompt_of
from test_gpu_moe_ops import top_k_literal

pytestmark = pytest.mark.gpu
Q4_K, Q5_K, IQ4_XS = 12, 13, 23
MOE_KQ = Family("moe_kq", "moe_kq_")
SETTERS = {"moe": "set_prefill_moe", "q0": "set_prefill_q0", "lowbit": "set_prefill_lowbit", "xs": "set_prefill_xs"}
SWITCH = {Q2_K: "lowbit", Q3_K: "lowbit", IQ4_XS: "xs"}


def switches(bamd, on):
    """the named switches on, the others at off; on=None: everything back to the process's environment default"""
    for name, setter in SETTERS.items():
        getattr(bamd, setter)(os.environ.get("BAMD_PREFILL_" + name.upper(), "")[:1] == "1" if on is None else name in on)


def gen(t, K, rows, rng, amp):
    return random_iq4_xs_tensor(K, rows, rng, amp) if t == IQ4_XS else family(Q6_K).gen(t, K, rows, rng, amp)


def mul_mat(po, t, W, rows, K, x):
    x = np.ascontiguousarray(x, np.float32)      # Q2_K / Q3_K: lowbit_ref; Q4_K / Q5_K: the oracle, as family_cases gives it to Q6_K
    return iq4xs_ref.mul_mat(po, W, rows, K, x) if t == IQ4_XS else (FAMILIES[t] if t in (Q2_K, Q3_K) else family(Q6_K)).ref(po, t, W, rows, K, x)


def reference(po, gi, tgu, ge, ue, td, de, E, F, n_used, x, nw):
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
    rng = np.random.default_rng(9900 + T + n_expert * 16 + n_used + E + F + tgu + td)
    ge, ue, de = gen(tgu, E, F * n_expert, rng, 1.5), gen(tgu, E, F * n_expert, rng, 1.5), gen(td, F, E * n_expert, rng, 1.0)
    gi = rng.standard_normal((n_expert, E)).astype(np.float32) * np.float32(2.0 / np.sqrt(E))
    x = rng.standard_normal((T, E)).astype(np.float32)
    if same:
        x[:] = x[0]
    nw = (1.0 + 0.1 * rng.standard_normal(E)).astype(np.float32)
    got = []
    try:
        for sw, want in ((on, mfma_runs), (set(), 0)):         # the path under test, then the grouped integer-dot launches with every switch off
            switches(bamd, sw)
            mfma, dot = bamd.moe_batch_mfma_runs(), bamd.moe_batch_runs()
            got.append(bamd.op_moe_ffn_batch(gi, tgu, ge, ue, td, de, E, F, n_expert, n_used, x, nw, EPS))
            assert bamd.moe_batch_mfma_runs() == mfma + want and bamd.moe_batch_runs() == dot + 1 - want
    finally:
        switches(bamd, None)
    (y, sel, w), (y0, sel0, w0) = got
    assert np.array_equal(sel, sel0), "selected experts: switches on against off"
    assert_bits(w, w0, "weights: switches on against off")
    assert_bits(y, y0, "y: switches on against off")
    for t in [0] if same else range(T) if T == 9 else (0, T // 2, T - 1):       # beyond T = 9 three tokens: the low-bit restatement is slow
        ry, rsel, rw = reference(po, gi, tgu, ge, ue, td, de, E, F, n_used, x[t], nw)
        for u in range(T) if same else [t]:
            assert sel[u].tolist() == rsel.tolist(), "token %d: selected experts" % u
            assert_bits(w[u], rw, "token %d: weights" % u)
            assert_bits(y[u], ry, "token %d: y" % u)


# one super-block (prologue only, the clamps on from the first step), tiles of 1 - 3 pairs: dead slot tiles on every wave | the Q2_K recipe's pairing, a partial tile
# of 40 per expert, two and three super-blocks, the min term | experts without pairs, IQ4_XS's set copy across super-blocks | a full tile and a tile of 6, bsum16 from
# launch 5's records | all rows of x equal: two experts with 64 + 1 pairs | a new kernel and an existing one on one tile table, both ways | Q2_K in the down launch alone
@pytest.mark.parametrize("T,n_expert,n_used,E,F,tgu,td,same", [(9, 8, 2, 256, 256, Q3_K, Q3_K, False), (40, 8, 8, 512, 768, Q2_K, Q3_K, False),
                                                                (33, 16, 4, 256, 512, IQ4_XS, IQ4_XS, False), (70, 8, 8, 256, 256, Q2_K, Q2_K, False),
                                                                (65, 8, 2, 256, 256, Q3_K, Q3_K, True), (9, 8, 2, 256, 512, Q3_K, Q4_K, False),
                                                                (9, 8, 2, 256, 512, Q5_K, IQ4_XS, False), (9, 8, 2, 256, 512, Q4_K, Q2_K, False)])
def test_moe_ffn_batch_kq_on_the_matrix_cores(bamd, po, T, n_expert, n_used, E, F, tgu, td, same):
    run(bamd, po, T, n_expert, n_used, E, F, tgu, td, same, {"moe"} | {SWITCH[t] for t in (tgu, td) if t in SWITCH}, 1)


def test_family_switch_off_keeps_the_integer_dot_kernels(bamd, po):
    """set_prefill_moe alone: Q3_K experts need set_prefill_lowbit as well, so the grouped integer-dot launches run, with the same bits"""
    run(bamd, po, 9, 8, 2, 256, 256, Q3_K, Q3_K, False, {"moe"}, 0)


@pytest.mark.parametrize("cfg,on", [("tiny_q3_k_m", {"moe", "q0", "lowbit"}), ("tiny_q2_k", {"moe", "q0", "lowbit"}), ("tiny_iq4_xs", {"moe", "q0", "xs"})])
def test_model_prompt_on_the_matrix_cores(bamd, cfg, on):
    """the fixture's 24-token prompt under the smallest switch set its tensor types allow (Q8_0 attn_k / attn_v: q0), then a fresh model with the switches off"""
    fx = load_fixture(MOE_KQ, cfg)
    path = model_for(MOE_KQ, cfg, fx)
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
