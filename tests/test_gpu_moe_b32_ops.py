"""GPU: the mixture-of-experts feed-forward with experts of the 32-weight block formats (bamd_moe_b32.h: routed gate/up, routed down + combine; bamd_moe_batch_b32.hip:
the grouped prompt mat-muls).  op_moe_ffn against llm_build_moe_ffn composed as tests/test_gpu_moe_ops.py composes it, the per-type mat-mul from the restatements
family_cases holds to the reference (the oracle for a K-quant); op_moe_ffn_batch against op_moe_ffn token by token.  Ids, weights and y compared as bits."""
import numpy as np
import pytest

from bitcheck import EPS, assert_bits, normed, silu_mul
from family_cases import FAMILIES, IQ4_NL, Q4_0, Q4_1, Q5_0, Q5_1, Q8_0
from float_ref import sgemm_rows
from booster_amd.gguf import random_kquant_tensor
from test_gpu_moe_ops import top_k_literal

pytestmark = pytest.mark.gpu
Q5_K = 13


def gen(t, K, rows, rng, amp):
    return random_kquant_tensor(t, K, rows, rng, amp) if t == Q5_K else FAMILIES[t].gen(t, K, rows, rng, amp)


def mul_mat(po, t, W, rows, K, x):
    x = np.ascontiguousarray(x, np.float32)
    return po.mul_mat_q(t, W, rows, K, x)[0] if t == Q5_K else FAMILIES[t].ref(po, t, W, rows, K, x)


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


def inputs(seed, n_expert, E, F, tgu, td, T):
    rng = np.random.default_rng(seed)
    ge, ue, de = gen(tgu, E, F * n_expert, rng, 1.5), gen(tgu, E, F * n_expert, rng, 1.5), gen(td, F, E * n_expert, rng, 1.0)
    gi = rng.standard_normal((n_expert, E)).astype(np.float32) * np.float32(2.0 / np.sqrt(E))
    x = rng.standard_normal((T, E)).astype(np.float32)
    nw = (1.0 + 0.1 * rng.standard_normal(E)).astype(np.float32)
    return gi, ge, ue, de, x, nw


# one record per row | an odd record count in down, ring depth 1 | a single slot | the summs chain, four waves combining | two activation forms in one feed-forward |
# b32 gate/up into a K-quant down | eight images of F = 8192 in the down launch: 8 x 9 KB = 72 KB of LDS, past the 64 KB a launch gets without asking
@pytest.mark.parametrize("n_expert,n_used,E,F,tgu,td", [(8, 2, 256, 256, Q4_0, Q4_0), (8, 2, 512, 768, Q5_0, Q8_0), (8, 1, 256, 256, Q8_0, Q8_0),
                                                          (16, 4, 256, 512, Q4_1, Q5_1), (8, 2, 256, 512, Q4_0, Q4_1), (8, 2, 256, 512, IQ4_NL, Q5_K),
                                                          (8, 8, 256, 8192, Q4_0, Q4_0),
                                                          # E = 1024: the ring of four records in gate/up, what every real model takes (E % 1024 == 0), per family
                                                          (8, 2, 1024, 256, Q8_0, Q5_0), (8, 2, 1024, 256, Q5_1, Q4_1), (8, 2, 1024, 256, IQ4_NL, IQ4_NL)])
def test_moe_ffn_b32(bamd, po, n_expert, n_used, E, F, tgu, td):
    gi, ge, ue, de, x, nw = inputs(9500 + n_expert * 16 + n_used + E + F + tgu + td, n_expert, E, F, tgu, td, 1)
    y, sel, w = bamd.op_moe_ffn(gi, tgu, ge, ue, td, de, E, F, n_expert, n_used, x[0], nw, EPS)
    ry, rsel, rw = reference(po, gi, tgu, ge, ue, td, de, E, F, n_used, x[0], nw)
    assert sel.tolist() == rsel.tolist(), "selected experts"
    assert_bits(w, rw, "weights")
    assert_bits(y, ry, "y")


# T = 1: six experts without a pair | 9 | 37: 74 pairs over 8 experts, so an expert holds more than one tile of 8 and partial tiles exist
@pytest.mark.parametrize("T", [1, 9, 37])
@pytest.mark.parametrize("tgu,td", [(Q4_0, Q4_0), (Q5_1, Q5_1), (IQ4_NL, Q5_K)])
def test_moe_ffn_batch_b32(bamd, tgu, td, T):
    n_expert, n_used, E, F = 8, 2, 256, 512
    gi, ge, ue, de, x, nw = inputs(9600 + T + tgu + td, n_expert, E, F, tgu, td, T)
    runs = bamd.moe_batch_runs()
    y, sel, w = bamd.op_moe_ffn_batch(gi, tgu, ge, ue, td, de, E, F, n_expert, n_used, x, nw, EPS)
    assert bamd.moe_batch_runs() > runs
    for t in range(T):
        ry, rsel, rw = bamd.op_moe_ffn(gi, tgu, ge, ue, td, de, E, F, n_expert, n_used, x[t], nw, EPS)
        assert sel[t].tolist() == rsel.tolist(), "token %d: selected experts" % t
        assert_bits(w[t], rw, "token %d: weights" % t)
        assert_bits(y[t], ry, "token %d: y" % t)


# F = 18432: eight images of 72 blocks are past the LDS of a CU, so the tile table is built for 4 pairs and both grouped launches take their instances of 4 pairs;
# E = 512 and F have even record counts: the ring of two records in gate/up and in down
@pytest.mark.parametrize("tgu,td", [(Q4_0, Q8_0), (Q5_1, Q4_1), (IQ4_NL, IQ4_NL)])
def test_moe_ffn_batch_b32_tiles_of_four(bamd, tgu, td):
    n_expert, n_used, E, F, T = 8, 2, 512, 18432, 9
    gi, ge, ue, de, x, nw = inputs(9700 + tgu + td, n_expert, E, F, tgu, td, T)
    y, sel, w = bamd.op_moe_ffn_batch(gi, tgu, ge, ue, td, de, E, F, n_expert, n_used, x, nw, EPS)
    for t in range(T):
        ry, rsel, rw = bamd.op_moe_ffn(gi, tgu, ge, ue, td, de, E, F, n_expert, n_used, x[t], nw, EPS)
        assert sel[t].tolist() == rsel.tolist(), "token %d: selected experts" % t
        assert_bits(w[t], rw, "token %d: weights" % t)
        assert_bits(y[t], ry, "token %d: y" % t)
