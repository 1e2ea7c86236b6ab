"""GPU: the mixture-of-experts feed-forward (bamd_op_moe_ffn: router | routed gate/up | routed down + combine, bamd_moe.hip) against llm_build_moe_ffn composed
from pieces the suite already holds to the reference: the oracle's RMSNorm, soft_max, mul_mat_q and silu, float_ref's tinyBLAS<8> chain, and the argsort loops
of ggml.c:15185-15199 copied literally.  Selected ids, weights and y compared as bits."""
import numpy as np
import pytest

from bitcheck import EPS, assert_bits, normed, silu_mul
from booster_amd.gguf import random_kquant_tensor
from float_ref import sgemm_rows

pytestmark = pytest.mark.gpu
Q4_K, Q5_K, Q6_K = 12, 13, 14
BLOCK = {Q4_K: 144, Q5_K: 176, Q6_K: 210}


def top_k_literal(p, n_used):
    idx = list(range(len(p)))
    for j in range(len(p)):                                   # ggml_compute_forward_argsort_f32, GGML_SORT_ORDER_DESC
        for k in range(j + 1, len(p)):
            if p[idx[j]] < p[idx[k]]:
                idx[j], idx[k] = idx[k], idx[j]
    return np.array(idx[:n_used], np.int32)


def reference(po, gi, tgu, ge, ue, td, de, E, F, n_used, x, nw):
    cur = normed(po, x, nw)
    probs = po.soft_max(sgemm_rows(gi, cur), None, 1.0)
    sel = top_k_literal(probs, n_used)
    s = np.float64(0.0)
    for v in probs[sel]:
        s += np.float64(v)
    w = probs[sel] / np.float32(s)
    gub, db = E // 256 * BLOCK[tgu] * F, F // 256 * BLOCK[td] * E
    acc = None
    for e, we in zip(sel, w):
        gate = po.mul_mat_q(tgu, ge[e * gub:(e + 1) * gub], F, E, cur)[0]
        up = po.mul_mat_q(tgu, ue[e * gub:(e + 1) * gub], F, E, cur)[0]
        down = po.mul_mat_q(td, de[e * db:(e + 1) * db], E, F, silu_mul(po, gate, up))[0] * we
        acc = down if acc is None else acc + down
    return x + acc, sel, w


def experts(rng, tgu, td, E, F, n_expert):
    return (random_kquant_tensor(tgu, E, F * n_expert, rng, 1.5), random_kquant_tensor(tgu, E, F * n_expert, rng, 1.5),
            random_kquant_tensor(td, F, E * n_expert, rng, 1.0))


def check(bamd, po, gi, tgu, ge, ue, td, de, E, F, n_used, x, nw, what):
    y, sel, w = bamd.op_moe_ffn(gi, tgu, ge, ue, td, de, E, F, gi.shape[0], n_used, x, nw, EPS)
    ry, rsel, rw = reference(po, gi, tgu, ge, ue, td, de, E, F, n_used, x, nw)
    assert sel.tolist() == rsel.tolist(), what + ": selected experts"
    assert_bits(w, rw, what + ": weights")
    assert_bits(y, ry, what + ": y")
    return rsel


# one record per row | mixed types, an odd record count in down | the single-slot product | two softmax groups, four waves combining | the limits |
# eight Q8_K blobs of F = 8192 in the down launch: 8 x 9.2 KB = 74 KB of LDS, past the 64 KB a launch gets without asking
@pytest.mark.parametrize("n_expert,n_used,E,F,tgu,td", [(8, 2, 256, 256, Q4_K, Q4_K), (8, 2, 512, 768, Q4_K, Q6_K), (8, 1, 256, 256, Q4_K, Q4_K),
                                                          (16, 4, 256, 512, Q5_K, Q5_K), (64, 8, 256, 256, Q4_K, Q4_K), (8, 8, 256, 8192, Q4_K, Q4_K)])
def test_moe_ffn(bamd, po, n_expert, n_used, E, F, tgu, td):
    rng = np.random.default_rng(9100 + n_expert * 16 + n_used + E + F)
    ge, ue, de = experts(rng, tgu, td, E, F, n_expert)
    gi = rng.standard_normal((n_expert, E)).astype(np.float32) * np.float32(2.0 / np.sqrt(E))
    x = rng.standard_normal(E).astype(np.float32)
    nw = (1.0 + 0.1 * rng.standard_normal(E)).astype(np.float32)
    check(bamd, po, gi, tgu, ge, ue, td, de, E, F, n_used, x, nw, "%d experts, %d used" % (n_expert, n_used))


@pytest.mark.parametrize("router", ["all_equal", "two_at_the_maximum", "equal_across_the_cut"])
def test_moe_router_ties(bamd, po, router):
    """ties resolve as the exchange sort resolves them: a swap carries an entry past its equals, so the order is not a stable sort's"""
    E = F = 256
    rng = np.random.default_rng(77)
    ge, ue, de = experts(rng, Q4_K, Q4_K, E, F, 8)
    x = rng.standard_normal(E).astype(np.float32)
    nw = np.ones(E, np.float32)
    cur = normed(po, x, nw)
    gi = np.zeros((8, E), np.float32)
    if router != "all_equal":
        gi[:] = rng.standard_normal((8, E)).astype(np.float32) * np.float32(0.002)
        hi, lo = cur * np.float32(4.0 / E), cur * np.float32(2.0 / E)
        if router == "two_at_the_maximum":
            gi[2] = hi; gi[5] = hi
        else:
            gi[0] = lo; gi[1] = lo; gi[3] = hi                # the maximum behind two equal runners-up: the swap that brings it forward sends row 0 behind row 1
    sel = check(bamd, po, gi, Q4_K, ge, ue, Q4_K, de, E, F, 2, x, nw, router)
    assert sel.tolist() == {"all_equal": [0, 1], "two_at_the_maximum": [2, 5], "equal_across_the_cut": [3, 1]}[router]
