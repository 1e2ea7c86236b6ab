"""GPU: the mixture-of-experts feed-forward with unquantised experts, F16 / F32 / BF16 (bamd_moe_flt.hip: routed gate/up, routed down + combine;
bamd_moe_batch_flt.hip: the grouped prompt mat-muls).  op_moe_ffn against llm_build_moe_ffn composed as tests/test_gpu_moe_b32_ops.py composes it, the expert
mat-mul from tests/moe_flt_ref.py (held to the reference by tests/test_moe_flt_ref.py; the oracle for a K-quant); op_moe_ffn_batch against op_moe_ffn token by
token.  Ids, weights and y compared as bits."""
import numpy as np
import pytest

from bitcheck import EPS, assert_bits, normed, silu_mul
from float_ref import BF16, F16, F32, sgemm_rows
from moe_flt_ref import mul_mat_id_rows
from booster_amd.gguf import random_float_tensor, random_kquant_tensor
from test_gpu_moe_ops import top_k_literal

pytestmark = pytest.mark.gpu
Q5_K = 13
# the largest F the routed down launch takes for two slots: 2 images of F values (2 or 4 bytes each) + the product tile of 2 x 8 row-groups in 160 KiB of LDS
F_MAX = {F16: 40704, BF16: 40704, F32: 20224}


def gen(t, K, rows, n_expert, rng, amp):
    """n_expert matrices [rows][K]; a large one is drawn once and repeated for every expert (the routed launches still stream the selected expert's own copy)"""
    draw = (lambda r: random_kquant_tensor(t, K, r, rng, amp)) if t == Q5_K else (lambda r: random_float_tensor(t, K, r, rng, amp))
    return draw(rows * n_expert) if rows * K < (1 << 21) else np.tile(draw(rows), n_expert)


def mul_mat(po, t, W, rows, K, x):
    x = np.ascontiguousarray(x, np.float32)
    return po.mul_mat_q(t, W, rows, K, x)[0] if t == Q5_K else mul_mat_id_rows(t, W, rows, K, x)


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
        h = silu_mul(po, gate, up)
        assert np.abs(h).max() < 65504.0, "h would overflow f16"
        down = mul_mat(po, td, de[e * db:(e + 1) * db], E, F, h) * we
        acc = down if acc is None else acc + down
    assert np.isfinite(acc).all()
    return x + acc, sel, w, np.abs(h).max()


def inputs(seed, n_expert, E, F, tgu, td, T, amp=1.0):
    rng = np.random.default_rng(seed)
    ge, ue, de = gen(tgu, E, F, n_expert, rng, 1.5 * amp), gen(tgu, E, F, n_expert, rng, 1.5 * amp), gen(td, F, E, n_expert, rng, 1.0)
    gi = rng.standard_normal((n_expert, E)).astype(np.float32) * np.float32(2.0 / np.sqrt(E))
    x = rng.standard_normal((T, E)).astype(np.float32)
    nw = (1.0 + 0.1 * rng.standard_normal(E)).astype(np.float32)
    return gi, ge, ue, de, x, nw


# one chunk per row, the smallest shape, per type | a single slot | an odd chunk count in down, four waves combining | E a multiple of 1024, what real models have |
# type_gu and type_d independent, a float gate/up into a K-quant down | h in the f16-subnormal range: the down launch's conversion meets subnormals and ties |
# the largest F each type's down launch accepts for two slots: the limit the loader checks
@pytest.mark.parametrize("n_expert,n_used,E,F,tgu,td,amp", [(8, 2, 256, 256, F16, F16, 1.0), (8, 2, 256, 256, F32, F32, 1.0), (8, 2, 256, 256, BF16, BF16, 1.0),
                                                              (8, 1, 256, 256, F16, F16, 1.0), (16, 4, 256, 768, F32, F32, 1.0),
                                                              (8, 2, 1024, 512, F16, F16, 1.0), (8, 2, 1024, 512, BF16, BF16, 1.0),
                                                              (8, 2, 256, 512, BF16, F16, 1.0), (8, 2, 256, 512, F16, Q5_K, 1.0),
                                                              (8, 2, 256, 512, F16, F16, 1e-3),
                                                              (8, 2, 256, F_MAX[F16], F16, F16, 1.0), (8, 2, 256, F_MAX[BF16], BF16, BF16, 1.0), (8, 2, 256, F_MAX[F32], F32, F32, 1.0)])
def test_moe_ffn_flt(bamd, po, n_expert, n_used, E, F, tgu, td, amp):
    gi, ge, ue, de, x, nw = inputs(9800 + n_expert * 16 + n_used + E + F + tgu + td, n_expert, E, F, tgu, td, 1, amp)
    y, sel, w = bamd.op_moe_ffn(gi, tgu, ge, ue, td, de, E, F, n_expert, n_used, x[0], nw, EPS)
    ry, rsel, rw, hmax = reference(po, gi, tgu, ge, ue, td, de, E, F, n_used, x[0], nw)
    if amp < 1.0:
        assert 0.0 < hmax < 6.1e-5, "h is meant to lie in the f16-subnormal range"
    assert sel.tolist() == rsel.tolist(), "selected experts"
    assert_bits(w, rw, "weights")
    assert_bits(y, ry, "y")


def batch_against_token_by_token(bamd, tgu, td, E, F, T, seed):
    n_expert, n_used = 8, 2
    gi, ge, ue, de, x, nw = inputs(seed, n_expert, E, F, tgu, td, T)
    runs = bamd.moe_batch_runs()
    y, sel, w = bamd.op_moe_ffn_batch(gi, tgu, ge, ue, td, de, E, F, n_expert, n_used, x, nw, EPS)
    assert bamd.moe_batch_runs() > runs
    for t in range(T):
        ry, rsel, rw = bamd.op_moe_ffn(gi, tgu, ge, ue, td, de, E, F, n_expert, n_used, x[t], nw, EPS)
        assert sel[t].tolist() == rsel.tolist(), "token %d: selected experts" % t
        assert_bits(w[t], rw, "token %d: weights" % t)
        assert_bits(y[t], ry, "token %d: y" % t)


# T = 1: six experts without a pair | 9 | 37: 74 pairs over 8 experts, so an expert holds more than one tile of 8 and partial tiles exist
@pytest.mark.parametrize("T", [1, 9, 37])
@pytest.mark.parametrize("tgu,td", [(F16, F16), (BF16, BF16), (F32, Q5_K)])
def test_moe_ffn_batch_flt(bamd, tgu, td, T):
    batch_against_token_by_token(bamd, tgu, td, 256, 512, T, 9900 + T + tgu + td)


# F = 10240: eight f16 images of F are 160 KiB and, with the pair ids and gate values beside them, past the LDS of a CU, so the tile table is built for 4 pairs and
# both grouped launches take their instances of 4 pairs (ring of two chunks: E = 512 and F have even chunk counts)
def test_moe_ffn_batch_flt_tiles_of_four(bamd):
    batch_against_token_by_token(bamd, F16, F16, 512, 10240, 9, 9950)
